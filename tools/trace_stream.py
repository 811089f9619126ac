#!/usr/bin/env python
"""Where the cycles of a K1s13 slab body go (maxsim_stream13_kernel, `make -C colpali_amd/csrc trace`): per wave of the first 64
workgroups, s_memtime ticks from the top of the slab body to the return of its vmcnt wait ("wait") and over the rest of the body
("rest": operand reads, decode, MFMAs, folds, the cursor), summed over the wave's slabs, and the wave's lifetime in s_memrealtime
ticks (100 MHz): s_memtime counts shader clocks, so the two together give the clock the wave ran at (MSIM_STREAM_TRACE_PTR debug knob).

    python tools/trace_stream.py [orders, default 0,4] [queries of 32 tokens, default 4]

The orders are maxsim_stream.hip's ORDER (MSIM_STREAM_ORDER): 0 = the pieces handed to the hook and clustered by the compiler,
1 = all eight in front of the wait, 2 = one piece pinned per NU MFMAs, 3 = four in front of the wait and four behind the first
row group's reads, 4 = one piece pinned per NU / 2 MFMAs.  One process per order: the library reads the knob once."""
import os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
WAVES = 64 * 4


def child(nq):
    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    os.environ.setdefault("COLPALI_AMD_LIB", os.path.join(HERE, "_ab", "libmaxsim_trace.so"))
    dev = torch.device("cuda:0")
    trace = torch.zeros(WAVES * 4, dtype=torch.int64, device=dev)
    os.environ["MSIM_STREAM_TRACE_PTR"] = str(trace.data_ptr())
    import bench, colpali_amd as amd
    docs, doc_len = int(os.environ.get("AB_DOCS", "125000")), int(os.environ.get("AB_DOC_LEN", "1024"))
    corpus = bench.make_shard(docs, doc_len, dev, 1234)
    q = bench.make_queries(nq, 32, dev, 3)
    out = torch.empty((nq, docs), dtype=torch.float32, device=dev)
    assert corpus.pack13() and corpus._pack13 is not None
    for _ in range(3):
        amd.maxsim_scores(q, corpus, out=out)
    torch.cuda.synchronize()
    trace.zero_()
    a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(); amd.maxsim_scores(q, corpus, out=out); e.record(); torch.cuda.synchronize()
    t = trace.view(WAVES, 4).cpu().double()
    t = t[t[:, 2] > 0]
    wait, rest, n, real = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    mhz = float(((wait + rest) / (real / 100.0)).mean())          # body ticks per microsecond of the wave's lifetime (document epilogues not in the ticks)
    share = wait / (wait + rest)
    print(f"order {os.environ.get('MSIM_STREAM_ORDER', 'shipped')}, {nq} x 32 tokens: {a.elapsed_time(e):.3f} ms (scan + list launch), {len(t)} waves, "
          f"{int(n.sum())} slabs; ticks per slab: wait {float((wait / n).mean()):.1f}, rest {float((rest / n).mean()):.1f}; "
          f"share of the wait: mean {float(share.mean()):.3f}, min {float(share.min()):.3f}, max {float(share.max()):.3f}; "
          f"wave lifetime {float(real.mean()) / 100.0:.0f} us, body ticks per us {mhz:.0f}", flush=True)


if __name__ == "__main__":
    if os.environ.get("TRACE_STREAM_CHILD"):
        child(int(sys.argv[1]))
        sys.exit(0)
    orders = sys.argv[1] if len(sys.argv) > 1 else "0,4"
    nq = sys.argv[2] if len(sys.argv) > 2 else "4"
    for o in orders.split(","):
        env = dict(os.environ, TRACE_STREAM_CHILD="1", MSIM_STREAM_ORDER=o)
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), nq], env=env, timeout=300).returncode
        if rc != 0:           # a fault, an abort or a time limit: start nothing more on the GPU
            sys.exit(rc)
