#!/usr/bin/env python
"""Where the cycles of a K1s13 slab body go (maxsim_stream13_kernel, `make -C colpali_amd/csrc trace`): per wave of the first 64
and of the last 64 workgroups of the grid (the oldest and the youngest), s_memtime ticks from the top of the slab body to the return
of its vmcnt wait ("wait") and over the rest of the body ("rest": operand reads, decode, MFMAs, folds, the cursor), summed over the
wave's slabs, the wave's lifetime and start in s_memrealtime ticks (100 MHz) and its hardware id (HW_ID, XCC_ID): s_memtime counts
shader clocks, so the two clocks together give the clock the wave ran at (MSIM_STREAM_TRACE_PTR debug knob).

    python tools/trace_stream.py [orders, default 4] [queries of 32 tokens, default 4] [priorities, default 0] [decodes, default 1]

The orders are maxsim_stream.hip's ORDER (MSIM_STREAM_ORDER): 0 = the pieces handed to the hook and clustered by the compiler,
1 = all eight in front of the wait, 2 = one piece pinned per NU MFMAs, 3 = four in front of the wait and four behind the first
row group's reads, 4 = one piece pinned per NU / 2 MFMAs.  The priorities are maxsim_stream13.hip's PRIO (MSIM_STREAM13_PRIO):
0 = none, 1 = flipped per document, 2 = per 32 slabs, 3 = static; the decodes its DECODE (MSIM_STREAM13_DECODE): 0 = or3, 1 = bfi.
Priorities and decodes other than the shipped ones exist at the shipped order only.  One process per combination: the library reads
the knobs once.

Per run: one line over all traced waves, one per generation (first / last workgroups), and -- where waves of two traced workgroups
report the same XCD, shader engine, CU and SIMD -- one for the older and one for the younger partner of those pairs, with how many
pairs report wave slots of opposite parity (what PRIO takes its phase from)."""
import os, subprocess, sys

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE_WGS, WORDS = 64, 6                                     # maxsim_stream.hip: kStreamTraceWgs, kStreamTraceWords
WAVES = 2 * TRACE_WGS * 4


def describe(tag, rows, t_first, slots=None):
    if slots is not None:
        tag += " (wave slots " + ", ".join(f"{v}: {int((slots == v).sum())}" for v in sorted(set(int(x) for x in slots))) + ")"
    wait, rest, n, real, start = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 5]
    print(f"    {tag}: {len(rows)} waves, {int(n.sum())} slabs ({float(n.mean()):.0f} per wave); start {float((start - t_first).mean()) / 100.0:.0f} us, "
          f"lifetime {float(real.mean()) / 100.0:.0f} us ({float(real.min()) / 100.0:.0f}-{float(real.max()) / 100.0:.0f}), "
          f"end {float((start + real - t_first).mean()) / 100.0:.0f} us ({float((start + real - t_first).max()) / 100.0:.0f} the last); "
          f"ticks per slab: wait {float((wait / n).mean()):.1f}, rest {float((rest / n).mean()):.1f}", flush=True)


def child(nq):
    sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..")))
    import torch
    os.environ.setdefault("COLPALI_AMD_LIB", os.path.join(HERE, "_ab", "libmaxsim_trace.so"))
    dev = torch.device("cuda:0")
    trace = torch.zeros(WAVES * WORDS, dtype=torch.int64, device=dev)
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
    raw = trace.view(WAVES, WORDS).cpu()
    gen = torch.arange(WAVES) >= TRACE_WGS * 4                  # False: a wave of the first workgroups, True: of the last
    keep = raw[:, 2] > 0
    raw, gen = raw[keep], gen[keep]
    t = raw.double()
    wait, rest, n, real = t[:, 0], t[:, 1], t[:, 2], t[:, 3]
    mhz = float(((wait + rest) / (real / 100.0)).mean())          # body ticks per microsecond of the wave's lifetime (document epilogues not in the ticks)
    share = wait / (wait + rest)
    knobs = ", ".join(f"{k} {os.environ.get(v, 'shipped')}" for k, v in (("order", "MSIM_STREAM_ORDER"), ("prio", "MSIM_STREAM13_PRIO"),
                                                                         ("decode", "MSIM_STREAM13_DECODE")))
    print(f"{knobs}, {nq} x 32 tokens: {a.elapsed_time(e):.3f} ms (scan + list launch), {len(t)} waves, "
          f"{int(n.sum())} slabs; ticks per slab: wait {float((wait / n).mean()):.1f}, rest {float((rest / n).mean()):.1f}; "
          f"share of the wait: mean {float(share.mean()):.3f}, min {float(share.min()):.3f}, max {float(share.max()):.3f}; "
          f"wave lifetime {float(real.mean()) / 100.0:.0f} us, body ticks per us {mhz:.0f}", flush=True)
    t_first = float(t[:, 5].min())
    hw = raw[:, 4]
    for g, tag in ((False, "first workgroups"), (True, "last workgroups")):
        if bool((gen == g).any()):
            describe(tag, t[gen == g], t_first, (hw & 15)[gen == g])
    # partners: the same XCD, shader engine / array, CU and SIMD, different workgroups
    slot, simd, cu, sh_se, xcc, wg = hw & 15, (hw >> 4) & 3, (hw >> 8) & 15, (hw >> 12) & 15, (hw >> 32) & 15, hw >> 40
    where = {}
    for i in range(len(raw)):
        where.setdefault((int(xcc[i]), int(sh_se[i]), int(cu[i]), int(simd[i])), []).append(i)
    slots = sorted(set(int(s) for s in slot))
    print(f"    wave slots seen: {slots}; traced waves on {len(where)} SIMDs, {sum(1 for v in where.values() if len(v) > 1)} of them with more than one", flush=True)
    older, younger, opposite, pairs = [], [], 0, 0
    for v in where.values():
        v = [i for i in v]
        if len(v) != 2 or int(wg[v[0]]) == int(wg[v[1]]):
            continue
        v.sort(key=lambda i: float(t[i, 5]))
        pairs += 1
        opposite += int((int(slot[v[0]]) ^ int(slot[v[1]])) & 1)
        older.append(v[0]); younger.append(v[1])
    if pairs:
        print(f"    {pairs} pairs of traced waves share a SIMD; slots of opposite parity in {opposite}; "
              f"the older partner is a wave of the first workgroups in {sum(1 for i in older if not bool(gen[i]))}, "
              f"its slot is even in {sum(1 for i in older if not int(slot[i]) & 1)}", flush=True)
        describe("older partners", t[older], t_first)
        describe("younger partners", t[younger], t_first)
    else:
        print("    no two traced workgroups share a SIMD: generations only", flush=True)


if __name__ == "__main__":
    if os.environ.get("TRACE_STREAM_CHILD"):
        child(int(sys.argv[1]))
        sys.exit(0)
    orders = sys.argv[1] if len(sys.argv) > 1 else "4"
    nq = sys.argv[2] if len(sys.argv) > 2 else "4"
    prios = sys.argv[3] if len(sys.argv) > 3 else "0"
    decodes = sys.argv[4] if len(sys.argv) > 4 else "1"
    for o in orders.split(","):
        for d in decodes.split(","):
            for p in prios.split(","):
                env = dict(os.environ, TRACE_STREAM_CHILD="1", MSIM_STREAM_ORDER=o, MSIM_STREAM13_PRIO=p, MSIM_STREAM13_DECODE=d)
                rc = subprocess.run([sys.executable, os.path.abspath(__file__), nq], env=env, timeout=300).returncode
                if rc != 0:           # a fault, an abort or a time limit: start nothing more on the GPU
                    sys.exit(rc)
