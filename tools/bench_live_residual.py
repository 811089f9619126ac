"""The live compressed shard (colpali_amd.LiveResidualCorpus, msim_res_append, msim_res_live_compact) on the headline shard; one JSON
object on stdout (not part of bench.py, run by no test).

    python tools/bench_live_residual.py [--out FILE] [--docs 125000 --doc-len 1024] [--k 1024] [--reps 5] [--legs encode,add,compact,search]

Everything runs in one process, the two sides of every comparison alternate call by call, and next to every difference stands the
spread (max - min) of the repeated identical calls of each side.  Timed with device events after a warm-up of every shape.
  * encode (a): the device-resident pages of the whole shard -> codes + residuals at the tail of the arrays, the fused entry
    (msim_res_append) against the composition msim_cent_encode_docs + msim_res_encode_docs writing to the same place, bits 2 and 4.
    The outputs are compared bit for bit first.
  * add (b): add() of 1000 host pages of --doc-len rows against the H2D floor of their bytes at 56 GB/s (pinned memory).
  * compact (c): compact() after deleting 1 / 10 / 50 % of the pages uniformly at random, against the bytes the move needs at
    8 TB/s: 4 x (16 bits + 2) per row that changes place.  The result is checked: offsets, and a sample of pages.
  * search (d): search over the live shard with nothing deleted against the same search over the frozen ResidualCorpus (a
    ShardedRetriever over the same arrays), for candidates= and for prefilter=index.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_legs.common import HBM_PEAK_GBS, make_queries, make_shard  # noqa: E402
from tools.bench_live import H2D_GBS, once_ms  # noqa: E402


def stats(ms):
    s = sorted(ms)
    return {"median_ms": s[len(s) // 2], "min_ms": s[0], "max_ms": s[-1], "spread_ms": s[-1] - s[0], "n": len(s)}


def alternate(fa, fb, reps, warm=1):
    """a and b, call by call in one process: (stats of a, stats of b, median difference a - b)"""
    for _ in range(warm):
        fa(), fb()
    a, b = [], []
    for _ in range(reps):
        a.append(once_ms(fa))
        b.append(once_ms(fb))
    sa, sb = stats(a), stats(b)
    return sa, sb, sa["median_ms"] - sb["median_ms"]


def make_codec(amd, corpus, k, bits, dev):
    """centroids: k seeded rows of the shard; cutoffs / weights trained on the residuals of a sample (build time, not timed)"""
    g = torch.Generator().manual_seed(11)
    rows = int(corpus.blob.shape[0])
    C = corpus.blob.index_select(0, torch.randint(0, rows, (k,), generator=g).to(dev)).contiguous()
    pick = torch.randint(0, rows, (1 << 16,), generator=g).to(dev)
    sample = corpus.blob.index_select(0, pick)
    near = (sample.float() @ C.float().T).argmax(dim=1)
    cut, w = amd.train_residual_codec(sample.float() - C.float().index_select(0, near), bits)
    return C, cut.to(dev), w.to(dev)


def encode_leg(amd, corpus, k, bits, dev, reps):
    L = amd._lib.lib()
    n, rows = len(corpus), int(corpus.blob.shape[0])
    doc_len = int(corpus.lengths[0])
    C, cut, _ = make_codec(amd, corpus, k, bits, dev)
    row0 = 4096                                          # a multiple of 8: the composition needs a 16-byte aligned code pointer
    outs = [(torch.zeros((row0 + rows,), dtype=torch.int16, device=dev), torch.zeros((row0 + rows, 16 * bits), dtype=torch.uint8, device=dev))
            for _ in range(2)]
    dt, st = amd._lib.dtype_code(corpus.blob.dtype), None

    def fused():
        codes, res = outs[0]
        rc = L.msim_res_append(dt, corpus.blob.data_ptr(), corpus.offsets.data_ptr(), n, rows, 128, doc_len, C.data_ptr(), k, cut.data_ptr(),
                               bits, codes.data_ptr(), res.data_ptr(), row0, row0 + rows, None, amd._lib.current_stream_handle(dev))
        assert rc == 0, L.msim_last_error()

    def composed():
        codes, res = outs[1]
        s = amd._lib.current_stream_handle(dev)
        rc = L.msim_cent_encode_docs(dt, corpus.blob.data_ptr(), corpus.offsets.data_ptr(), n, rows, 128, doc_len, C.data_ptr(), k,
                                     codes.data_ptr() + 2 * row0, None, s)
        assert rc == 0, L.msim_last_error()
        rc = L.msim_res_encode_docs(dt, corpus.blob.data_ptr(), rows, 128, codes.data_ptr() + 2 * row0, C.data_ptr(), k, cut.data_ptr(), bits,
                                    res.data_ptr() + 16 * bits * row0, s)
        assert rc == 0, L.msim_last_error()

    def cent_only():
        rc = L.msim_cent_encode_docs(dt, corpus.blob.data_ptr(), corpus.offsets.data_ptr(), n, rows, 128, doc_len, C.data_ptr(), k,
                                     outs[1][0].data_ptr() + 2 * row0, None, amd._lib.current_stream_handle(dev))
        assert rc == 0, L.msim_last_error()

    fused(), composed()
    torch.cuda.synchronize()
    same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    sf, sc, diff = alternate(fused, composed, reps, warm=0)
    so = stats([once_ms(cent_only) for _ in range(reps)])
    flop = 2.0 * rows * k * 128
    out = {"rows": rows, "k": k, "bits": bits, "bit_identical": bool(same), "fused": sf, "composed": sc, "fused_minus_composed_ms": diff,
           "cent_encode_alone": so, "fused_mfma_TFLOPs": flop / sf["median_ms"] / 1e9}
    del outs
    torch.cuda.empty_cache()
    return out


def add_leg(amd, corpus, k, bits, dev, n_pages, doc_len, reps):
    C, cut, w = make_codec(amd, corpus, k, bits, dev)
    pages = [torch.empty((doc_len, 128), dtype=torch.bfloat16).normal_() for _ in range(n_pages)]
    nbytes = n_pages * doc_len * 256
    live = amd.LiveResidualCorpus(C, cut, w, bits, (reps + 2) * n_pages * doc_len, (reps + 2) * n_pages)
    ms = []
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        live.add(pages)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    s = stats(ms[2:])
    floor = nbytes / (H2D_GBS * 1e9) * 1e3
    return {"pages": n_pages, "bytes": nbytes, "bits": bits, "ingest_rows": live.ingest_rows, "add": s, "h2d_floor_ms": floor,
            "share_of_floor": floor / s["median_ms"]}


def filled(amd, corpus, codec, bits, **kw):
    C, cut, w = codec
    n, doc_len = len(corpus), int(corpus.lengths[0])
    live = amd.LiveResidualCorpus(C, cut, w, bits, int(corpus.blob.shape[0]), n, **kw)
    live.add(corpus.blob.view(n, doc_len, 128))
    return live


def compact_leg(amd, corpus, codec, bits, frac, seed):
    n, doc_len = len(corpus), int(corpus.lengths[0])
    live = filled(amd, corpus, codec, bits)
    g = torch.Generator().manual_seed(seed)
    gone = torch.randperm(n, generator=g)[:max(1, int(n * frac))].sort().values
    alive = np.ones(n, dtype=bool)
    alive[gone.numpy()] = False
    sample = np.flatnonzero(alive)[:: max(1, n // 64)]
    keep = [(live.codes.view(torch.int16)[int(s) * doc_len:(int(s) + 1) * doc_len].clone(),
             live.residuals[int(s) * doc_len:(int(s) + 1) * doc_len].clone()) for s in sample]
    live.delete(gone.tolist())
    ms = once_ms(live.compact)
    live.check()
    new_off = np.concatenate([[0], np.cumsum(np.where(alive, doc_len, 0))])
    assert np.array_equal(live.view().offsets.cpu().numpy(), new_off) and live.rows_used == int(new_off[-1])
    for s, (c, r) in zip(sample.tolist(), keep):
        assert torch.equal(live.codes.view(torch.int16)[new_off[s]:new_off[s + 1]], c), f"codes of page {s} differ after compaction"
        assert torch.equal(live.residuals[new_off[s]:new_off[s + 1]], r), f"residuals of page {s} differ after compaction"
    moved_rows = int(alive[int(gone[0]):].sum()) * doc_len
    nbytes = 4.0 * moved_rows * (16 * bits + 2)
    bound_ms = nbytes / (HBM_PEAK_GBS * 1e9) * 1e3
    return {"bits": bits, "deleted": int(gone.numel()), "moved_rows": moved_rows, "compact_ms": ms, "bound_ms": bound_ms,
            "share_of_bound": bound_ms / ms, "moved_GBps": nbytes / ms / 1e6, "bounce_bytes": live.bounce_bytes}


def search_leg(amd, corpus, codec, bits, dev, n_q, q_len, m, reps):
    live = filled(amd, corpus, codec, bits, bounce_bytes=1 << 20)
    frozen = live.view()
    ref = amd.ShardedRetriever(frozen)
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    cand = torch.randint(0, len(corpus), (n_q, m), generator=torch.Generator().manual_seed(5)).to(dev)
    out = {"bits": bits, "n_q": n_q, "m": m}
    for name, kw_live, kw_ref in (("candidates", dict(candidates=cand), dict(candidates=cand)),
                                  ("prefilter", dict(prefilter=live.index, n_candidates=m), dict(prefilter=frozen.index, n_candidates=m))):
        a, b = live.search(pq, 10, **kw_live), ref.search(pq, 10, **kw_ref)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        sl, sr, diff = alternate(lambda: live.search(pq, 10, **kw_live), lambda: ref.search(pq, 10, **kw_ref), reps)
        out[name] = {"live": sl, "frozen": sr, "live_minus_frozen_ms": diff}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--legs", default="encode,add,compact,search")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live_residual.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_live_residual", "docs": args.docs, "doc_len": args.doc_len, "k": args.k, "hbm_peak_GBps": HBM_PEAK_GBS}
    corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)

    def save():
        res["wall_s"] = time.perf_counter() - t0
        if args.out:
            with open(args.out, "w") as f:
                f.write(json.dumps(res) + "\n")

    if "encode" in legs:
        res["encode"] = {f"bits{b}": encode_leg(amd, corpus, args.k, b, dev, args.reps) for b in (2, 4)}
        save()
    if "add" in legs:
        res["add"] = add_leg(amd, corpus, args.k, 2, dev, 1000, args.doc_len, args.reps)
        save()
    if legs & {"compact", "search"}:
        for b in (2, 4):
            codec = make_codec(amd, corpus, args.k, b, dev)
            if "compact" in legs:
                res.setdefault("compact", {})[f"bits{b}"] = {f"{int(f * 100)}%": compact_leg(amd, corpus, codec, b, f, 7) for f in (0.01, 0.10, 0.50)}
                save()
            if "search" in legs:
                res.setdefault("search", {})[f"bits{b}"] = search_leg(amd, corpus, codec, b, dev, 4, args.q_len, 1024, args.reps)
                save()
            torch.cuda.empty_cache()
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
