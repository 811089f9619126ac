"""The live corpus (colpali_amd.LiveCorpus, msim_live_*) on the headline shard; one JSON object on stdout (not part of bench.py).

    python tools/bench_live.py [--out FILE] [--docs 125000 --doc-len 1024] [--steps 5] [--bounce-mb 256] [--legs compact,search,add]

Legs, each timed with device events (compact: one call per fresh set of deletions; the others after a warm-up):
  * stream: a device-to-device copy of 4 GiB, the run's own ceiling for a read + write stream (bytes read + written / time).
  * compact: compact() after deleting 1 %, 10 % and 50 % of the pages uniformly at random.  Bound = the bytes the bounce scheme
    must move (2 reads + 2 writes of every row that changes place; rows below the first deleted page do not move) / 8 TB/s.  Beside
    it: pack_passages of the surviving pages from host memory (the only alternative without a live corpus), on a sample of
    --repack-docs pages and scaled by bytes.  The result is checked: offsets and a sample of pages against the survivors.
  * search: LiveCorpus.search with nothing deleted against ShardedRetriever.search on the same rows, alternating, at 4 and 1000
    queries of 32 tokens; the mask's estimate is n_q x n x 8 B / 8 TB/s plus one launch.
  * add: add() of 1000 pages of --doc-len rows from a host list against the H2D floor of their bytes at 56 GB/s.
search and add report the median over --steps and, as *_spread_ms, max - min of those identical calls.
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
from tools.bench_rerank import timed  # noqa: E402

H2D_GBS = 56.0


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stream_leg(dev):
    n = 4 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    t = timed(lambda: dst.copy_(src), 5, 2)
    t["GBps_read_plus_write"] = 2 * n / t["median_ms"] / 1e6
    return t


def compact_leg(amd, corpus, frac, bounce_bytes, repack_docs, seed):
    n, doc_len = len(corpus), int(corpus.lengths[0])
    row_bytes = corpus.blob.shape[1] * corpus.blob.element_size()
    live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=bounce_bytes)
    g = torch.Generator().manual_seed(seed)
    gone = torch.randperm(n, generator=g)[:max(1, int(n * frac))].sort().values
    alive = np.ones(n, dtype=bool)
    alive[gone.numpy()] = False
    sample = torch.from_numpy(np.flatnonzero(alive)[:: max(1, n // 64)])
    keep = [corpus.blob[int(s) * doc_len:(int(s) + 1) * doc_len].clone() for s in sample]
    live.delete(gone.tolist())
    ms = once_ms(live.compact)
    live.check()
    new_off = np.concatenate([[0], np.cumsum(np.where(alive, doc_len, 0))])
    assert np.array_equal(live.view().offsets.cpu().numpy(), new_off) and live.rows_used == int(new_off[-1])
    for s, page in zip(sample.tolist(), keep):
        assert torch.equal(live.blob[new_off[s]:new_off[s + 1]], page), f"page {s} differs after compaction"
    moved_rows = int(alive[int(gone[0]):].sum()) * doc_len
    bound_ms = 4.0 * moved_rows * row_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
    out = {"deleted": int(gone.numel()), "first_deleted": int(gone[0]), "moved_rows": moved_rows, "compact_ms": ms,
           "bound_ms": bound_ms, "share_of_bound": bound_ms / ms, "moved_GBps": 4.0 * moved_rows * row_bytes / ms / 1e6}
    del live
    torch.cuda.empty_cache()
    # the alternative at the parent commit: pack the survivors again from host memory (a sample, scaled by bytes)
    k = min(repack_docs, int(alive.sum()))
    host = [torch.empty((doc_len, corpus.blob.shape[1]), dtype=corpus.blob.dtype).normal_() for _ in range(k)]
    amd.pack_passages(host, corpus.device, batch_size=None)
    t0 = time.perf_counter()
    amd.pack_passages(host, corpus.device, batch_size=None)
    torch.cuda.synchronize()
    sample_ms = (time.perf_counter() - t0) * 1e3
    out["repack_sample_docs"], out["repack_sample_ms"] = k, sample_ms
    out["repack_scaled_ms"] = sample_ms * int(alive.sum()) / k
    return out


def search_leg(amd, corpus, n_q, q_len, dev, steps):
    live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=1 << 20)
    ref = amd.ShardedRetriever(corpus)
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    a, b = live.search(pq, 10), ref.search(pq, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lv, rf = [], []
    for _ in range(steps):                               # alternating, same run
        lv.append(once_ms(lambda: live.search(pq, 10)))
        rf.append(once_ms(lambda: ref.search(pq, 10)))
    scores = torch.zeros((n_q, len(corpus)), dtype=torch.float32, device=dev)
    mask = timed(lambda: amd.live.mask_scores(scores, live.alive[:len(live)]), 10, 3)
    lv.sort(), rf.sort()
    est = n_q * len(corpus) * 8 / (HBM_PEAK_GBS * 1e9) * 1e3
    return {"live_ms": lv[len(lv) // 2], "static_ms": rf[len(rf) // 2], "difference_ms": lv[len(lv) // 2] - rf[len(rf) // 2],
            "live_spread_ms": lv[-1] - lv[0], "static_spread_ms": rf[-1] - rf[0], "mask_alone_ms": mask["median_ms"],
            "mask_estimate_ms": est}


def add_leg(amd, dev, n_pages, doc_len, steps):
    pages = [torch.empty((doc_len, 128), dtype=torch.bfloat16).normal_() for _ in range(n_pages)]
    nbytes = n_pages * doc_len * 256
    live = amd.LiveCorpus((steps + 2) * n_pages * doc_len, (steps + 2) * n_pages, dev)
    ms = []
    for i in range(steps + 2):
        t0 = time.perf_counter()
        live.add(pages)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[2:])
    floor = nbytes / (H2D_GBS * 1e9) * 1e3
    return {"pages": n_pages, "bytes": nbytes, "add_ms": ms[len(ms) // 2], "add_spread_ms": ms[-1] - ms[0], "h2d_floor_ms": floor,
            "share_of_floor": floor / ms[len(ms) // 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bounce-mb", default="256")
    ap.add_argument("--repack-docs", type=int, default=2000)
    ap.add_argument("--legs", default="stream,compact,search,add")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_live", "docs": args.docs, "doc_len": args.doc_len, "hbm_peak_GBps": HBM_PEAK_GBS}
    if "stream" in legs:
        res["stream"] = stream_leg(dev)
        torch.cuda.empty_cache()
    if "add" in legs:
        res["add"] = add_leg(amd, dev, 1000, args.doc_len, args.steps)
        torch.cuda.empty_cache()
    if legs & {"compact", "search"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        if "search" in legs:
            res["search"] = {str(n): search_leg(amd, corpus, n, args.q_len, dev, args.steps if n <= 8 else 3) for n in (4, 1000)}
            torch.cuda.empty_cache()
        if "compact" in legs:
            res["compact"] = {}
            for mb in [int(x) for x in args.bounce_mb.split(",")]:
                res["compact"][f"bounce_{mb}MiB"] = {f"{int(f * 100)}%": compact_leg(amd, corpus, f, mb << 20, args.repack_docs, 7)
                                                    for f in (0.01, 0.10, 0.50)}
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
