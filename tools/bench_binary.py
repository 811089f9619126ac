"""The 1-bit sign index (msim_bin_*, colpali_amd.BinaryIndex) on the headline shard; one JSON object on stdout (not part of
bench.py).

    python tools/bench_binary.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--legs build,stage1,two_stage,recall]

Legs, each timed with device events after a warm-up; the variants of a leg ALTERNATE call by call inside one timed loop, and every
figure is the median with its range:
  * build: BinaryIndex.build of the shard beside Int8Index.build; bound = (the shard's rows read once + the codes written) / 8 TB/s.
  * stage1: binary_scores at 4 and 1000 queries of 32 tokens on the full shard, beside int8_scores and the exact scan
    (maxsim_scores) of the same shard.  Bounds of binary_scores: memory (rows x 16 + n_q n_d 4) B / 8 TB/s, matrix cores
    2 n_q 32 rows 128 / 5 POPS.
  * two_stage: ShardedRetriever.search(prefilter=<BinaryIndex>, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside
    the same search through the Int8Index and the exact search.
  * recall: recall@10 against the exact search on the planted 10 000-page set of tools/bench_fde.py:planted_pages, for the binary
    index beside the Int8Index of the full pages and the bf16 pooled prefilter (HierarchicalTokenPooler(pool_factor=3)).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_legs.common import HBM_PEAK_GBS, make_queries, make_shard  # noqa: E402
from tools.bench_fde import planted_pages  # noqa: E402
from tools.bench_int8 import I8_PEAK_TOPS, pooled_of  # noqa: E402

MS = (100, 400, 1000)


def alternating(variants, steps, warmup):
    """{name: {median_ms, min_ms, max_ms}} of the callables in `variants`, timed round-robin: step s runs every variant once, so
    a drift of the clock or of a neighbour's load falls on all of them alike"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    evs = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
           for name in variants}
    torch.cuda.synchronize()
    for s in range(steps):
        for name, fn in variants.items():
            a, b = evs[name][s]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    out = {}
    for name in variants:
        ms = sorted(a.elapsed_time(b) for a, b in evs[name])
        out[name] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
    return out


def stage1_bounds_ms(n_q, q_len, n_d, rows):
    return {"memory_ms": (rows * 16 + n_q * n_d * 4) / (HBM_PEAK_GBS * 1e9) * 1e3,
            "matrix_ms": 2.0 * n_q * q_len * rows * 128 / (I8_PEAK_TOPS * 1e12) * 1e3}


def stage1_leg(amd, corpus, bidx, i8idx, n_q, q_len, dev, steps, warmup):
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    out = torch.empty((n_q, len(bidx)), dtype=torch.float32, device=dev)
    leg = alternating({"binary_scores": lambda: amd.binary_scores(pq, bidx, out=out),
                       "int8_scores": lambda: amd.int8_scores(pq, i8idx, out=out),
                       "exact_scan": lambda: amd.maxsim_scores(pq, corpus)}, steps, warmup)
    leg["bounds"] = stage1_bounds_ms(n_q, q_len, len(bidx), int(bidx.codes.shape[0]))
    leg["binary_share_of_bound"] = max(leg["bounds"].values()) / leg["binary_scores"]["median_ms"]
    leg["binary_vs_int8"] = leg["int8_scores"]["median_ms"] / leg["binary_scores"]["median_ms"]
    leg["binary_vs_exact"] = leg["exact_scan"]["median_ms"] / leg["binary_scores"]["median_ms"]
    return leg


def recall_leg(amd, dev, n_docs, k=10):
    pages, q = planted_pages(dev, n_docs=n_docs)
    full = amd.pack_passages(pages, dev, batch_size=None)
    pooled = pooled_of(amd, pages, dev)
    del pages
    pq = amd.pack_queries(q, dev, compact=False)
    r = amd.ShardedRetriever(full)
    _, exact = r.search(pq, k=k)
    exact = exact.tolist()

    def recall(prefilter, m):
        _, two = r.search(pq, k=k, prefilter=prefilter, n_candidates=m)
        return sum(len(set(a) & set(b)) for a, b in zip(exact, two.tolist())) / (len(pq) * k)

    b_full, b_pooled, i8_full = amd.BinaryIndex.build(full), amd.BinaryIndex.build(pooled), amd.Int8Index.build(full)
    return {"docs": n_docs, "queries": len(pq), "k": k, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs,
            "binary_full": {str(m): recall(b_full, m) for m in MS}, "binary_pooled": {str(m): recall(b_pooled, m) for m in MS},
            "int8_full": {str(m): recall(i8_full, m) for m in MS}, "pooled_bf16": {str(m): recall(pooled, m) for m in MS},
            "bytes": {"binary_full": b_full.nbytes, "binary_pooled": b_pooled.nbytes, "int8_full": i8_full.nbytes,
                      "pooled_bf16": pooled.nbytes, "shard": full.nbytes}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="build,stage1,two_stage,recall")
    ap.add_argument("--recall-docs", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_binary.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_binary", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "hbm_peak_GBps": HBM_PEAK_GBS,
           "i8_peak_TOPs": I8_PEAK_TOPS}
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        bidx, i8idx = amd.BinaryIndex.build(corpus), amd.Int8Index.build(corpus)
        res["bytes"] = {"shard": corpus.nbytes, "binary": bidx.nbytes, "int8": i8idx.nbytes}
        if "build" in legs:
            b = alternating({"binary_build": lambda: amd.BinaryIndex.build(corpus), "int8_build": lambda: amd.Int8Index.build(corpus)},
                            max(3, args.steps // 2), 1)
            b["binary_bound_ms"] = (corpus.nbytes + bidx.codes.numel()) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["binary_share_of_bound"] = b["binary_bound_ms"] / b["binary_build"]["median_ms"]
            res["build"] = b
        if "stage1" in legs:
            res["stage1"] = {str(n): stage1_leg(amd, corpus, bidx, i8idx, n, args.q_len, dev, args.steps if n == 4 else max(3, args.steps // 2),
                                                args.warmup if n == 4 else 1) for n in (4, 1000)}
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
            r = amd.ShardedRetriever(corpus)
            variants = {f"binary_m{m}": (lambda m=m: r.search(pq, k=10, prefilter=bidx, n_candidates=m)) for m in MS}
            variants.update({f"int8_m{m}": (lambda m=m: r.search(pq, k=10, prefilter=i8idx, n_candidates=m)) for m in MS})
            variants["exact_search"] = lambda: r.search(pq, k=10)
            ts = alternating(variants, max(3, args.steps // 2), 1)
            ts["n_queries"] = 1000
            res["two_stage"] = ts
        del corpus, bidx, i8idx
        torch.cuda.empty_cache()
    if "recall" in legs:
        res["recall"] = recall_leg(amd, dev, args.recall_docs)
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
