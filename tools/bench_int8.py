"""The int8 token-level index (msim_i8_*, colpali_amd.Int8Index) on the headline shard; one JSON object on stdout (not part of
bench.py).

    python tools/bench_int8.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--legs build,stage1,two_stage,recall]

Legs, each timed with device events after a warm-up:
  * build: Int8Index.build of the shard; bound = (the shard's rows read twice + the codes written) / 8 TB/s (the second read is
    meant to hit in L2, so the HBM bound is one read + the write; both are reported).
  * stage1: int8_scores at 4 and 1000 queries of 32 tokens on the full shard and on a 343-row pooled-size shard, beside the exact
    scan (maxsim_scores) of the same shard; bound = max((rows x 128 + n_q n_d 4) B / 8 TB/s, 2 n_q 32 rows 128 / 5 POPS).
  * two_stage: ShardedRetriever.search(prefilter=<Int8Index>, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside
    the exact search, the bf16 pooled prefilter (343 rows, m = 100) and the FDE prefilter (m = 100) in the same run.
  * recall: recall@10 against the exact search on the planted 10 000-page set of tools/bench_fde.py:planted_pages, for the int8
    index of the full pages and of the pooled pages (HierarchicalTokenPooler(pool_factor=3)), beside the bf16 pooled prefilter
    and FDE at m = 100.
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
from tools.bench_rerank import timed  # noqa: E402

MS = (100, 400, 1000)
I8_PEAK_TOPS = 5000.0          # dense int8 MFMA peak (2x bf16)


def stage1_bound_ms(n_q, q_len, n_d, rows):
    return max((rows * 128 + n_q * n_d * 4) / (HBM_PEAK_GBS * 1e9), 2.0 * n_q * q_len * rows * 128 / (I8_PEAK_TOPS * 1e12)) * 1e3


def stage1_leg(amd, corpus, index, n_q, q_len, dev, steps, warmup):
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    out = torch.empty((n_q, len(index)), dtype=torch.float32, device=dev)
    leg = {"bound_ms": stage1_bound_ms(n_q, q_len, len(index), int(index.codes.shape[0])),
           "int8_scores": timed(lambda: amd.int8_scores(pq, index, out=out), steps, warmup),
           "exact_scan": timed(lambda: amd.maxsim_scores(pq, corpus), max(2, steps // 3), 1)}
    leg["int8_scores"]["share_of_bound"] = leg["bound_ms"] / leg["int8_scores"]["median_ms"]
    leg["speedup_vs_exact"] = leg["exact_scan"]["median_ms"] / leg["int8_scores"]["median_ms"]
    return leg


def pooled_of(amd, pages, dev):
    pooler = amd.HierarchicalTokenPooler()
    pooled = []
    for d0 in range(0, pages.shape[0], 1000):
        pooled += pooler.pool_embeddings(list(pages[d0:d0 + 1000].unbind(0)), pool_factor=3)
    return amd.pack_passages(pooled, dev, batch_size=None)


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

    i8_full, i8_pooled = amd.Int8Index.build(full), amd.Int8Index.build(pooled)
    out = {"docs": n_docs, "queries": len(pq), "k": k, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs,
           "int8_full": {str(m): recall(i8_full, m) for m in MS}, "int8_pooled": {str(m): recall(i8_pooled, m) for m in MS},
           "pooled_bf16_m100": recall(pooled, 100), "fde_m100": recall(amd.FdeIndex.build(full), 100)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--coarse-len", type=int, default=343)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="build,stage1,two_stage,recall")
    ap.add_argument("--recall-docs", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_int8.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_int8", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "hbm_peak_GBps": HBM_PEAK_GBS,
           "i8_peak_TOPs": I8_PEAK_TOPS}
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        index = amd.Int8Index.build(corpus)
        if "build" in legs:
            b = timed(lambda: amd.Int8Index.build(corpus), max(2, args.steps // 5), 1)
            b["bound_ms"] = (corpus.nbytes + index.codes.numel()) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["bound_two_reads_ms"] = (2 * corpus.nbytes + index.codes.numel()) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["share_of_bound"] = b["bound_ms"] / b["median_ms"]
            res["build"] = b
        if "stage1" in legs:
            res["stage1"] = {"full": {str(n): stage1_leg(amd, corpus, index, n, args.q_len, dev, args.steps, args.warmup)
                                      for n in (4, 1000)}}
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
            r = amd.ShardedRetriever(corpus)
            ts = {"n_queries": 1000, "int8": {}}
            for m in MS:
                ts["int8"][str(m)] = timed(lambda: r.search(pq, k=10, prefilter=index, n_candidates=m), args.steps, args.warmup)
            fde = amd.FdeIndex.build(corpus)
            ts["fde_m100"] = timed(lambda: r.search(pq, k=10, prefilter=fde, n_candidates=100), args.steps, args.warmup)
            del fde
            ts["exact_search"] = timed(lambda: r.search(pq, k=10), 3, 1)
            res["two_stage"] = ts
        del index
        if legs & {"stage1", "two_stage"}:
            coarse = make_shard(args.docs, args.coarse_len, dev, seed=4321)
            cidx = amd.Int8Index.build(coarse)
            if "stage1" in legs:
                res["stage1"]["pooled"] = {str(n): stage1_leg(amd, coarse, cidx, n, args.q_len, dev, args.steps, args.warmup)
                                           for n in (4, 1000)}
            if "two_stage" in legs:
                ts = res["two_stage"]
                ts["pooled_bf16_m100"] = timed(lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=100), max(3, args.steps // 3), 1)
                ts["int8_pooled_m100"] = timed(lambda: r.search(pq, k=10, prefilter=cidx, n_candidates=100), args.steps, args.warmup)
            del coarse, cidx
        del corpus
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
