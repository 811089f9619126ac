"""The centroid-code index (msim_cent_*, colpali_amd.CentroidIndex) on the headline shard; one JSON object on stdout (not part of
bench.py).

    python tools/bench_centroid.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--legs build,stage1,two_stage,recall]

Legs, each timed with device events after a warm-up:
  * build: train_centroids (K = 1024, 8 iterations on 2^18 sampled rows) and CentroidIndex.build with given centroids, for K = 1024
    and 2048.
  * stage1: centroid_scores at 4 and 1000 queries of 32 tokens for K = 1024 and 2048, beside int8_scores and the exact scan of the
    same shard.  LDS bound = n_q x rows x 64 B / (256 B/clk/CU x CUs x clock); the clock is the one the device reports right after
    the timed loop (the nominal 2.4 GHz, and labelled so, where it reports none).
  * two_stage: ShardedRetriever.search(prefilter=<CentroidIndex>, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside
    the int8, FDE and bf16 pooled (343 rows) prefilters and the exact search in the same run.
  * recall: recall@10 against the exact search on the planted 10 000-page set of tools/bench_fde.py:planted_pages for K = 1024 and
    2048 (centroids trained on that set), beside the int8, pooled and FDE first stages.
The bank-conflict counter comes from a separate `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE` run of this script with
`--legs stage1`.
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

from bench_legs.common import make_queries, make_shard  # noqa: E402
from tools.bench_fde import planted_pages  # noqa: E402
from tools.bench_int8 import pooled_of  # noqa: E402
from tools.bench_rerank import timed  # noqa: E402

MS = (100, 400, 1000)
KS = (1024, 2048)
LDS_BYTES_PER_CLK_CU = 256
NOMINAL_MHZ = 2400.0


def observed_clock_mhz():
    try:
        mhz = float(torch.cuda.clock_rate())
        if mhz > 0:
            return mhz, "reported"
    except Exception:
        pass
    return NOMINAL_MHZ, "nominal"


def stage1_leg(amd, corpus, index, i8, n_q, q_len, dev, steps, warmup, cus):
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    out = torch.empty((n_q, len(index)), dtype=torch.float32, device=dev)
    leg = {"centroid_scores": timed(lambda: amd.centroid_scores(pq, index, out=out), steps, warmup)}
    mhz, how = observed_clock_mhz()
    blocks = -(-q_len // 32)
    leg["clock_mhz"], leg["clock"] = mhz, how
    leg["lds_bound_ms"] = n_q * blocks * int(index.codes.shape[0]) * 64 / (LDS_BYTES_PER_CLK_CU * cus * mhz * 1e6) * 1e3
    leg["lds_bound_fraction"] = leg["lds_bound_ms"] / leg["centroid_scores"]["median_ms"]
    if i8 is not None:
        leg["int8_scores"] = timed(lambda: amd.int8_scores(pq, i8, out=out), max(2, steps // 2), 1)
        leg["exact_scan"] = timed(lambda: amd.maxsim_scores(pq, corpus), max(2, steps // 3), 1)
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

    out = {"docs": n_docs, "queries": len(pq), "k": k}
    for K in KS:
        idx = amd.CentroidIndex.build(full, n_centroids=K)
        out[f"centroid_K{K}"] = {str(m): recall(idx, m) for m in MS}
        del idx
    i8 = amd.Int8Index.build(full)
    out["int8_full"] = {str(m): recall(i8, m) for m in MS}
    out["pooled_bf16_m100"] = recall(pooled, 100)
    out["fde_m100"] = recall(amd.FdeIndex.build(full), 100)
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
        raise SystemExit("bench_centroid.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_centroid", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "cus": cus}
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        cents = {K: amd.train_centroids(corpus, K) for K in KS}
        index = {K: amd.CentroidIndex.build(corpus, centroids=cents[K]) for K in KS}
        res["index_bytes"] = {str(K): index[K].nbytes for K in KS}
        res["corpus_bytes"] = corpus.nbytes
        if "build" in legs:
            res["build"] = {"train_K1024": timed(lambda: amd.train_centroids(corpus, 1024), 2, 1)}
            for K in KS:
                res["build"][f"encode_K{K}"] = timed(lambda: amd.CentroidIndex.build(corpus, centroids=cents[K]), 2, 1)
        i8 = amd.Int8Index.build(corpus) if legs & {"stage1", "two_stage"} else None
        if "stage1" in legs:
            res["stage1"] = {}
            for K in KS:
                res["stage1"][f"K{K}"] = {str(n): stage1_leg(amd, corpus, index[K], i8 if K == KS[0] else None, n, args.q_len, dev,
                                                             args.steps, args.warmup, cus) for n in (4, 1000)}
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
            r = amd.ShardedRetriever(corpus)
            ts = {"n_queries": 1000}
            for K in KS:
                ts[f"centroid_K{K}"] = {str(m): timed(lambda: r.search(pq, k=10, prefilter=index[K], n_candidates=m), args.steps,
                                                      args.warmup) for m in MS}
            ts["int8"] = {str(m): timed(lambda: r.search(pq, k=10, prefilter=i8, n_candidates=m), max(3, args.steps // 3), 1) for m in MS}
            del i8
            fde = amd.FdeIndex.build(corpus)
            ts["fde_m100"] = timed(lambda: r.search(pq, k=10, prefilter=fde, n_candidates=100), args.steps, args.warmup)
            del fde
            coarse = make_shard(args.docs, args.coarse_len, dev, seed=4321)
            ts["pooled_bf16_m100"] = timed(lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=100), max(3, args.steps // 3), 1)
            del coarse
            ts["exact_search"] = timed(lambda: r.search(pq, k=10), 3, 1)
            res["two_stage"] = ts
        del corpus, index, cents
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
