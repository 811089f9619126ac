"""Fixed dimensional encodings (msim_fde_*, colpali_amd.FdeIndex) on the headline shard; one JSON object on stdout (not part of
bench.py).

    python tools/bench_fde.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--legs build,stage1,two_stage,recall]

Legs, each timed with device events after a warm-up:
  * build: FdeIndex.build of the shard (default config: R = 20, k_sim = 5, d_proj = 16, F = 10 240); bound = (the shard's rows +
    the index) / 8 TB/s.
  * stage1: fde_scores at 4 and 1000 queries of 32 tokens -- the query encoder plus the scorer -- and the scorer alone on encoded
    queries; bound = max((n_d F 2 + n_q n_d 4) B / 8 TB/s, 2 n_q n_d F / 2.5 PFLOP/s).
  * two_stage: ShardedRetriever.search(prefilter=<FdeIndex>, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside the
    pooled prefilter (343 rows per page, m = 100) and the exact search.
  * recall: recall@10 against the exact search on the planted 10 000-page set of tools/bench_rerank.py:planted_recall, for each m,
    beside the pooled prefilter at m = 100 (reported, not gated; the encoding is not tuned on this set).
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

from bench_legs.common import HBM_PEAK_GBS, MFMA_PEAK_TFLOPS, make_queries, make_shard  # noqa: E402
from tools.bench_rerank import timed  # noqa: E402

MS = (100, 400, 1000)


def stage1_bound_ms(n_q, n_d, F):
    return max((n_d * F * 2 + n_q * n_d * 4) / (HBM_PEAK_GBS * 1e9), 2.0 * n_q * n_d * F / (MFMA_PEAK_TFLOPS * 1e12)) * 1e3


def planted_pages(dev, n_docs=10_000, doc_len=1024, n_q=100, q_len=32, seed=5):
    """The planted set of tools/bench_rerank.py:planted_recall, drawn the same way from the same seed."""
    g = torch.Generator(device=dev).manual_seed(seed)
    pages = []
    for d0 in range(0, n_docs, 500):
        n = min(500, n_docs - d0)
        topics = torch.randn((n, 48, 128), generator=g, device=dev)
        pick = torch.randint(0, 48, (n, doc_len), generator=g, device=dev)
        rows = torch.gather(topics, 1, pick.unsqueeze(-1).expand(n, doc_len, 128)) + 0.6 * torch.randn((n, doc_len, 128), generator=g, device=dev)
        pages.append(torch.nn.functional.normalize(rows, dim=-1).to(torch.bfloat16))
    pages = torch.cat(pages)
    target = torch.randint(0, n_docs, (n_q,), generator=g, device=dev)
    tok = torch.randint(0, doc_len, (n_q, q_len), generator=g, device=dev)
    q = pages[target.unsqueeze(1), tok].float() + 0.8 * torch.randn((n_q, q_len, 128), generator=g, device=dev) / 128 ** 0.5
    return pages, torch.nn.functional.normalize(q, dim=-1).to(torch.bfloat16)


def recall_leg(amd, dev, n_docs, k=10):
    from tools.bench_rerank import planted_recall

    pooled = planted_recall(amd, dev, n_docs=n_docs, m=100, k=k)
    pages, q = planted_pages(dev, n_docs=n_docs)
    full = amd.pack_passages(pages, dev, batch_size=None)
    del pages
    pq = amd.pack_queries(q, dev, compact=False)
    index = amd.FdeIndex.build(full)
    r = amd.ShardedRetriever(full)
    _, exact = r.search(pq, k=k)
    exact = exact.tolist()
    out = {"docs": n_docs, "queries": len(pq), "k": k, "pooled_prefilter_m100": pooled["recall_at_10"], "fde": {}}
    for m in MS:
        _, two = r.search(pq, k=k, prefilter=index, n_candidates=m)
        hits = sum(len(set(a) & set(b)) for a, b in zip(exact, two.tolist()))
        out["fde"][str(m)] = hits / (len(pq) * k)
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
        raise SystemExit("bench_fde.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    config = amd.FdeConfig()
    F = config.dim
    res = {"tool": "bench_fde", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "F": F,
           "config": {"reps": config.reps, "ksim": config.ksim, "dproj": config.dproj, "fill_empty": config.fill_empty},
           "hbm_peak_GBps": HBM_PEAK_GBS, "mfma_peak_TFLOPs": MFMA_PEAK_TFLOPS}
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        index = amd.FdeIndex.build(corpus, config)
        if "build" in legs:
            b = timed(lambda: amd.FdeIndex.build(corpus, config), max(2, args.steps // 5), 1)
            b["bound_ms"] = (corpus.nbytes + index.Fd.numel() * 2) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["share_of_bound"] = b["bound_ms"] / b["median_ms"]
            res["build"] = b
        if "stage1" in legs:
            res["stage1"] = {}
            for n_q in (4, 1000):
                pq = amd.pack_queries(make_queries(n_q, args.q_len, dev, seed=99), dev, compact=False)
                out = torch.empty((n_q, len(index)), dtype=torch.float32, device=dev)
                Fq = amd.encode_queries(pq, index)
                leg = {"bound_ms": stage1_bound_ms(n_q, len(index), F),
                       "fde_scores": timed(lambda: amd.fde_scores(pq, index, out=out), args.steps, args.warmup),
                       "scorer_only": timed(lambda: amd.fde.scores_from_encodings(Fq, index.Fd, out=out), args.steps, args.warmup),
                       "encode_queries": timed(lambda: amd.encode_queries(pq, index), args.steps, args.warmup)}
                for key in ("fde_scores", "scorer_only"):
                    leg[key]["share_of_bound"] = leg["bound_ms"] / leg[key]["median_ms"]
                res["stage1"][str(n_q)] = leg
                del out
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
            r = amd.ShardedRetriever(corpus)
            ts = {"n_queries": 1000, "fde": {}}
            for m in MS:
                ts["fde"][str(m)] = timed(lambda: r.search(pq, k=10, prefilter=index, n_candidates=m), args.steps, args.warmup)
            coarse = make_shard(args.docs, args.coarse_len, dev, seed=4321)
            ts["pooled_prefilter_m100"] = timed(lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=100), max(3, args.steps // 3), 1)
            del coarse
            ts["exact_search"] = timed(lambda: r.search(pq, k=10), 3, 1)
            ts["speedup_vs_pooled_m100"] = ts["pooled_prefilter_m100"]["median_ms"] / ts["fde"]["100"]["median_ms"]
            res["two_stage"] = ts
        del corpus, index
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
