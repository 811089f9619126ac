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

    python tools/bench_fde.py --dim 320 [--out FILE] [--summary profiles/fde_wide_summary.md] [--legs build,stage1,search,recall]

--dim 320 measures the 320-wide index (msim_fdew_*, colpali_amd.FdeWideIndex) on the shard of tools/bench_fp4.py --dim 320
(50 000 x 1024 x 320 bf16 by default), the variants of a leg alternating call by call in one timed loop (median and range): see
`main_wide`.
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


# ------------------------------------------------------------------------------------------------------------------ width 320
WIDE_M1 = (1000, 4000)
N_REFINE = 100
POOLED_LEN = 343


def wide_recall_leg(amd, dev, n_docs, config, k=10):
    """recall@10 against the exact search on the planted set at width 320 (tools/bench_fp4.py: wide_planted)"""
    from tools.bench_fp4 import wide_planted

    full, pooled, pq = wide_planted(amd, dev, n_docs)
    r = amd.ShardedRetriever(full)
    exact = r.search(pq, k=k)[1].tolist()
    fde, f4 = amd.FdeWideIndex.build(full, config), amd.Fp4WideIndex.build(full)

    def hits(**kw):
        got = r.search(pq, k=k, **kw)[1].tolist()
        return sum(len(set(a) & set(b)) for a, b in zip(exact, got)) / (len(pq) * k)

    out = {"docs": n_docs, "queries": len(pq), "k": k, "n_refine": N_REFINE, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs,
           "fde_wide": {str(m): hits(prefilter=fde, n_candidates=m) for m in MS},
           "pooled_corpus": {str(m): hits(prefilter=pooled, n_candidates=m) for m in MS},
           "fp4_wide_m100": hits(prefilter=f4, n_candidates=100)}
    for m1 in WIDE_M1:
        out[f"fde_wide_refine_m{m1}"] = hits(prefilter=fde, n_candidates=m1, refine=f4, n_refine=N_REFINE)
    return out


def _rng(v):
    return f"{v['median_ms']:.2f} ({v['min_ms']:.2f} – {v['max_ms']:.2f})"


def wide_summary(res):
    L = ["# FDE index at width 320: measured on one MI355X", "",
         f"`tools/bench_fde.py --dim 320 --steps {res['steps']} --warmup {res['warmup']}` on the 320-wide shard ({res['docs']} pages × "
         f"{res['doc_len']} rows, bf16), queries of {res['q_len']} tokens, configuration R = {res['config']['reps']}, k_sim = "
         f"{res['config']['ksim']}, d_proj = {res['config']['dproj']} (F = {res['F']}).  The variants of a leg alternate call by call in "
         "one timed loop; median ms, with the range in brackets.", ""]
    if "build" in res:
        b = res["build"]
        L += ["## Build", "", f"`FdeWideIndex.build`: {_rng(b['fde_wide_build'])} ms; the bound (the shard's rows + the index at "
              f"{res['hbm_peak_GBps'] / 1000:.0f} TB/s) is {b['bound_ms']:.1f} ms.  Beside it in the loop, `Fp4WideIndex.build`: "
              f"{_rng(b['fp4_wide_build'])} ms.", ""]
    if "stage1" in res:
        L += ["## Stage 1: query encoder + scorer", "", "| queries | `fde_wide_scores` | scorer alone | query encoder alone | bound |",
              "|---|---|---|---|---|"]
        for n_q, leg in res["stage1"].items():
            L.append(f"| {n_q} × {res['q_len']} | {_rng(leg['fde_wide_scores'])} | {_rng(leg['scorer_only'])} | "
                     f"{_rng(leg['encode_queries'])} | {leg['bound_ms']:.2f} |")
        L.append("")
    if "search" in res:
        L += [f"## Search at 1000 × {res['q_len']}, k = 10, all alternating in one loop", "", "| variant | ms |", "|---|---|"]
        L += [f"| `{name}` | {_rng(v)} |" for name, v in res["search"].items() if isinstance(v, dict)]
        L.append("")
    if "recall" in res:
        r = res["recall"]
        L += [f"## Recall@10 against the exact search, planted {r['docs']}-page set at width 320 ({r['queries']} queries)", "",
              "| first stage | " + " | ".join(f"m = {m}" for m in MS) + " |", "|---|" + "---|" * len(MS),
              "| `FdeWideIndex` | " + " | ".join(f"{r['fde_wide'][str(m)]:.3f}" for m in MS) + " |",
              f"| pooled pages ({r['pooled_rows_per_doc']:.0f} rows) | " + " | ".join(f"{r['pooled_corpus'][str(m)]:.3f}" for m in MS) + " |",
              "", f"`Fp4WideIndex` at m = 100: {r['fp4_wide_m100']:.3f}.  The cascade `prefilter=<FdeWideIndex>, refine=<Fp4WideIndex>, "
              f"n_refine={r['n_refine']}`: " + ", ".join(f"{r[f'fde_wide_refine_m{m1}']:.3f} at n_candidates = {m1}" for m1 in WIDE_M1) + ".", ""]
    return "\n".join(L)


def main_wide(args):
    """--dim 320: build beside the FP4 build; encoder + scorer at 4 and 1000 queries; the two-stage search at m = 100 / 400 / 1000 and
    the cascade through the FP4 rows at n_candidates = 1000 / 4000, beside the pooled prefilter and the FP4 first stage; recall."""
    from tools.bench_binary import alternating
    from tools.bench_rerank import make_queries_dim, make_shard_dim

    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    docs = args.docs if args.docs is not None else 50_000
    t0 = time.perf_counter()
    config = amd.FdeConfig()
    F = config.dim
    res = {"tool": "bench_fde", "dim": 320, "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len, "F": F, "steps": args.steps,
           "warmup": args.warmup, "config": {"reps": config.reps, "ksim": config.ksim, "dproj": config.dproj, "fill_empty": config.fill_empty},
           "hbm_peak_GBps": HBM_PEAK_GBS, "mfma_peak_TFLOPs": MFMA_PEAK_TFLOPS}
    if legs & {"build", "stage1", "search"}:
        corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
        index = amd.FdeWideIndex.build(corpus, config)
        if "build" in legs:
            b = alternating({"fde_wide_build": lambda: amd.FdeWideIndex.build(corpus, config),
                             "fp4_wide_build": lambda: amd.Fp4WideIndex.build(corpus)}, max(3, args.steps // 3), 1)
            b["bound_ms"] = (corpus.nbytes + index.Fd.numel() * 2) / (HBM_PEAK_GBS * 1e9) * 1e3
            res["build"] = b
        if "stage1" in legs:
            res["stage1"] = {}
            for n_q in (4, 1000):
                pq = amd.pack_queries(make_queries_dim(n_q, args.q_len, 320, dev, seed=99), dev, compact=False)
                out = torch.empty((n_q, len(index)), dtype=torch.float32, device=dev)
                Fq = amd.fde_wide_encode_queries(pq, index)
                leg = alternating({"fde_wide_scores": lambda: amd.fde_wide_scores(pq, index, out=out),
                                   "scorer_only": lambda: amd.fde.scores_from_encodings(Fq, index.Fd, out=out),
                                   "encode_queries": lambda: amd.fde_wide_encode_queries(pq, index)}, args.steps, args.warmup)
                leg["bound_ms"] = stage1_bound_ms(n_q, len(index), F)
                res["stage1"][str(n_q)] = leg
                del out
        if "search" in legs:
            pq = amd.pack_queries(make_queries_dim(1000, args.q_len, 320, dev, seed=99), dev, compact=False)
            coarse = make_shard_dim(docs, POOLED_LEN, 320, dev, seed=4321)
            f4 = amd.Fp4WideIndex.build(corpus)
            r = amd.ShardedRetriever(corpus)
            variants = {f"fde_wide_m{m}": (lambda m=m: r.search(pq, k=10, prefilter=index, n_candidates=m)) for m in MS}
            for m1 in WIDE_M1:
                variants[f"fde_wide_m{m1}_refine_m{N_REFINE}"] = lambda m1=m1: r.search(pq, k=10, prefilter=index, n_candidates=m1, refine=f4,
                                                                                        n_refine=N_REFINE)
            variants["pooled_m100"] = lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=100)
            variants["fp4_wide_m100"] = lambda: r.search(pq, k=10, prefilter=f4, n_candidates=100)
            res["search"] = alternating(variants, max(3, args.steps // 2), 1)
            del coarse, f4
        del corpus, index
        torch.cuda.empty_cache()
    if "recall" in legs:
        res["recall"] = wide_recall_leg(amd, dev, args.recall_docs, config)
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(wide_summary(res) + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128, choices=(128, 320), help="320: the FdeWideIndex on the 320-wide shard")
    ap.add_argument("--summary", default=None, help="--dim 320: write the markdown summary here")
    ap.add_argument("--docs", type=int, default=None, help="default: 125 000 at width 128, 50 000 at width 320 (the same bytes)")
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
    if args.dim == 320:
        if args.legs == "build,stage1,two_stage,recall":
            args.legs = "build,stage1,search,recall"
        return main_wide(args)
    args.docs = 125_000 if args.docs is None else args.docs
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
