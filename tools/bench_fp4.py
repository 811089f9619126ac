"""The FP4 index (msim_f4_*, colpali_amd.Fp4Index) on the headline shard; one JSON object on stdout and a summary in markdown
(not part of bench.py).

    python tools/bench_fp4.py [--out FILE] [--summary profiles/fp4_summary.md] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024]
                              [--legs build,stage1,pooled,two_stage,recall]

Legs, each timed with device events after a warm-up; the variants of a leg ALTERNATE call by call inside one timed loop, and every
figure is the median with its range:
  * build: Fp4Index.build of the shard beside Int8Index.build and BinaryIndex.build; bound = (the shard's rows read once + the
    codes and scales written) / 8 TB/s.
  * stage1: fp4_scores and fp6_scores (e2m3 query tokens against the same Fp4Index) at 4 and 1000 queries of 32 tokens on the full
    shard, beside int8_scores, binary_scores and the exact scan (maxsim_scores) of the same shard.  Bounds of fp4_scores: memory (rows x 65 + n_q n_d 4) B / 8 TB/s, matrix cores
    2 n_q 32 rows 128 / 10 PFLOPS.
  * pooled: the stage1 leg on a shard of the same page count and 343 rows per page (a pool factor of 3).
  * two_stage: ShardedRetriever.search(prefilter=<Fp4Index>, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside the
    same search with fp4_score_fn=fp6_scores, through the Int8Index and the BinaryIndex, and the exact search.
  * recall: recall@10 against the exact search on the planted 10 000-page set of tools/bench_fde.py:planted_pages, for the FP4
    index of the full and the pooled pages, scored with e2m1 and with e2m3 query tokens, beside the Int8Index and the BinaryIndex
    of the full pages.
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
from tools.bench_binary import alternating  # noqa: E402
from tools.bench_fde import planted_pages  # noqa: E402
from tools.bench_int8 import pooled_of  # noqa: E402

MS = (100, 400, 1000)
FP4_PEAK_TFLOPS = 10000.0      # dense block-scaled FP4 MFMA peak (4x bf16)
POOLED_LEN = 343


def stage1_bounds_ms(n_q, q_len, n_d, rows):
    return {"memory_ms": (rows * 65 + n_q * n_d * 4) / (HBM_PEAK_GBS * 1e9) * 1e3,
            "matrix_ms": 2.0 * n_q * q_len * rows * 128 / (FP4_PEAK_TFLOPS * 1e12) * 1e3}


def stage1_leg(amd, corpus, f4idx, i8idx, bidx, n_q, q_len, dev, steps, warmup):
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    out = torch.empty((n_q, len(f4idx)), dtype=torch.float32, device=dev)
    leg = alternating({"fp4_scores": lambda: amd.fp4_scores(pq, f4idx, out=out),
                       "fp6_scores": lambda: amd.fp6_scores(pq, f4idx, out=out),
                       "int8_scores": lambda: amd.int8_scores(pq, i8idx, out=out),
                       "binary_scores": lambda: amd.binary_scores(pq, bidx, out=out),
                       "exact_scan": lambda: amd.maxsim_scores(pq, corpus)}, steps, warmup)
    leg["bounds"] = stage1_bounds_ms(n_q, q_len, len(f4idx), int(f4idx.codes.shape[0]))
    leg["fp4_share_of_memory_bound"] = leg["bounds"]["memory_ms"] / leg["fp4_scores"]["median_ms"]
    leg["fp4_share_of_matrix_bound"] = leg["bounds"]["matrix_ms"] / leg["fp4_scores"]["median_ms"]
    leg["fp6_vs_fp4"] = leg["fp6_scores"]["median_ms"] / leg["fp4_scores"]["median_ms"]
    # "equal" only when the gap of the medians is inside the larger of the two spreads of this loop
    spread = max(leg[k]["max_ms"] - leg[k]["min_ms"] for k in ("fp4_scores", "fp6_scores"))
    leg["fp6_equals_fp4"] = abs(leg["fp6_scores"]["median_ms"] - leg["fp4_scores"]["median_ms"]) <= spread
    leg["fp4_vs_int8"] = leg["int8_scores"]["median_ms"] / leg["fp4_scores"]["median_ms"]
    leg["fp4_vs_binary"] = leg["binary_scores"]["median_ms"] / leg["fp4_scores"]["median_ms"]
    leg["fp4_vs_exact"] = leg["exact_scan"]["median_ms"] / leg["fp4_scores"]["median_ms"]
    return leg


def stage1_legs(amd, corpus, idxs, q_len, dev, steps, warmup):
    return {str(n): stage1_leg(amd, corpus, *idxs, n, q_len, dev, steps if n == 4 else max(3, steps // 2), warmup if n == 4 else 1)
            for n in (4, 1000)}


def recall_leg(amd, dev, n_docs, k=10):
    pages, q = planted_pages(dev, n_docs=n_docs)
    full = amd.pack_passages(pages, dev, batch_size=None)
    pooled = pooled_of(amd, pages, dev)
    del pages
    pq = amd.pack_queries(q, dev, compact=False)
    r = amd.ShardedRetriever(full)
    _, exact = r.search(pq, k=k)
    exact = exact.tolist()

    r6 = amd.ShardedRetriever(full, fp4_score_fn=amd.fp6_scores)

    def recall(prefilter, m, retriever=r):
        _, two = retriever.search(pq, k=k, prefilter=prefilter, n_candidates=m)
        return sum(len(set(a) & set(b)) for a, b in zip(exact, two.tolist())) / (len(pq) * k)

    stages = {"fp4_full": amd.Fp4Index.build(full), "fp4_pooled": amd.Fp4Index.build(pooled), "int8_full": amd.Int8Index.build(full),
              "binary_full": amd.BinaryIndex.build(full)}
    out = {"docs": n_docs, "queries": len(pq), "k": k, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs}
    for name, idx in stages.items():
        out[name] = {str(m): recall(idx, m) for m in MS}
    for name in ("full", "pooled"):                       # the same two indexes, e2m3 query tokens
        out[f"fp6_{name}"] = {str(m): recall(stages[f"fp4_{name}"], m, r6) for m in MS}
    out["bytes"] = {name: idx.nbytes for name, idx in stages.items()}
    out["bytes"].update({"fp6_full": stages["fp4_full"].nbytes, "fp6_pooled": stages["fp4_pooled"].nbytes})
    out["bytes"]["shard"] = full.nbytes
    return out


def _ms(v):
    return f"{v['median_ms']:.2f} ms ({v['min_ms']:.2f}–{v['max_ms']:.2f})"


def _stage1_table(legs):
    rows = ["| | `fp4_scores` | `fp6_scores` | `int8_scores` | `binary_scores` | exact scan | memory bound (share) | matrix-core bound (share) |",
            "|---|---|---|---|---|---|---|---|"]
    for n, leg in legs.items():
        b = leg["bounds"]
        rows.append(f"| {n} × 32 | {_ms(leg['fp4_scores'])} | {_ms(leg['fp6_scores'])} | {_ms(leg['int8_scores'])} | {_ms(leg['binary_scores'])} | "
                    f"{_ms(leg['exact_scan'])} | {b['memory_ms']:.2f} ms ({leg['fp4_share_of_memory_bound']:.2f}) | "
                    f"{b['matrix_ms']:.2f} ms ({leg['fp4_share_of_matrix_bound']:.2f}) |")
    for n, leg in legs.items():
        rows.append("")
        rows.append(f"{n} × 32: `fp6_scores` / `fp4_scores` = {leg['fp6_vs_fp4']:.3f}; the gap of the medians is "
                    f"{'inside' if leg['fp6_equals_fp4'] else 'OUTSIDE'} the larger spread of the two in this loop.")
    return rows


def summary(res):
    """the markdown summary of one run's JSON: measured figures only, a leg that did not run is named as not measured"""
    L = ["# FP4 index: measured on one MI355X", "",
         f"`tools/bench_fp4.py --steps {res['steps']} --warmup {res['warmup']}` on the headline shard ({res['docs']} pages × {res['doc_len']} "
         "rows, bf16), queries of 32 tokens.  The variants of a leg alternate call by call in one timed loop; median, with the range in "
         "brackets.  The bounds are derived (8 TB/s; 10 PFLOPS dense FP4), not measured; a share is bound / measured.", ""]
    if "bytes" in res:
        b = res["bytes"]
        L += [f"Sizes: shard {b['shard'] / 1e9:.2f} GB, `Int8Index` {b['int8'] / 1e9:.2f} GB, `Fp4Index` {b['fp4'] / 1e9:.2f} GB, "
              f"`BinaryIndex` {b['binary'] / 1e9:.2f} GB.", ""]
    for key, title in (("stage1", "Stage 1, full shard"), ("pooled", f"Stage 1, {POOLED_LEN}-row pooled pages")):
        L += [f"## {title}", ""]
        L += _stage1_table(res[key]) if key in res else ["Not measured in this run."]
        L += [""]
    L += ["## Build, two-stage search, recall", ""]
    if "build" in res:
        b = res["build"]
        L += [f"* Build: `Fp4Index.build` {_ms(b['fp4_build'])} in one launch, {b['fp4_share_of_bound']:.2f} of its {b['fp4_bound_ms']:.2f} ms "
              f"bound; `Int8Index.build` {_ms(b['int8_build'])}, `BinaryIndex.build` {_ms(b['binary_build'])} in the same loop."]
    else:
        L += ["* Build: not measured in this run."]
    if "two_stage" in res:
        t = res["two_stage"]
        per = lambda p: " / ".join(f"{t[f'{p}_m{m}']['median_ms']:.1f}" for m in MS)
        L += [f"* Two-stage search at 1000 × 32, k = 10, m = 100 / 400 / 1000: fp4 {per('fp4')} ms; fp6 queries {per('fp6')} ms; int8 {per('int8')} ms; binary "
              f"{per('binary')} ms; exact search {t['exact_search']['median_ms']:.1f} ms, all alternating in one loop."]
    else:
        L += ["* Two-stage search: not measured in this run."]
    if "recall" in res:
        r = res["recall"]
        L += [f"* Recall@10 against the exact search on the planted {r['docs']}-page set ({r['queries']} queries):", "",
              "| first stage | bytes | m = 100 | m = 400 | m = 1000 |", "|---|---|---|---|---|"]
        names = {"fp4_full": "`Fp4Index`, full pages", "fp6_full": "`Fp4Index`, full pages, e2m3 queries (`fp6_scores`)",
                 "fp4_pooled": f"`Fp4Index`, pooled pages ({r['pooled_rows_per_doc']:.0f} rows)",
                 "fp6_pooled": f"`Fp4Index`, pooled pages ({r['pooled_rows_per_doc']:.0f} rows), e2m3 queries",
                 "int8_full": "`Int8Index`, full pages", "binary_full": "`BinaryIndex`, full pages"}
        for key, name in names.items():
            L += [f"| {name} | {r['bytes'][key] / 1e6:.0f} MB | " + " | ".join(f"{r[key][str(m)]:.3f}" for m in MS) + " |"]
    else:
        L += ["* Recall: not measured in this run."]
    return "\n".join(L) + "\n"


def _progress(what, t0):
    print(f"[bench_fp4] {what} at {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="build,stage1,pooled,two_stage,recall")
    ap.add_argument("--recall-docs", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--summary", default=None, help="write the markdown summary here (profiles/fp4_summary.md)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fp4.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_fp4", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "steps": args.steps,
           "warmup": args.warmup, "hbm_peak_GBps": HBM_PEAK_GBS, "fp4_peak_TFLOPs": FP4_PEAK_TFLOPS}
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        f4idx, i8idx, bidx = amd.Fp4Index.build(corpus), amd.Int8Index.build(corpus), amd.BinaryIndex.build(corpus)
        _progress("shard and indexes", t0)
        res["bytes"] = {"shard": corpus.nbytes, "fp4": f4idx.nbytes, "int8": i8idx.nbytes, "binary": bidx.nbytes}
        if "build" in legs:
            b = alternating({"fp4_build": lambda: amd.Fp4Index.build(corpus), "int8_build": lambda: amd.Int8Index.build(corpus),
                             "binary_build": lambda: amd.BinaryIndex.build(corpus)}, max(3, args.steps // 2), 1)
            b["fp4_bound_ms"] = (corpus.nbytes + f4idx.codes.numel() + f4idx.scales.numel()) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["fp4_share_of_bound"] = b["fp4_bound_ms"] / b["fp4_build"]["median_ms"]
            res["build"] = b
            _progress("build", t0)
        if "stage1" in legs:
            res["stage1"] = stage1_legs(amd, corpus, (f4idx, i8idx, bidx), args.q_len, dev, args.steps, args.warmup)
            _progress("stage1", t0)
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
            r = amd.ShardedRetriever(corpus)
            r6 = amd.ShardedRetriever(corpus, fp4_score_fn=amd.fp6_scores)
            variants = {}
            for name, idx in (("fp4", f4idx), ("int8", i8idx), ("binary", bidx)):
                variants.update({f"{name}_m{m}": (lambda m=m, idx=idx: r.search(pq, k=10, prefilter=idx, n_candidates=m)) for m in MS})
            variants.update({f"fp6_m{m}": (lambda m=m: r6.search(pq, k=10, prefilter=f4idx, n_candidates=m)) for m in MS})
            variants["exact_search"] = lambda: r.search(pq, k=10)
            ts = alternating(variants, max(3, args.steps // 2), 1)
            ts["n_queries"] = 1000
            res["two_stage"] = ts
            _progress("two_stage", t0)
        del corpus, f4idx, i8idx, bidx
        torch.cuda.empty_cache()
    if "pooled" in legs:
        corpus = make_shard(args.docs, POOLED_LEN, dev, seed=4321)
        idxs = (amd.Fp4Index.build(corpus), amd.Int8Index.build(corpus), amd.BinaryIndex.build(corpus))
        res["pooled"] = stage1_legs(amd, corpus, idxs, args.q_len, dev, args.steps, args.warmup)
        _progress("pooled", t0)
        del corpus, idxs
        torch.cuda.empty_cache()
    if "recall" in legs:
        res["recall"] = recall_leg(amd, dev, args.recall_docs)
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(summary(res))
    print(line)


if __name__ == "__main__":
    main()
