"""The FP4 index (msim_f4_*, colpali_amd.Fp4Index) on the headline shard; one JSON object on stdout and a summary in markdown
(not part of bench.py).

    python tools/bench_fp4.py [--out FILE] [--summary profiles/fp4_summary.md] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024]
                              [--legs build,stage1,pooled,two_stage,recall]
    python tools/bench_fp4.py --legs refine --summary profiles/fp4_summary.md      (rewrites only its own section of the summary)
    python tools/bench_fp4.py --dim 320 [--out FILE] [--summary profiles/fp4_wide_summary.md] [--legs build,stage1,two_stage,recall]
    python tools/bench_fp4.py --dim 320 --legs refine --summary profiles/fp4_wide_summary.md   (rewrites only its own section)

--dim 320 measures the 320-wide index (msim_f4w_*, colpali_amd.Fp4WideIndex) on the shard of tools/bench_rerank.py --dim 320
(50 000 x 1024 x 320 bf16 by default): see `main_wide`.

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
  * refine (not in the default list): the list form and the three-stage search.  `fp4_rerank_scores` and `fp6_rerank_scores` at
    1000 x 32 x m in {1000, 4000} and 4 x 32 x m = 4000 on uniform and clustered lists (the generators of tools/bench_rerank.py),
    beside `rerank_scores` on the same lists and `fp4_scores` of the whole shard plus a gather; bound = n_q m rows 65 B / 8 TB/s.
    The cascade search(prefilter=FdeIndex | CentroidIndex, n_candidates=m1, refine=Fp4Index, n_refine=100) at m1 in {1000, 4000}
    beside the same FDE search without refine and search(prefilter=Fp4Index, n_candidates=100), all in one loop (m1 = 4000 is the deep
    top-k's range: the same prefilter= route).  Recall@10 of the
    same configurations on the planted set, with e2m1 and e2m3 query tokens.
    With --dim 320: `fp4_wide_rerank_scores` at 1000 x 32 x m = 1000 and 4 x 32 x m = 4000 on uniform and clustered lists beside
    `rerank_scores` on the same lists and `fp4_wide_scores` plus a gather; bounds = n_q m rows 161 B / 8 TB/s for the list form and
    distinct pages x rows x 640 B / 8 TB/s for the exact rerank.  The cascade search(prefilter=<343-row pooled shard>,
    n_candidates=m1, refine=Fp4WideIndex, n_refine=100) at m1 in {400, 1000} beside the same search without refine and
    search(prefilter=Fp4WideIndex, n_candidates=100); recall@10 of the same variants on the planted set at width 320.
    Every --dim 320 leg carries its e2m3 variant in the same loop: `fp6_wide_scores` beside `fp4_wide_scores` (stage1),
    fp4_wide_score_fn=fp6_wide_scores (two_stage, recall), `fp6_wide_rerank_scores` beside `fp4_wide_rerank_scores` and the e2m3
    hooks in the cascade and its recall (refine).
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


# ------------------------------------------------------------------------------------------------- the list form and the cascade
REFINE_M1 = (1000, 4000)
N_REFINE = 100
REFINE_MARK = "## FP4 candidate rerank and three-stage search"


def rerank_legs(amd, corpus, f4idx, q_len, doc_len, dev, steps):
    """the list form alone: per (n_q, m, list distribution) the four variants alternating in one loop"""
    from tools.bench_rerank import clustered_candidates, uniform_candidates

    n = len(corpus)
    out = {}
    for n_q, m in ((1000, 1000), (1000, 4000), (4, 4000)):
        pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
        full = torch.empty((n_q, n), dtype=torch.float32, device=dev)
        for dist_name, cand in (("uniform", uniform_candidates(n_q, n, m, dev, seed=7)),
                                ("clustered", clustered_candidates(n_q, n, m, dev, seed=7, pool=min(2 * m, n)))):
            s4, s6 = (torch.empty((n_q, m), dtype=torch.float32, device=dev) for _ in range(2))
            leg = alternating({"fp4_rerank": lambda: amd.fp4_rerank_scores(pq, f4idx, cand, out=s4),
                               "fp6_rerank": lambda: amd.fp6_rerank_scores(pq, f4idx, cand, out=s6),
                               "exact_rerank": lambda: amd.rerank(pq, corpus, cand),
                               "fp4_scan_gather": lambda: torch.gather(amd.fp4_scores(pq, f4idx, out=full), 1, cand)},
                              steps if n_q == 4 else max(3, steps // 2), 1)
            leg["bound_ms"] = n_q * m * doc_len * 65 / (HBM_PEAK_GBS * 1e9) * 1e3
            for k in ("fp4", "fp6"):
                leg[f"{k}_share_of_bound"] = leg["bound_ms"] / leg[f"{k}_rerank"]["median_ms"]
            leg["distinct_pages"] = int(torch.unique(cand).numel())
            leg["bits_equal_scan_gather"] = bool(torch.equal(s4.view(torch.int32), torch.gather(full, 1, cand).view(torch.int32)))
            out[f"{n_q}x{q_len}_m{m}_{dist_name}"] = leg
        del full
    return out


def staged_search(amd, r, pq, score_fn, index, m1, k=10, **refine):
    """search behind a first stage of m1 pages: `prefilter=index, n_candidates=m1` for every m1 the top-k takes (amd.TOPK_MAX_K =
    8192: above 1024 the deep selection, the same order); `score_fn` is the first stage's scorer, for the caller's reference"""
    if m1 > amd.TOPK_MAX_K:
        raise NotImplementedError(f"a first stage of {m1} pages: the top-k selects at most {amd.TOPK_MAX_K} per row")
    return r.search(pq, k=k, prefilter=index, n_candidates=m1, **refine)


def cascade_leg(amd, corpus, f4idx, q_len, dev, steps):
    pq = amd.pack_queries(make_queries(1000, q_len, dev, seed=99), dev, compact=False)
    fde, cen = amd.FdeIndex.build(corpus), amd.CentroidIndex.build(corpus)
    r = amd.ShardedRetriever(corpus)
    refine = dict(refine=f4idx, n_refine=N_REFINE)
    variants = {}
    for m1 in REFINE_M1:
        variants[f"fde_refine_m{m1}"] = lambda m1=m1: staged_search(amd, r, pq, amd.fde_scores, fde, m1, **refine)
        variants[f"centroid_refine_m{m1}"] = lambda m1=m1: staged_search(amd, r, pq, amd.centroid_scores, cen, m1, **refine)
        variants[f"fde_only_m{m1}"] = lambda m1=m1: staged_search(amd, r, pq, amd.fde_scores, fde, m1)
    variants["fp4_m100"] = lambda: r.search(pq, k=10, prefilter=f4idx, n_candidates=100)
    out = alternating(variants, max(3, steps // 2), 1)
    out["n_queries"], out["n_refine"] = 1000, N_REFINE
    return out


def refine_recall_leg(amd, dev, n_docs, k=10):
    pages, q = planted_pages(dev, n_docs=n_docs)
    full = amd.pack_passages(pages, dev, batch_size=None)
    del pages
    pq = amd.pack_queries(q, dev, compact=False)
    r4 = amd.ShardedRetriever(full)
    r6 = amd.ShardedRetriever(full, fp4_score_fn=amd.fp6_scores, fp4_rerank_fn=amd.fp6_rerank_scores)
    exact = r4.search(pq, k=k)[1].tolist()
    f4idx, fde, cen = amd.Fp4Index.build(full), amd.FdeIndex.build(full), amd.CentroidIndex.build(full)

    def hits(got):
        return sum(len(set(a) & set(b)) for a, b in zip(exact, got[1].tolist())) / (len(pq) * k)

    out = {"docs": n_docs, "queries": len(pq), "k": k, "n_refine": N_REFINE}
    for code, r in (("e2m1", r4), ("e2m3", r6)):
        for m1 in REFINE_M1:
            out[f"fde_refine_m{m1}_{code}"] = hits(staged_search(amd, r, pq, amd.fde_scores, fde, m1, k, refine=f4idx, n_refine=N_REFINE))
            out[f"centroid_refine_m{m1}_{code}"] = hits(staged_search(amd, r, pq, amd.centroid_scores, cen, m1, k, refine=f4idx,
                                                                    n_refine=N_REFINE))
        out[f"fp4_m100_{code}"] = hits(r.search(pq, k=k, prefilter=f4idx, n_candidates=100))
    for m1 in REFINE_M1:
        out[f"fde_only_m{m1}"] = hits(staged_search(amd, r4, pq, amd.fde_scores, fde, m1, k))
        out[f"centroid_only_m{m1}"] = hits(staged_search(amd, r4, pq, amd.centroid_scores, cen, m1, k))
    return out


def refine_section(res):
    """the summary's section of the refine leg: measured figures only"""
    f = res["refine"]
    L = [REFINE_MARK, "",
         f"`tools/bench_fp4.py --legs refine --steps {res['steps']}` on the headline shard ({res['docs']} pages × {res['doc_len']} rows).  "
         "The variants of a row alternate call by call in one timed loop; median, with the range in brackets.  The bound is n_q × m × "
         "rows × 65 B at 8 TB/s (every listed page read once per entry: no page shared between queries); a share is bound / measured.  "
         "`distinct pages` says how far that holds: where the lists of a batch name each page several times, the repeats come from the "
         "caches, and `rerank_scores` reads a page once for all the queries that list it.", "",
         "| shape, list | `fp4_rerank_scores` (share) | `fp6_rerank_scores` (share) | `rerank_scores` (exact) | `fp4_scores` + gather | bound | "
         "distinct pages | bits = scan |", "|---|---|---|---|---|---|---|---|"]
    for name, leg in f["rerank"].items():
        L += [f"| {name.replace('_', ' ')} | {_ms(leg['fp4_rerank'])} ({leg['fp4_share_of_bound']:.2f}) | {_ms(leg['fp6_rerank'])} "
              f"({leg['fp6_share_of_bound']:.2f}) | {_ms(leg['exact_rerank'])} | {_ms(leg['fp4_scan_gather'])} | {leg['bound_ms']:.2f} ms | "
              f"{leg['distinct_pages']} | {'yes' if leg['bits_equal_scan_gather'] else 'NO'} |"]
    c, rc = f["cascade"], f["recall"]
    L += ["", f"Search at 1000 × 32, k = 10, n_refine = {c['n_refine']}, all alternating in one loop; recall@10 against the exact search on the "
          f"planted {rc['docs']}-page set ({rc['queries']} queries), e2m1 / e2m3 query tokens in the FP4 stages:", "",
         "| search | time | recall@10 (e2m1 / e2m3) |", "|---|---|---|"]
    for m1 in REFINE_M1:
        for first, name in (("fde", "FdeIndex"), ("centroid", "CentroidIndex")):
            key = f"{first}_refine_m{m1}"
            L += [f"| `prefilter={name}, n_candidates={m1}, refine=Fp4Index, n_refine={c['n_refine']}` | {_ms(c[key])} | "
                  f"{rc[key + '_e2m1']:.3f} / {rc[key + '_e2m3']:.3f} |"]
        L += [f"| `prefilter=FdeIndex, n_candidates={m1}` (no refine) | {_ms(c[f'fde_only_m{m1}'])} | {rc[f'fde_only_m{m1}']:.3f} "
              f"(CentroidIndex alone: {rc[f'centroid_only_m{m1}']:.3f}) |"]
    L += [f"| `prefilter=Fp4Index, n_candidates=100` | {_ms(c['fp4_m100'])} | {rc['fp4_m100_e2m1']:.3f} / {rc['fp4_m100_e2m3']:.3f} |", ""]
    return L


def splice_refine_section(text, section, mark=REFINE_MARK):
    """`text` (an earlier summary) with its refine section (the one headed `mark`) replaced by `section` (appended when it has none)"""
    at = text.find(mark)
    if at >= 0:
        nxt = text.find("\n## ", at + 1)
        text = text[:at] + (text[nxt + 1:] if nxt >= 0 else "")
    return text.rstrip("\n") + "\n\n" + "\n".join(section)


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
    if "refine" in res:
        L += [""] + refine_section(res)
    return "\n".join(L) + "\n"


# ------------------------------------------------------------------------------------------------------------------ width 320
WIDE_ROW_BYTES = 161           # 160 code bytes and one scale byte


def _overlap(a, b):
    """whether the (min, max) ranges of two timed variants overlap"""
    return a["min_ms"] <= b["max_ms"] and b["min_ms"] <= a["max_ms"]


def wide_bounds_ms(n_q, q_len, n_d, rows):
    """memory: the index read once and the scores written; matrix cores: three K = 128 instructions per 16 x 16 tile"""
    return {"memory_ms": (rows * WIDE_ROW_BYTES + n_q * n_d * 4) / (HBM_PEAK_GBS * 1e9) * 1e3,
            "matrix_ms": 2.0 * n_q * q_len * rows * 384 / (FP4_PEAK_TFLOPS * 1e12) * 1e3}


def wide_planted(amd, dev, n_docs, dim=320, doc_len=1024, n_q=100, q_len=32, seed=5):
    """the planted set of tools/bench_rerank.py:planted_recall at `dim`: (full shard, pooled shard, packed queries)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    pages = []
    for d0 in range(0, n_docs, 500):
        n = min(500, n_docs - d0)
        topics = torch.randn((n, 48, dim), generator=g, device=dev)
        pick = torch.randint(0, 48, (n, doc_len), generator=g, device=dev)
        rows = torch.gather(topics, 1, pick.unsqueeze(-1).expand(n, doc_len, dim)) + 0.6 * torch.randn((n, doc_len, dim), generator=g, device=dev)
        pages.append(torch.nn.functional.normalize(rows, dim=-1).to(torch.bfloat16))
    pages = torch.cat(pages)
    full = amd.pack_passages(pages, dev, batch_size=None)
    pooler = amd.HierarchicalTokenPooler()
    pooled_list = []
    for d0 in range(0, n_docs, 1000):
        pooled_list += pooler.pool_embeddings(list(pages[d0:d0 + 1000].unbind(0)), pool_factor=3)
    pooled = amd.pack_passages(pooled_list, dev, batch_size=None)
    target = torch.randint(0, n_docs, (n_q,), generator=g, device=dev)
    tok = torch.randint(0, doc_len, (n_q, q_len), generator=g, device=dev)
    q = pages[target.unsqueeze(1), tok].float() + 0.8 * torch.randn((n_q, q_len, dim), generator=g, device=dev) / dim ** 0.5
    return full, pooled, amd.pack_queries(torch.nn.functional.normalize(q, dim=-1).to(torch.bfloat16), dev, compact=False)


def wide_recall_leg(amd, dev, n_docs, k=10):
    full, pooled, pq = wide_planted(amd, dev, n_docs)
    r = amd.ShardedRetriever(full)
    exact = r.search(pq, k=k)[1].tolist()
    idx = amd.Fp4WideIndex.build(full)

    r6 = amd.ShardedRetriever(full, fp4_wide_score_fn=amd.fp6_wide_scores)      # the same index, e2m3 query tokens

    def recall(prefilter, m, retriever=r):
        two = retriever.search(pq, k=k, prefilter=prefilter, n_candidates=m)[1].tolist()
        return sum(len(set(a) & set(b)) for a, b in zip(exact, two)) / (len(pq) * k)

    return {"docs": n_docs, "queries": len(pq), "k": k, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs,
            "fp4_wide_full": {str(m): recall(idx, m) for m in MS}, "fp6_wide_full": {str(m): recall(idx, m, r6) for m in MS},
            "pooled_corpus": {str(m): recall(pooled, m) for m in MS},
            "bytes": {"fp4_wide_full": idx.nbytes, "fp6_wide_full": idx.nbytes, "pooled_corpus": pooled.nbytes, "shard": full.nbytes}}


# ------------------------------------------------------------------------------------- width 320: the list form and the cascade
WIDE_REFINE_M1 = (400, 1000)
WIDE_REFINE_MARK = "## FP4 candidate rerank and three-stage search at width 320"
WIDE_EXACT_ROW_BYTES = 640     # a bf16 row of the 320-wide shard


def wide_rerank_legs(amd, corpus, idx, q_len, doc_len, dev, steps):
    """the wide list form alone: per (n_q, m, list distribution) the three variants alternating in one loop"""
    from tools.bench_rerank import clustered_candidates, make_queries_dim, uniform_candidates

    n = len(corpus)
    out = {}
    for n_q, m in ((1000, 1000), (4, 4000)):
        pq = amd.pack_queries(make_queries_dim(n_q, q_len, 320, dev, seed=99), dev, compact=False)
        full = torch.empty((n_q, n), dtype=torch.float32, device=dev)
        for dist_name, cand in (("uniform", uniform_candidates(n_q, n, m, dev, seed=7)),
                                ("clustered", clustered_candidates(n_q, n, m, dev, seed=7, pool=min(2 * m, n)))):
            s4 = torch.empty((n_q, m), dtype=torch.float32, device=dev)
            s6 = torch.empty((n_q, m), dtype=torch.float32, device=dev)
            leg = alternating({"fp4_wide_rerank": lambda: amd.fp4_wide_rerank_scores(pq, idx, cand, out=s4),
                               "fp6_wide_rerank": lambda: amd.fp6_wide_rerank_scores(pq, idx, cand, out=s6),
                               "exact_rerank": lambda: amd.rerank(pq, corpus, cand),
                               "fp4_wide_scan_gather": lambda: torch.gather(amd.fp4_wide_scores(pq, idx, out=full), 1, cand)},
                              steps if n_q == 4 else max(3, steps // 2), 1)
            leg["distinct_pages"] = int(torch.unique(cand).numel())
            leg["bound_ms"] = n_q * m * doc_len * WIDE_ROW_BYTES / (HBM_PEAK_GBS * 1e9) * 1e3
            leg["exact_bound_ms"] = leg["distinct_pages"] * doc_len * WIDE_EXACT_ROW_BYTES / (HBM_PEAK_GBS * 1e9) * 1e3
            leg["share_of_bound"] = leg["bound_ms"] / leg["fp4_wide_rerank"]["median_ms"]
            leg["exact_vs_fp4_wide"] = leg["exact_rerank"]["median_ms"] / leg["fp4_wide_rerank"]["median_ms"]
            leg["faster_than_exact"] = leg["fp4_wide_rerank"]["max_ms"] < leg["exact_rerank"]["min_ms"]     # the ranges do not overlap
            leg["bits_equal_scan_gather"] = bool(torch.equal(s4.view(torch.int32), torch.gather(full, 1, cand).view(torch.int32)))
            leg["fp6_vs_fp4_wide"] = leg["fp6_wide_rerank"]["median_ms"] / leg["fp4_wide_rerank"]["median_ms"]
            leg["fp6_ranges_overlap"] = _overlap(leg["fp6_wide_rerank"], leg["fp4_wide_rerank"])
            leg["fp6_bits_equal_scan_gather"] = bool(torch.equal(
                s6.view(torch.int32), torch.gather(amd.fp6_wide_scores(pq, idx, out=full), 1, cand).view(torch.int32)))
            out[f"{n_q}x{q_len}_m{m}_{dist_name}"] = leg
        del full
    return out


def wide_cascade_leg(amd, corpus, idx, coarse, q_len, dev, steps):
    from tools.bench_rerank import make_queries_dim

    pq = amd.pack_queries(make_queries_dim(1000, q_len, 320, dev, seed=99), dev, compact=False)
    r = amd.ShardedRetriever(corpus)
    r6 = amd.ShardedRetriever(corpus, fp4_wide_score_fn=amd.fp6_wide_scores, fp4_wide_rerank_fn=amd.fp6_wide_rerank_scores)
    variants = {}
    for m1 in WIDE_REFINE_M1:
        variants[f"pooled_refine_m{m1}"] = lambda m1=m1: r.search(pq, k=10, prefilter=coarse, n_candidates=m1, refine=idx, n_refine=N_REFINE)
        variants[f"pooled_refine_m{m1}_e2m3"] = lambda m1=m1: r6.search(pq, k=10, prefilter=coarse, n_candidates=m1, refine=idx,
                                                                         n_refine=N_REFINE)
        variants[f"pooled_only_m{m1}"] = lambda m1=m1: r.search(pq, k=10, prefilter=coarse, n_candidates=m1)
    variants["fp4_wide_m100"] = lambda: r.search(pq, k=10, prefilter=idx, n_candidates=100)
    variants["fp4_wide_m100_e2m3"] = lambda: r6.search(pq, k=10, prefilter=idx, n_candidates=100)
    out = alternating(variants, max(3, steps // 2), 1)
    out["n_queries"], out["n_refine"], out["coarse_rows_per_doc"] = 1000, N_REFINE, POOLED_LEN
    return out


def wide_refine_recall_leg(amd, dev, n_docs, k=10):
    full, pooled, pq = wide_planted(amd, dev, n_docs)
    r = amd.ShardedRetriever(full)
    exact = r.search(pq, k=k)[1].tolist()
    idx = amd.Fp4WideIndex.build(full)

    def hits(got):
        return sum(len(set(a) & set(b)) for a, b in zip(exact, got[1].tolist())) / (len(pq) * k)

    out = {"docs": n_docs, "queries": len(pq), "k": k, "n_refine": N_REFINE, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs}
    r6 = amd.ShardedRetriever(full, fp4_wide_score_fn=amd.fp6_wide_scores, fp4_wide_rerank_fn=amd.fp6_wide_rerank_scores)
    for m1 in WIDE_REFINE_M1:
        out[f"pooled_refine_m{m1}"] = hits(r.search(pq, k=k, prefilter=pooled, n_candidates=m1, refine=idx, n_refine=N_REFINE))
        out[f"pooled_refine_m{m1}_e2m3"] = hits(r6.search(pq, k=k, prefilter=pooled, n_candidates=m1, refine=idx, n_refine=N_REFINE))
        out[f"pooled_only_m{m1}"] = hits(r.search(pq, k=k, prefilter=pooled, n_candidates=m1))
    out["fp4_wide_m100"] = hits(r.search(pq, k=k, prefilter=idx, n_candidates=100))
    out["fp4_wide_m100_e2m3"] = hits(r6.search(pq, k=k, prefilter=idx, n_candidates=100))
    return out


def wide_refine_section(res):
    """the wide summary's section of the refine leg: measured figures only"""
    f = res["refine"]
    L = [WIDE_REFINE_MARK, "",
         f"`tools/bench_fp4.py --dim 320 --legs refine --steps {res['steps']}` on the 320-wide shard ({res['docs']} pages × {res['doc_len']} "
         "rows).  The variants of a row alternate call by call in one timed loop; median, with the range in brackets.  The list form's "
         "bound is n_q × m × rows × 161 B at 8 TB/s (every listed page read once per entry: no page shared between queries); the exact "
         "rerank's is distinct pages × rows × 640 B at 8 TB/s (a page read once for all the queries that list it); a share is bound / "
         "measured.  `faster` says whether the list form's whole range lies below the exact rerank's in this loop.", "",
         "| shape, list | `fp4_wide_rerank_scores` (share) | `rerank_scores` (exact) | exact / list form | faster | `fp4_wide_scores` + gather | "
         "bound, list form | bound, exact | distinct pages | bits = scan |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, leg in f["rerank"].items():
        L += [f"| {name.replace('_', ' ')} | {_ms(leg['fp4_wide_rerank'])} ({leg['share_of_bound']:.2f}) | {_ms(leg['exact_rerank'])} | "
              f"{leg['exact_vs_fp4_wide']:.2f} × | {'yes' if leg['faster_than_exact'] else 'NO'} | {_ms(leg['fp4_wide_scan_gather'])} | "
              f"{leg['bound_ms']:.2f} ms | {leg['exact_bound_ms']:.2f} ms | {leg['distinct_pages']} | "
              f"{'yes' if leg['bits_equal_scan_gather'] else 'NO'} |"]
    L += ["", "The same lists with e2m3 query tokens (`fp6_wide_rerank_scores`, alternating with the rows above in the same loop); "
          "`ranges` says whether the two list forms' ranges overlap:", "",
          "| shape, list | `fp6_wide_rerank_scores` | `fp4_wide_rerank_scores` | e2m3 / e2m1 | ranges | bits = e2m3 scan |", "|---|---|---|---|---|---|"]
    for name, leg in f["rerank"].items():
        L += [f"| {name.replace('_', ' ')} | {_ms(leg['fp6_wide_rerank'])} | {_ms(leg['fp4_wide_rerank'])} | {leg['fp6_vs_fp4_wide']:.3f} | "
              f"{'overlap' if leg['fp6_ranges_overlap'] else 'APART'} | {'yes' if leg['fp6_bits_equal_scan_gather'] else 'NO'} |"]
    c, rc = f["cascade"], f["recall"]
    L += ["", f"Search at 1000 × 32, k = 10, n_refine = {c['n_refine']}, all alternating in one loop (the pooled shard of the timing has "
          f"{c['coarse_rows_per_doc']} random rows per page); recall@10 against the exact search on the planted {rc['docs']}-page set at "
          f"width 320 ({rc['queries']} queries, pooled pages of {rc['pooled_rows_per_doc']:.0f} rows):", "",
          "| search | time | recall@10 |", "|---|---|---|"]
    for m1 in WIDE_REFINE_M1:
        L += [f"| `prefilter=pooled, n_candidates={m1}, refine=Fp4WideIndex, n_refine={c['n_refine']}` | {_ms(c[f'pooled_refine_m{m1}'])} | "
              f"{rc[f'pooled_refine_m{m1}']:.3f} |",
              f"| the same with the e2m3 hooks (`fp6_wide_rerank_scores`) | {_ms(c[f'pooled_refine_m{m1}_e2m3'])} | "
              f"{rc[f'pooled_refine_m{m1}_e2m3']:.3f} |",
              f"| `prefilter=pooled, n_candidates={m1}` (no refine) | {_ms(c[f'pooled_only_m{m1}'])} | {rc[f'pooled_only_m{m1}']:.3f} |"]
    L += [f"| `prefilter=Fp4WideIndex, n_candidates=100` | {_ms(c['fp4_wide_m100'])} | {rc['fp4_wide_m100']:.3f} |",
          f"| the same with `fp4_wide_score_fn=fp6_wide_scores` | {_ms(c['fp4_wide_m100_e2m3'])} | {rc['fp4_wide_m100_e2m3']:.3f} |", ""]
    return L


def wide_summary(res):
    L = ["# FP4 index at width 320: measured on one MI355X", "",
         f"`tools/bench_fp4.py --dim 320 --steps {res['steps']} --warmup {res['warmup']}` on the 320-wide shard ({res['docs']} pages × "
         f"{res['doc_len']} rows, bf16), queries of 32 tokens.  The variants of a leg alternate call by call in one timed loop; median, "
         "with the range in brackets.  The bounds are derived (8 TB/s; 10 PFLOPS dense FP4, three K = 128 instructions per 16 × 16 "
         "tile), not measured; a share is bound / measured.", ""]
    if "bytes" in res:
        b = res["bytes"]
        L += [f"Sizes: shard {b['shard'] / 1e9:.2f} GB, `Fp4WideIndex` {b['fp4_wide'] / 1e9:.2f} GB ({b['fp4_wide'] / b['shard']:.3f} of it).", ""]
    if "build" in res:
        b = res["build"]
        L += [f"Build: `Fp4WideIndex.build` {_ms(b['fp4_wide_build'])} in one launch, {b['share_of_bound']:.2f} of its {b['bound_ms']:.2f} ms bound "
              "(the shard read once, codes and scales written).", ""]
    if "stage1" in res:
        L += ["## Stage 1", "", "| | `fp4_wide_scores` | `fp6_wide_scores` | exact scan | ratio | memory bound (share) | matrix-core bound (share) |",
              "|---|---|---|---|---|---|---|"]
        for n, leg in res["stage1"].items():
            bd = leg["bounds"]
            L += [f"| {n} × 32 | {_ms(leg['fp4_wide_scores'])} | {_ms(leg['fp6_wide_scores'])} | {_ms(leg['exact_scan'])} | {leg['exact_vs_fp4_wide']:.2f} × | "
                  f"{bd['memory_ms']:.2f} ms ({bd['memory_ms'] / leg['fp4_wide_scores']['median_ms']:.2f}) | "
                  f"{bd['matrix_ms']:.2f} ms ({bd['matrix_ms'] / leg['fp4_wide_scores']['median_ms']:.2f}) |"]
        L += ["", "Ratio, bounds and shares are `fp4_wide_scores`'.  e2m3 query tokens against the same index:"]
        for n, leg in res["stage1"].items():
            L += [f"{n} × 32: `fp6_wide_scores` / `fp4_wide_scores` = {leg['fp6_vs_fp4_wide']:.3f}; the two ranges "
                  f"{'overlap' if leg['fp6_ranges_overlap'] else 'are APART'} in this loop."]
        L += [""]
    if "two_stage" in res:
        t = res["two_stage"]
        L += ["## Two-stage search at 1000 × 32, k = 10", "", "| | time | exact search / this |", "|---|---|---|"]
        ex = t["exact_search"]
        for key, name in [(f"fp4_wide_m{m}", f"`prefilter=<Fp4WideIndex>`, m = {m}") for m in MS] + \
                         [(f"fp6_wide_m{m}", f"the same with `fp4_wide_score_fn=fp6_wide_scores`, m = {m}") for m in MS] + \
                         [("pooled_m100", f"`prefilter=<PackedCorpus of {t['coarse_rows_per_doc']}-row pages>`, m = 100"), ("exact_search", "exact search")]:
            L += [f"| {name} | {_ms(t[key])} | {ex['median_ms'] / t[key]['median_ms']:.2f} |"]
        a = t["fp4_wide_m100"]
        apart = a["max_ms"] < ex["min_ms"]
        L += ["", f"Two-stage search at m = 100 against the exact search of the same shard in the same loop: {ex['median_ms'] / a['median_ms']:.2f} × "
              f"faster; the two ranges {'do not overlap' if apart else 'OVERLAP: the claim does not hold in this run'}.", ""]
    if "recall" in res:
        r = res["recall"]
        L += [f"## Recall@10 against the exact search, planted {r['docs']}-page set at width 320 ({r['queries']} queries)", "",
              "| first stage | bytes | m = 100 | m = 400 | m = 1000 |", "|---|---|---|---|---|"]
        for key, name in (("fp4_wide_full", "`Fp4WideIndex`, full pages"),
                          ("fp6_wide_full", "`Fp4WideIndex`, full pages, e2m3 queries (`fp6_wide_scores`)"),
                          ("pooled_corpus", f"pooled `PackedCorpus` ({r['pooled_rows_per_doc']:.0f} rows per page)")):
            L += [f"| {name} | {r['bytes'][key] / 1e6:.0f} MB | " + " | ".join(f"{r[key][str(m)]:.3f}" for m in MS) + " |"]
    if "refine" in res:
        L += [""] + wide_refine_section(res)
    return "\n".join(L) + "\n"


def main_wide(args):
    """--dim 320: index bytes, build, stage 1 beside the exact 320-wide scan, two-stage search beside the exact search and the
    pooled-prefilter two-stage search, recall@10 on the planted set; --legs refine: the list form and the three-stage search."""
    import colpali_amd as amd
    from tools.bench_rerank import make_queries_dim, make_shard_dim

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    docs = 50_000 if args.docs is None else args.docs
    t0 = time.perf_counter()
    res = {"tool": "bench_fp4", "dim": 320, "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len, "steps": args.steps,
           "warmup": args.warmup, "hbm_peak_GBps": HBM_PEAK_GBS, "fp4_peak_TFLOPs": FP4_PEAK_TFLOPS}
    if "refine" in legs:
        corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
        idx = amd.Fp4WideIndex.build(corpus)
        _progress("shard and index", t0)
        res["refine"] = {"rerank": wide_rerank_legs(amd, corpus, idx, args.q_len, args.doc_len, dev, args.steps)}
        _progress("refine: list form", t0)
        coarse = make_shard_dim(docs, POOLED_LEN, 320, dev, seed=4321)
        res["refine"]["cascade"] = wide_cascade_leg(amd, corpus, idx, coarse, args.q_len, dev, args.steps)
        _progress("refine: cascade", t0)
        del corpus, idx, coarse
        torch.cuda.empty_cache()
        res["refine"]["recall"] = wide_refine_recall_leg(amd, dev, args.recall_docs)
        _progress("refine: recall", t0)
    if legs & {"build", "stage1", "two_stage"}:
        corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
        idx = amd.Fp4WideIndex.build(corpus)
        _progress("shard and index", t0)
        res["bytes"] = {"shard": corpus.nbytes, "fp4_wide": idx.nbytes}
        rows = int(idx.codes.shape[0])
        if "build" in legs:
            b = alternating({"fp4_wide_build": lambda: amd.Fp4WideIndex.build(corpus)}, max(3, args.steps // 2), 1)
            b["bound_ms"] = (corpus.nbytes + rows * WIDE_ROW_BYTES) / (HBM_PEAK_GBS * 1e9) * 1e3
            b["share_of_bound"] = b["bound_ms"] / b["fp4_wide_build"]["median_ms"]
            res["build"] = b
            _progress("build", t0)
        if "stage1" in legs:
            res["stage1"] = {}
            for n in (4, 1000):
                pq = amd.pack_queries(make_queries_dim(n, args.q_len, 320, dev, seed=99), dev, compact=False)
                out = torch.empty((n, len(idx)), dtype=torch.float32, device=dev)
                out6 = torch.empty((n, len(idx)), dtype=torch.float32, device=dev)
                leg = alternating({"fp4_wide_scores": lambda: amd.fp4_wide_scores(pq, idx, out=out),
                                   "fp6_wide_scores": lambda: amd.fp6_wide_scores(pq, idx, out=out6),
                                   "exact_scan": lambda: amd.maxsim_scores(pq, corpus)},
                                  args.steps if n == 4 else max(3, args.steps // 2), args.warmup if n == 4 else 1)
                leg["bounds"] = wide_bounds_ms(n, args.q_len, len(idx), rows)
                leg["exact_vs_fp4_wide"] = leg["exact_scan"]["median_ms"] / leg["fp4_wide_scores"]["median_ms"]
                leg["fp6_vs_fp4_wide"] = leg["fp6_wide_scores"]["median_ms"] / leg["fp4_wide_scores"]["median_ms"]
                leg["fp6_ranges_overlap"] = _overlap(leg["fp6_wide_scores"], leg["fp4_wide_scores"])
                res["stage1"][str(n)] = leg
                del out, out6
            _progress("stage1", t0)
        if "two_stage" in legs:
            pq = amd.pack_queries(make_queries_dim(1000, args.q_len, 320, dev, seed=99), dev, compact=False)
            coarse = make_shard_dim(docs, POOLED_LEN, 320, dev, seed=4321)
            r = amd.ShardedRetriever(corpus)
            r6 = amd.ShardedRetriever(corpus, fp4_wide_score_fn=amd.fp6_wide_scores)
            variants = {f"fp4_wide_m{m}": (lambda m=m: r.search(pq, k=10, prefilter=idx, n_candidates=m)) for m in MS}
            variants.update({f"fp6_wide_m{m}": (lambda m=m: r6.search(pq, k=10, prefilter=idx, n_candidates=m)) for m in MS})
            variants["pooled_m100"] = lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=100)
            variants["exact_search"] = lambda: r.search(pq, k=10)
            ts = alternating(variants, max(3, args.steps // 2), 1)
            ts["n_queries"], ts["coarse_rows_per_doc"] = 1000, POOLED_LEN
            res["two_stage"] = ts
            del coarse
            _progress("two_stage", t0)
        del corpus, idx
        torch.cuda.empty_cache()
    if "recall" in legs:
        res["recall"] = wide_recall_leg(amd, dev, args.recall_docs)
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        text = wide_summary(res)
        if legs == {"refine"} and os.path.exists(args.summary):            # the other legs' recorded figures stay
            with open(args.summary) as f:
                text = splice_refine_section(f.read(), wide_refine_section(res), WIDE_REFINE_MARK)
        with open(args.summary, "w") as f:
            f.write(text)
    print(line)


def _progress(what, t0):
    print(f"[bench_fp4] {what} at {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128, choices=(128, 320), help="320: the Fp4WideIndex on the 320-wide shard")
    ap.add_argument("--docs", type=int, default=None, help="default: 125 000 at width 128, 50 000 at width 320 (the same bytes)")
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
    if args.dim == 320:
        return main_wide(args)
    if args.docs is None:
        args.docs = 125_000
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_fp4", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "steps": args.steps,
           "warmup": args.warmup, "hbm_peak_GBps": HBM_PEAK_GBS, "fp4_peak_TFLOPs": FP4_PEAK_TFLOPS}
    if "refine" in legs:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        f4idx = amd.Fp4Index.build(corpus)
        _progress("shard and index", t0)
        res["refine"] = {"rerank": rerank_legs(amd, corpus, f4idx, args.q_len, args.doc_len, dev, args.steps)}
        _progress("refine: list form", t0)
        res["refine"]["cascade"] = cascade_leg(amd, corpus, f4idx, args.q_len, dev, args.steps)
        _progress("refine: cascade", t0)
        del corpus, f4idx
        torch.cuda.empty_cache()
        res["refine"]["recall"] = refine_recall_leg(amd, dev, args.recall_docs)
        _progress("refine: recall", t0)
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
        text = summary(res)
        if legs == {"refine"} and os.path.exists(args.summary):            # the other legs' recorded figures stay
            with open(args.summary) as f:
                text = splice_refine_section(f.read(), refine_section(res))
        with open(args.summary, "w") as f:
            f.write(text)
    print(line)


if __name__ == "__main__":
    main()
