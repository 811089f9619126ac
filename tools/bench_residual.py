"""The residual-compressed corpus (msim_res_*, colpali_amd.ResidualCorpus) on the headline shard; one JSON object on stdout (not part
of bench.py).

    python tools/bench_residual.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--legs build,rerank,two_stage,recall,scan,align,gather]

Legs, each timed with device events after a warm-up, for 2 and 4 residual bits (K = 1024 centroids):
  * build: `train_residual_codec` on the residuals of 2^18 sampled rows, and `ResidualCorpus.build` with a given index, cutoffs
    and weights (the encode pass alone); `nbytes` beside the bf16 corpus's.
  * rerank: `residual_rerank_scores` (msim_res_candidates) at 1000 x 32 x m = 100 and at 4 x 32 x m = 1000, uniform and clustered
    lists (tools/bench_rerank.py; a cluster of 10 queries draws its lists from a pool of max(200, 2 m) pages), beside `rerank` over
    `rc.decompress()` on the SAME lists in the same run, and whether the two agree bit for bit.  The compressed rerank reads 34 / 66 bytes per row from HBM but 256 bytes per row of centroids from L2, and it
    reads a page once per entry where K1c reads it once per group of queries: which one is faster is what this leg is for.
  * two_stage: ShardedRetriever(rc).search(prefilter=rc.index, n_candidates=m) at 1000 x 32 for m in {100, 400, 1000}, beside the
    same search over the bf16 shard with the same centroid index.
  * recall: recall@10 and the mean absolute score error of the two-stage search over the compressed shard against the exact search
    on the planted 10 000-page set of tools/bench_fde.py:planted_pages (centroids and codec trained on that set).
  * scan (not in the default legs): the full scan `residual_scores` (msim_res_scores) at 4 x 32, 32 x 32 and 1000 x 32 queries, beside
    `maxsim_scores` over `rc.decompress()` at the same batches and `residual_rerank_scores` over ALL ids at 4 x 32 (the only way to
    scan such a shard without it: every page decoded once per query).  The variants of one batch ALTERNATE step by step inside one
    timing loop, and the outputs' bit-equality at those sizes is recorded.  `--scan-ref 0` times `residual_scores` alone (A/B runs
    of a measurement build).
  * align (not in the default legs): `residual_align` (msim_res_align_candidates) at 1000 x 32 queries x k = 10 hits, with and
    without `maps`, beside the only way there was before it: read the ids back, `rc.decompress(local ids)`, `align` over that copy
    (the read-back, the per-page decode launches and the bf16 copy are all inside the timed region), and beside `align` over a
    RESIDENT `rc.decompress()` (K1a itself: what the in-kernel decode costs).  Variants alternate step by step; bit-equality of the
    outputs is recorded.
  * gather (not in the default legs): `residual_gather_pages` (msim_res_gather_pages) on `[1000, 8]` ids beside `gather_pages` over a
    RESIDENT `rc.decompress()` (whose 256 bytes per row are what the compressed shard exists to avoid), alternating, with the bytes
    compared.

    python tools/bench_residual.py --dim 320 [--out FILE] [--summary profiles/residual_wide_summary.md] [--docs 50000]

--dim 320 measures the 320-wide compressed shard (msim_cent_wide_*, msim_res_wide_*, colpali_amd.ResidualWideCorpus) on the shard of
tools/bench_rerank.py --dim 320 (50 000 x 1024 x 320 bf16, 32.8 GB), for 2 and 4 residual bits: the encode (centroid codes, then
residuals), `decompress()`, `residual_wide_rerank_scores` beside `rerank_scores` over a resident `decompress()` on the same uniform
and clustered lists (1000 x 32 x m = 100 and 4 x 32 x m = 1000) with their bit-equality, the two-stage search
`prefilter=rc.index` at m = 100 / 400 / 1000 beside the same search over the bf16 shard, and recall@10 and the mean score error on
the planted 320-wide set of tools/bench_fp4.py --dim 320.  `--dim 320 --legs scan` times the full scan alone -- `residual_wide_scores`
(msim_res_wide_scores) at 4 x 32, 32 x 32 and 1000 x 32 queries beside `maxsim_scores` over a resident `rc.decompress()` and, at 4 x 32,
`residual_wide_rerank_scores` over all ids, checks the bit identity with that rerank, and APPENDS its table to --summary.  One run; the variants of a comparison alternate step by step inside
one timing loop and every figure is a median (min - max).  `--dim 320 --legs align,gather` (either or both) runs the align and gather
legs above on the wide classes -- `residual_wide_align` / `residual_wide_gather_pages` (msim_res_wide_align_candidates,
msim_res_wide_gather_pages) beside the decompress-then-call detour (ids read back, `rc.decompress(local ids)`, then `align` /
`gather_pages` over that copy) and beside the call over a resident `rc.decompress()`, the three alternating in one loop -- and
APPENDS its table to --summary.
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
from tools.bench_rerank import clustered_candidates, timed, uniform_candidates  # noqa: E402

MS = (100, 400, 1000)
BITS = (2, 4)
K = 1024
SHAPES = ((1000, 100), (4, 1000))           # (queries, list length)


def rerank_leg(amd, rc, dec, n_q, m, q_len, dev, steps, warmup):
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    out = {}
    lists = (("uniform", uniform_candidates(n_q, len(rc), m, dev, 7)),
             ("clustered", clustered_candidates(n_q, len(rc), m, dev, 8, pool=max(200, 2 * m))))
    for name, cand in lists:
        scores = torch.empty((n_q, m), dtype=torch.float32, device=dev)
        leg = {"residual": timed(lambda: amd.residual_rerank_scores(pq, rc, cand, out=scores), steps, warmup),
               "bf16_decompressed": timed(lambda: amd.rerank(pq, dec, cand, out=scores), steps, warmup)}
        leg["residual_over_bf16"] = leg["residual"]["median_ms"] / leg["bf16_decompressed"]["median_ms"]
        got = amd.residual_rerank_scores(pq, rc, cand)[0]
        want = amd.rerank(pq, dec, cand)
        torch.cuda.synchronize()
        leg["bit_identical"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        rows = int(rc.lengths[0]) * n_q * m
        leg["residual_row_bytes_per_s"] = rows * (2 + 16 * rc.bits) / (leg["residual"]["median_ms"] * 1e-3)
        out[name] = leg
    return out


def timed_alternating(fns, steps, warmup):
    """`timed` for several variants at once: every step runs each variant in turn, so a drift of the clock hits all of them alike"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    evs = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)] for name in fns}
    torch.cuda.synchronize()
    for i in range(steps):
        for name, fn in fns.items():
            evs[name][i][0].record()
            fn()
            evs[name][i][1].record()
    torch.cuda.synchronize()
    out = {}
    for name in fns:
        ms = sorted(a.elapsed_time(b) for a, b in evs[name])
        out[name] = {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}
    return out


SCAN_BATCHES = (4, 32, 1000)


def scan_leg(amd, rc, dec, q_len, dev, steps, warmup):
    """dec=None: the scan alone.  A `ResidualWideCorpus` is scanned by `residual_wide_scores` beside `residual_wide_rerank_scores`."""
    n = len(rc)
    wide = isinstance(rc, amd.ResidualWideCorpus)
    scan_fn, rerank_fn = (amd.residual_wide_scores, amd.residual_wide_rerank_scores) if wide else (amd.residual_scores, amd.residual_rerank_scores)
    out = {}
    for n_q in SCAN_BATCHES:
        if wide:
            from tools.bench_rerank import make_queries_dim

            pq = amd.pack_queries(make_queries_dim(n_q, q_len, rc.width, dev, seed=99), dev, compact=False)
        else:
            pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
        scores = torch.empty((n_q, n), dtype=torch.float32, device=dev)
        fns = {"residual_scan": lambda: scan_fn(pq, rc, out=scores)}
        if dec is not None:
            ref = torch.empty((n_q, n), dtype=torch.float32, device=dev)
            fns["bf16_decompressed_scan"] = lambda: amd.maxsim_scores(pq, dec, out=ref)
            if n_q == SCAN_BATCHES[0]:
                ids = (torch.arange(n, device=dev) + rc.id_base).expand(n_q, n).contiguous()
                listed = torch.empty((n_q, n), dtype=torch.float32, device=dev)
                fns["residual_rerank_all_ids"] = lambda: rerank_fn(pq, rc, ids, out=listed)
        leg = timed_alternating(fns, steps, warmup)
        if dec is not None:
            leg["residual_over_bf16"] = leg["residual_scan"]["median_ms"] / leg["bf16_decompressed_scan"]["median_ms"]
            # (width 320: queries of one length in at most four 32-token tiles send the decompressed scan to another kernel, whose token
            # sum has another fp32 order -- the bit identity that is claimed there is the one with the rerank)
            leg["bit_identical_to_bf16_scan"] = bool(torch.equal(scores.view(torch.int32), ref.view(torch.int32)))
            leg["max_abs_diff_to_bf16_scan"] = float((scores - ref).abs().nan_to_num(0.0).max())
            if "residual_rerank_all_ids" in fns:
                leg["scan_over_rerank_all_ids"] = leg["residual_scan"]["median_ms"] / leg["residual_rerank_all_ids"]["median_ms"]
                leg["bit_identical_to_rerank_all_ids"] = bool(torch.equal(scores.view(torch.int32), listed.view(torch.int32)))
                del ids, listed
            del ref
        passes = (n_q * q_len + 127) // 128
        leg["passes_over_the_shard"] = passes
        leg["row_bytes_per_s"] = int(rc.codes.shape[0]) * (2 + rc.width // 8 * rc.bits) * passes / (leg["residual_scan"]["median_ms"] * 1e-3)
        out[f"{n_q}x{q_len}"] = leg
        del scores, pq
    return out


ALIGN_SHAPE = (1000, 10)                    # (queries, hits per query)
GATHER_SHAPE = (1000, 8)                    # the ids of a mined batch


def _rows_fns(amd, rc):
    """(fused align, fused gather, width) of the shard's class"""
    if isinstance(rc, amd.ResidualWideCorpus):
        return amd.residual_wide_align, amd.residual_wide_gather_pages, rc.width
    return amd.residual_align, amd.residual_gather_pages, 128


def _queries(amd, rc, n_q, q_len, dev):
    if isinstance(rc, amd.ResidualWideCorpus):
        from tools.bench_rerank import make_queries_dim

        return amd.pack_queries(make_queries_dim(n_q, q_len, rc.width, dev, seed=99), dev, compact=False)
    return amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)


def align_leg(amd, rc, dec, q_len, dev, steps, warmup):
    """the keys keep their names at both widths: `residual_align` is the fused call of the shard's class"""
    n_q, k = ALIGN_SHAPE
    fused = _rows_fns(amd, rc)[0]
    pq = _queries(amd, rc, n_q, q_len, dev)
    ids = uniform_candidates(n_q, len(rc), k, dev, 7) + rc.id_base
    listed = torch.arange(n_q * k, device=dev).reshape(n_q, k)
    R = int(rc.lengths.max())
    out = {}
    for maps in (False, True):
        def via_decompress():
            part = rc.decompress((ids - rc.id_base).reshape(-1))       # reads the ids back: one synchronisation per call
            return amd.align(pq, part, listed, maps=maps, max_rows=R)

        fns = {"residual_align": lambda: fused(pq, rc, ids, maps=maps, max_rows=R), "decompress_then_align": via_decompress,
               "align_resident_bf16": lambda: amd.align(pq, dec, ids, maps=maps, max_rows=R)}       # K1a itself: what the decode costs
        leg = timed_alternating(fns, steps, warmup)
        leg["residual_over_resident_bf16"] = leg["residual_align"]["median_ms"] / leg["align_resident_bf16"]["median_ms"]
        leg["residual_over_decompress"] = leg["residual_align"]["median_ms"] / leg["decompress_then_align"]["median_ms"]
        got, want = fns["residual_align"](), via_decompress()
        torch.cuda.synchronize()
        same = torch.equal(got.best_sim.view(torch.int32), want.best_sim.view(torch.int32)) and torch.equal(got.best_row, want.best_row)
        if maps:
            same = same and torch.equal(got.sims.view(torch.int32), want.sims.view(torch.int32))
        leg["bit_identical"] = bool(same)
        rows = int(rc.lengths[(ids - rc.id_base).reshape(-1).cpu()].sum())
        leg["rows_decoded_per_s"] = rows / (leg["residual_align"]["median_ms"] * 1e-3)
        out["maps" if maps else "no_maps"] = leg
        del got, want
        torch.cuda.empty_cache()
    return out


def gather_leg(amd, rc, dec, dev, steps, warmup, detour=False):
    """detour=True adds the way round there was before the fused call: ids read back, `rc.decompress(local ids)`, `gather_pages`"""
    n_q, n_neg = GATHER_SHAPE
    _, fused, width = _rows_fns(amd, rc)
    ids = uniform_candidates(n_q, len(rc), n_neg, dev, 11) + rc.id_base
    pad = int(rc.lengths.max())
    box = torch.empty((n_q, n_neg, pad, width), dtype=rc.dtype, device=dev)
    ref = torch.empty_like(box)
    fns = {"residual_gather_pages": lambda: fused(rc, ids, pad, out=box),
           "gather_pages_resident_bf16": lambda: amd.gather_pages(dec, ids, pad, out=ref)}
    if detour:
        listed = torch.arange(n_q * n_neg, device=dev).reshape(n_q, n_neg)
        via = torch.empty_like(box)

        def via_decompress():
            part = rc.decompress((ids - rc.id_base).reshape(-1))       # reads the ids back: one synchronisation per call
            return amd.gather_pages(part, listed, pad, out=via)

        fns["decompress_then_gather"] = via_decompress
    leg = timed_alternating(fns, steps, warmup)
    leg["residual_over_bf16"] = leg["residual_gather_pages"]["median_ms"] / leg["gather_pages_resident_bf16"]["median_ms"]
    leg["bit_identical"] = bool(torch.equal(box.view(torch.int16), ref.view(torch.int16)))
    if detour:
        leg["residual_over_decompress"] = leg["residual_gather_pages"]["median_ms"] / leg["decompress_then_gather"]["median_ms"]
        leg["bit_identical"] = leg["bit_identical"] and bool(torch.equal(box.view(torch.int16), via.view(torch.int16)))
    leg["bytes_written_per_s"] = box.numel() * 2 / (leg["residual_gather_pages"]["median_ms"] * 1e-3)
    return leg


def recall_leg(amd, dev, n_docs, k=10):
    pages, q = planted_pages(dev, n_docs=n_docs)
    full = amd.pack_passages(pages, dev, batch_size=None)
    del pages
    pq = amd.pack_queries(q, dev, compact=False)
    exact_s, exact_i = amd.ShardedRetriever(full).search(pq, k=k)
    index = amd.CentroidIndex.build(full, n_centroids=K)
    out = {"docs": n_docs, "queries": len(pq), "k": k, "n_centroids": K}
    for bits in BITS:
        rc = amd.ResidualCorpus.build(full, index=index, bits=bits)
        r = amd.ShardedRetriever(rc)
        leg = {}
        for m in MS:
            s, i = r.search(pq, k=k, prefilter=rc.index, n_candidates=m)
            leg[str(m)] = sum(len(set(a) & set(b)) for a, b in zip(exact_i.tolist(), i.tolist())) / (len(pq) * k)
        # the codec's own error: the exact top-k pages rescored from the compressed rows
        approx = amd.rerank(pq, rc, exact_i)
        ok = exact_i >= 0
        leg["mean_abs_score_error"] = float((approx - exact_s)[ok].abs().mean())
        leg["mean_exact_score"] = float(exact_s[ok].mean())
        out[f"bits{bits}"] = leg
        del rc, r
    return out


def _fmt(t):
    return f"{t['median_ms']:.2f} ({t['min_ms']:.2f} - {t['max_ms']:.2f})"


def wide_summary(res) -> str:
    """profiles/residual_wide_summary.md from one --dim 320 result"""
    L = ["# The residual-compressed shard at width 320 (ColQwen3)", "",
         f"`tools/bench_residual.py --dim 320 --steps {res['steps']} --warmup {res['warmup']}` on the 320-wide shard ({res['docs']} pages x "
         f"{res['doc_len']} rows x 320 bf16, {res['corpus_bytes'] / 1e9:.1f} GB), K = {res['n_centroids']} centroids.  One run; the variants of "
         "a comparison alternate step by step inside one timing loop; every time is a median (min - max) in ms.", ""]
    L += ["## Size and build", "", "| bits | shard bytes | bytes per row | share of bf16 | centroid encode | residual encode | decompress() |",
          "|---|---|---|---|---|---|---|"]
    for bits in BITS:
        b = res[f"bits{bits}"]
        L.append(f"| {bits} | {b['nbytes'] / 1e9:.2f} GB | {b['bytes_per_row']:.1f} | {b['nbytes'] / res['corpus_bytes']:.3f} | "
                 f"{_fmt(res['centroid_encode'])} | {_fmt(b['encode'])} | {_fmt(b['decompress'])} |")
    L += ["", "## Candidate rerank: from the compressed rows beside a resident decompressed copy", "",
          "| bits | queries x m | lists | residual_wide_rerank_scores | rerank_scores over decompress() | ratio | same bits |", "|---|---|---|---|---|---|---|"]
    for bits in BITS:
        for shape, by_list in res[f"bits{bits}"]["rerank"].items():
            for name, leg in by_list.items():
                L.append(f"| {bits} | {shape} | {name} | {_fmt(leg['residual'])} | {_fmt(leg['bf16_decompressed'])} | "
                         f"{leg['residual_over_bf16']:.2f} | {leg['bit_identical']} |")
    L += ["", "## Two-stage search, 1000 x 32 queries, k = 10: prefilter=rc.index over the compressed shard beside the bf16 shard", "",
          "| bits | n_candidates | compressed shard | bf16 shard |", "|---|---|---|---|"]
    for bits in BITS:
        for m, leg in res[f"bits{bits}"]["two_stage"].items():
            L.append(f"| {bits} | {m} | {_fmt(leg['residual'])} | {_fmt(leg['bf16'])} |")
    r = res["recall"]
    L += ["", f"## Recall@10 against the exact search, planted {r['docs']}-page set at width 320 ({r['queries']} queries)", "",
          "| bits | m = 100 | m = 400 | m = 1000 | mean abs score error | mean exact score |", "|---|---|---|---|---|---|"]
    for bits in BITS:
        b = r[f"bits{bits}"]
        L.append(f"| {bits} | {b['100']:.3f} | {b['400']:.3f} | {b['1000']:.3f} | {b['mean_abs_score_error']:.4f} | {b['mean_exact_score']:.3f} |")
    return "\n".join(L) + "\n"


def wide_scan_summary(res) -> str:
    """the section `--dim 320 --legs scan` appends to profiles/residual_wide_summary.md"""
    L = ["", "## Full scan: residual_wide_scores beside maxsim_scores over a resident decompress()", "",
         f"`tools/bench_residual.py --dim 320 --legs scan --steps {res['steps']} --warmup {res['warmup']}` on {res['docs']} pages x "
         f"{res['doc_len']} rows x 320 bf16 ({res['corpus_bytes'] / 1e9:.1f} GB), K = {res['n_centroids']}; the variants alternate step by step "
         "inside one timing loop; median (min - max) in ms.  The rerank over all ids is timed at the smallest batch only.", "",
         "| bits | queries | residual_wide_scores | maxsim_scores over decompress() | ratio | rerank over all ids | scan / rerank | "
         "same bits as the rerank | max abs diff to the decompressed scan | compressed row bytes read per s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for bits in BITS:
        for shape, leg in res[f"bits{bits}"]["scan"].items():
            rr = "residual_rerank_all_ids" in leg
            L.append(f"| {bits} | {shape} | {_fmt(leg['residual_scan'])} | {_fmt(leg['bf16_decompressed_scan'])} | {leg['residual_over_bf16']:.2f} | "
                     f"{_fmt(leg['residual_rerank_all_ids']) if rr else '-'} | {leg['scan_over_rerank_all_ids']:.2f} | " if rr else
                     f"| {bits} | {shape} | {_fmt(leg['residual_scan'])} | {_fmt(leg['bf16_decompressed_scan'])} | {leg['residual_over_bf16']:.2f} | - | - | ")
            L[-1] += (f"{leg['bit_identical_to_rerank_all_ids'] if rr else '-'} | {leg['max_abs_diff_to_bf16_scan']:.2e} | "
                      f"{leg['row_bytes_per_s'] / 1e9:.1f} GB |")
    return "\n".join(L) + "\n"


def main_wide_scan(args, amd, dev):
    """--dim 320 --legs scan: the full scan of the compressed shard alone; the section is APPENDED to --summary"""
    from tools.bench_rerank import make_shard_dim

    docs = args.docs if args.docs != 125_000 else 50_000
    t0 = time.perf_counter()
    res = {"tool": "bench_residual", "dim": 320, "legs": "scan", "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len,
           "n_centroids": K, "steps": args.steps, "warmup": args.warmup}
    corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
    index = amd.CentroidWideIndex.build(corpus, n_centroids=K)
    res["corpus_bytes"] = corpus.nbytes
    shards = {bits: amd.ResidualWideCorpus.build(corpus, index=index, bits=bits) for bits in BITS}
    del corpus
    torch.cuda.empty_cache()
    for bits, rc in shards.items():
        dec = rc.decompress() if args.scan_ref else None
        res[f"bits{bits}"] = {"nbytes": rc.nbytes, "scan": scan_leg(amd, rc, dec, args.q_len, dev, args.steps, args.warmup)}
        del dec
        torch.cuda.empty_cache()
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary and args.scan_ref:
        fresh = not os.path.exists(args.summary)
        with open(args.summary, "a") as f:
            f.write(("# The residual-compressed shard at width 320 (ColQwen3)\n" if fresh else "") + wide_scan_summary(res))
    print(line)


def wide_rows_summary(res) -> str:
    """the section `--dim 320 --legs align,gather` appends to profiles/residual_wide_summary.md"""
    L = ["", "## Rows out of the compressed shard: residual_wide_align / residual_wide_gather_pages", "",
         f"`tools/bench_residual.py --dim 320 --legs {res['legs']} --steps {res['steps']} --warmup {res['warmup']}` on {res['docs']} pages x "
         f"{res['doc_len']} rows x 320 bf16 ({res['corpus_bytes'] / 1e9:.1f} GB), K = {res['n_centroids']}; the three variants of a row alternate "
         "step by step inside one timing loop; median (min - max) in ms.  The detour reads the ids back, decodes the listed pages with "
         "`rc.decompress(ids)` and calls `align` / `gather_pages` over that copy.", "",
         "| bits | leg | fused | decompress-then-call | over a resident decompress() | fused / detour | fused / resident | same bits |",
         "|---|---|---|---|---|---|---|---|"]
    for bits in BITS:
        b = res[f"bits{bits}"]
        for name, leg in b.get("align", {}).items():
            L.append(f"| {bits} | align {ALIGN_SHAPE[0]} x {res['q_len']} x k = {ALIGN_SHAPE[1]}, {name} | {_fmt(leg['residual_align'])} | "
                     f"{_fmt(leg['decompress_then_align'])} | {_fmt(leg['align_resident_bf16'])} | {leg['residual_over_decompress']:.3f} | "
                     f"{leg['residual_over_resident_bf16']:.2f} | {leg['bit_identical']} |")
        if "gather" in b:
            leg = b["gather"]
            L.append(f"| {bits} | gather ids [{GATHER_SHAPE[0]}, {GATHER_SHAPE[1]}] | {_fmt(leg['residual_gather_pages'])} | "
                     f"{_fmt(leg['decompress_then_gather'])} | {_fmt(leg['gather_pages_resident_bf16'])} | {leg['residual_over_decompress']:.3f} | "
                     f"{leg['residual_over_bf16']:.2f} | {leg['bit_identical']} |")
    return "\n".join(L) + "\n"


def main_wide_rows(args, amd, dev, legs):
    """--dim 320 --legs align,gather: the two row-returning calls over the wide compressed shard; the section is APPENDED to --summary"""
    from tools.bench_rerank import make_shard_dim

    docs = args.docs if args.docs != 125_000 else 50_000
    t0 = time.perf_counter()
    res = {"tool": "bench_residual", "dim": 320, "legs": ",".join(sorted(legs)), "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len,
           "n_centroids": K, "steps": args.steps, "warmup": args.warmup}
    corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
    index = amd.CentroidWideIndex.build(corpus, n_centroids=K)
    res["corpus_bytes"] = corpus.nbytes
    shards = {bits: amd.ResidualWideCorpus.build(corpus, index=index, bits=bits) for bits in BITS}
    del corpus
    torch.cuda.empty_cache()
    for bits, rc in shards.items():
        dec = rc.decompress()
        leg = {"nbytes": rc.nbytes}
        if "align" in legs:
            leg["align"] = align_leg(amd, rc, dec, args.q_len, dev, args.steps, args.warmup)
        if "gather" in legs:
            leg["gather"] = gather_leg(amd, rc, dec, dev, args.steps, args.warmup, detour=True)
        res[f"bits{bits}"] = leg
        del dec
        torch.cuda.empty_cache()
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        fresh = not os.path.exists(args.summary)
        with open(args.summary, "a") as f:
            f.write(("# The residual-compressed shard at width 320 (ColQwen3)\n" if fresh else "") + wide_rows_summary(res))
    print(line)


def main_wide(args):
    """--dim 320: see the module docstring"""
    import colpali_amd as amd
    from tools.bench_fp4 import wide_planted
    from tools.bench_rerank import make_queries_dim, make_shard_dim

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    if set(args.legs.split(",")) == {"scan"}:
        return main_wide_scan(args, amd, dev)
    if set(args.legs.split(",")) <= {"align", "gather"}:
        return main_wide_rows(args, amd, dev, set(args.legs.split(",")))
    docs = args.docs if args.docs != 125_000 else 50_000
    t0 = time.perf_counter()
    res = {"tool": "bench_residual", "dim": 320, "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len, "n_centroids": K,
           "steps": args.steps, "warmup": args.warmup}
    corpus = make_shard_dim(docs, args.doc_len, 320, dev, seed=1234)
    index = amd.CentroidWideIndex.build(corpus, n_centroids=K)
    res["corpus_bytes"], res["index_bytes"] = corpus.nbytes, index.nbytes
    res["centroid_encode"] = timed_alternating({"encode": lambda: amd.CentroidWideIndex.build(corpus, centroids=index.centroids)}, 3, 1)["encode"]
    pq1000 = amd.pack_queries(make_queries_dim(1000, args.q_len, 320, dev, seed=99), dev, compact=False)
    for bits in BITS:
        rc = amd.ResidualWideCorpus.build(corpus, index=index, bits=bits)
        leg = {"nbytes": rc.nbytes, "bytes_per_row": rc.nbytes / max(int(rc.codes.shape[0]), 1)}
        leg["encode"] = timed_alternating({"encode": lambda: amd.ResidualWideCorpus.build(corpus, index=index, bits=bits, cutoffs=rc.cutoffs,
                                                                                         weights=rc.weights)}, 3, 1)["encode"]
        leg["decompress"] = timed_alternating({"decompress": lambda: rc.decompress()}, 3, 1)["decompress"]
        dec = rc.decompress()
        leg["rerank"] = {}
        for n_q, m in SHAPES:
            pq = amd.pack_queries(make_queries_dim(n_q, args.q_len, 320, dev, seed=99), dev, compact=False)
            by_list = {}
            for name, cand in (("uniform", uniform_candidates(n_q, len(rc), m, dev, 7)),
                               ("clustered", clustered_candidates(n_q, len(rc), m, dev, 8, pool=max(200, 2 * m)))):
                a = torch.empty((n_q, m), dtype=torch.float32, device=dev)
                b = torch.empty((n_q, m), dtype=torch.float32, device=dev)
                t = timed_alternating({"residual": lambda: amd.residual_wide_rerank_scores(pq, rc, cand, out=a),
                                       "bf16_decompressed": lambda: amd.retrieval.rerank_scores(pq, dec, cand, out=b)}, args.steps, args.warmup)
                t["residual_over_bf16"] = t["residual"]["median_ms"] / t["bf16_decompressed"]["median_ms"]
                t["bit_identical"] = bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                by_list[name] = t
            leg["rerank"][f"{n_q}x{m}"] = by_list
        del dec
        torch.cuda.empty_cache()
        r_c, r_b = amd.ShardedRetriever(rc), amd.ShardedRetriever(corpus)
        leg["two_stage"] = {str(m): timed_alternating({"residual": lambda: r_c.search(pq1000, k=10, prefilter=rc.index, n_candidates=m),
                                                       "bf16": lambda: r_b.search(pq1000, k=10, prefilter=index, n_candidates=m)},
                                                      args.steps, args.warmup) for m in MS}
        res[f"bits{bits}"] = leg
        del rc, r_c, r_b
        torch.cuda.empty_cache()
    del corpus, index
    torch.cuda.empty_cache()
    full, _, pq = wide_planted(amd, dev, args.recall_docs)
    exact_s, exact_i = amd.ShardedRetriever(full).search(pq, k=10)
    index = amd.CentroidWideIndex.build(full, n_centroids=K)
    rec = {"docs": args.recall_docs, "queries": len(pq), "k": 10, "n_centroids": K}
    for bits in BITS:
        rc = amd.ResidualWideCorpus.build(full, index=index, bits=bits)
        r = amd.ShardedRetriever(rc)
        leg = {}
        for m in MS:
            _, i = r.search(pq, k=10, prefilter=rc.index, n_candidates=m)
            leg[str(m)] = sum(len(set(a) & set(b)) for a, b in zip(exact_i.tolist(), i.tolist())) / (len(pq) * 10)
        approx = amd.rerank(pq, rc, exact_i)                        # the codec's own error: the exact top-k rescored from the compressed rows
        ok = exact_i >= 0
        leg["mean_abs_score_error"] = float((approx - exact_s)[ok].abs().mean())
        leg["mean_exact_score"] = float(exact_s[ok].mean())
        rec[f"bits{bits}"] = leg
        del rc, r
    res["recall"] = rec
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(wide_summary(res))
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128, choices=(128, 320), help="320: the ResidualWideCorpus on the 320-wide shard")
    ap.add_argument("--summary", default=None, help="--dim 320: write the markdown summary here")
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="build,rerank,two_stage,recall")
    ap.add_argument("--recall-docs", type=int, default=10_000)
    ap.add_argument("--scan-ref", type=int, default=1, help="0: the scan leg times residual_scores alone")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_residual.py needs an MI355X (there is no CPU fallback)")
    if args.dim == 320:
        return main_wide(args)
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_residual", "docs": args.docs, "doc_len": args.doc_len, "q_len": args.q_len, "n_centroids": K}
    if legs & {"build", "rerank", "two_stage", "scan", "align", "gather"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        index = amd.CentroidIndex.build(corpus, n_centroids=K)
        res["corpus_bytes"] = corpus.nbytes
        res["index_bytes"] = index.nbytes
        for bits in BITS:
            rc = amd.ResidualCorpus.build(corpus, index=index, bits=bits)
            leg = {"nbytes": rc.nbytes, "bytes_per_row": rc.nbytes / max(int(rc.codes.shape[0]), 1)}
            if "build" in legs:
                g = torch.Generator().manual_seed(0)
                pick = torch.randperm(int(corpus.blob.shape[0]), generator=g)[:1 << 18].to(dev)
                sample = (corpus.blob[pick].float() - index.centroids[(index.codes.view(torch.int16)[pick].to(torch.int64) & 0xFFFF)].float())
                leg["build"] = {"train_codec": timed(lambda: amd.train_residual_codec(sample, bits), 2, 1),
                                "encode": timed(lambda: amd.ResidualCorpus.build(corpus, index=index, bits=bits, cutoffs=rc.cutoffs,
                                                                                 weights=rc.weights), 2, 1)}
                del sample, pick
            if "rerank" in legs:
                dec = rc.decompress()
                leg["decompress"] = timed(lambda: rc.decompress(), 2, 1)
                leg["rerank"] = {f"{n_q}x{m}": rerank_leg(amd, rc, dec, n_q, m, args.q_len, dev, args.steps, args.warmup) for n_q, m in SHAPES}
                del dec
            if "two_stage" in legs:
                pq = amd.pack_queries(make_queries(1000, args.q_len, dev, seed=99), dev, compact=False)
                r_c, r_b = amd.ShardedRetriever(rc), amd.ShardedRetriever(corpus)
                leg["two_stage"] = {str(m): {"residual": timed(lambda: r_c.search(pq, k=10, prefilter=rc.index, n_candidates=m), args.steps,
                                                               args.warmup),
                                             "bf16": timed(lambda: r_b.search(pq, k=10, prefilter=index, n_candidates=m), args.steps,
                                                           args.warmup)} for m in MS}
            if "scan" in legs:
                dec = rc.decompress() if args.scan_ref else None
                leg["scan"] = scan_leg(amd, rc, dec, args.q_len, dev, args.steps, args.warmup)
                del dec
            if legs & {"align", "gather"}:
                dec = rc.decompress()
                if "align" in legs:
                    leg["align"] = align_leg(amd, rc, dec, args.q_len, dev, args.steps, args.warmup)
                if "gather" in legs:
                    leg["gather"] = gather_leg(amd, rc, dec, dev, args.steps, args.warmup)
                del dec
            res[f"bits{bits}"] = leg
            del rc
            torch.cuda.empty_cache()
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
