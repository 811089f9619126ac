"""Document-level search (colpali_amd.PageGroups, `ShardedRetriever.search(group_by=)`) on the headline shard: `search(group_by=)`
beside the page-level `search` of the same run, the two group kernels alone, and the torch composition of the group reduction on
the same scores; one JSON object on stdout (not part of bench.py).

    python tools/bench_group.py [--out FILE] [--steps 20 --warmup 3] [--search-steps 5 --search-warmup 2]
                                [--docs 125000 --doc-len 1024] [--queries 4,1000 --q-len 32] [--k 10] [--select-m 1000,4096]

Group shapes over the --docs pages of the shard:
  contiguous10   documents of 10 consecutive pages;
  ragged1-200    documents of U{1..200} consecutive pages (a fixed seed);
  single         one page per document.
For each batch size and shape, timed with device events after a warm-up (median of the steps):
  * `search(k)` and `search(k, group_by=)`: the scan plus the top-k, and the scan, `group_reduce`, the top-k over the documents and
    the gathers;
  * `group_reduce` alone on the scan's score matrix, beside its traffic bound at 8 TB/s -- 4 B per (query, page) read plus 12 B per
    (query, document) written -- and the fraction of that bound it reaches;
  * the torch composition on the same scores: `scatter_reduce_("amax")` for the document scores, an equality mask and a second
    `scatter_reduce_("amin")` over the page indices for the winning page; `torch.topk` over the documents is timed separately;
  * `group_select` alone on candidate rows of --select-m entries (random scores, the pages' documents), k = --k.
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
from tools.bench_rerank import timed  # noqa: E402


def group_labels(shape: str, n: int) -> torch.Tensor:
    """int64 [n]: the document of every page"""
    if shape == "contiguous10":
        return torch.arange(n, dtype=torch.int64) // 10
    if shape == "single":
        return torch.arange(n, dtype=torch.int64)
    if shape == "ragged1-200":
        g = torch.Generator().manual_seed(11)
        sizes = torch.randint(1, 201, (n,), generator=g)                 # more than enough documents; cut at n pages
        return torch.repeat_interleave(torch.arange(n, dtype=torch.int64), sizes)[:n].contiguous()
    raise ValueError(shape)


def torch_reduce(scores: torch.Tensor, idx: torch.Tensor, cols: torch.Tensor, n_groups: int):
    """the composition a caller without the kernel would write: document scores by amax, the winning page by an equality mask"""
    n_q, n = scores.shape
    doc_s = torch.full((n_q, n_groups), float("-inf"), dtype=torch.float32, device=scores.device)
    doc_s.scatter_reduce_(1, idx, scores, "amax", include_self=True)
    hit = scores == doc_s.gather(1, idx)
    page = torch.where(hit, cols, torch.full_like(cols, n))
    doc_p = torch.full((n_q, n_groups), n, dtype=torch.int64, device=scores.device)
    doc_p.scatter_reduce_(1, idx, page, "amin", include_self=True)
    return doc_s, doc_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--queries", default="4,1000")
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--shapes", default="contiguous10,ragged1-200,single")
    ap.add_argument("--select-m", default="1000,4096")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--search-steps", type=int, default=5)
    ap.add_argument("--search-warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_group.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    t0 = time.perf_counter()
    n, k = args.docs, args.k
    corpus = make_shard(n, args.doc_len, dev, seed=1234)
    retriever = amd.ShardedRetriever(corpus)
    shapes = args.shapes.split(",")
    groups = {s: amd.PageGroups.from_labels(group_labels(s, n).to(dev)).prepare() for s in shapes}
    res = {"tool": "bench_group", "docs": n, "doc_len": args.doc_len, "q_len": args.q_len, "k": k, "hbm_peak_GBps": HBM_PEAK_GBS,
           "shapes": {s: {"n_groups": g.n_groups, "max_group": g.max_group} for s, g in groups.items()}, "batches": {}}
    for n_q in (int(x) for x in args.queries.split(",")):
        pq = amd.pack_queries(make_queries(n_q, args.q_len, dev, seed=99), dev, compact=False)
        out = {"search": timed(lambda: retriever.search(pq, k), args.search_steps, args.search_warmup), "shapes": {}}
        scores = amd.maxsim_scores(pq, corpus)
        cols = torch.arange(n, dtype=torch.int64, device=dev)[None, :].expand(n_q, n)
        for name, g in groups.items():
            leg = {"search_group_by": timed(lambda: retriever.search(pq, k, group_by=g), args.search_steps, args.search_warmup)}
            leg["search_group_by"]["of_search"] = leg["search_group_by"]["median_ms"] / out["search"]["median_ms"]
            t = timed(lambda: amd.group_reduce(scores, g), args.steps, args.warmup)
            bytes_moved = 4.0 * n_q * n + 12.0 * n_q * g.n_groups
            t["bound_ms"] = bytes_moved / (HBM_PEAK_GBS * 1e9) * 1e3
            t["share_of_bound"] = t["bound_ms"] / t["median_ms"]
            t["GBps"] = bytes_moved / (t["median_ms"] * 1e-3) / 1e9
            leg["group_reduce"] = t
            idx = g.page_group.long()[None, :].expand(n_q, n)
            leg["torch_reduce"] = timed(lambda: torch_reduce(scores, idx, cols, g.n_groups), max(args.steps // 4, 3), 1)
            leg["torch_reduce"]["over_group_reduce"] = leg["torch_reduce"]["median_ms"] / t["median_ms"]
            doc_s, doc_p = amd.group_reduce(scores, g)
            want_s, want_p = torch_reduce(scores, idx, cols, g.n_groups)
            leg["equals_torch"] = bool(torch.equal(doc_s, want_s) and torch.equal(doc_p, want_p))      # random scores: no -inf, no zeros
            kk = min(k, g.n_groups)
            leg["torch_topk"] = timed(lambda: torch.topk(doc_s, kk, dim=1), args.steps, args.warmup)
            leg["topk"] = timed(lambda: amd.topk(doc_s, k), args.steps, args.warmup)
            del idx, want_s, want_p, doc_s, doc_p
            out["shapes"][name] = leg
        sel = {}
        gen = torch.Generator(device=dev).manual_seed(5)
        g10 = groups[shapes[0]]
        for m in (int(x) for x in args.select_m.split(",")):
            pages = torch.randint(0, n, (n_q, m), generator=gen, device=dev)
            s = torch.rand((n_q, m), generator=gen, device=dev)
            gids = g10.doc_ids(pages)
            sel[str(m)] = timed(lambda: amd.group_select(s, gids, pages, k), args.steps, args.warmup)
        out["group_select"] = {"groups": shapes[0], "by_m": sel}
        del scores, cols
        res["batches"][str(n_q)] = out
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
