"""Filtered search (colpali_amd.PageFilter, `ShardedRetriever.search(filter=)`) on the headline shard: the mask route and the list
route beside the unfiltered search of the same run; one JSON object on stdout (not part of bench.py).

    python tools/bench_filter.py [--out FILE] [--steps 5 --warmup 2] [--docs 125000 --doc-len 1024] [--queries 4,1000 --q-len 32]
                                 [--k 10] [--selectivity 0.001,0.01,0.05,0.2,0.5] [--tenants 100]

For each batch size every leg is timed with device events after a warm-up (median of --steps):
  * unfiltered: `search(k)`, the scan and the top-k.
  * per selectivity s, a SHARED filter that admits round(s x docs) pages (a fixed random subset), prepared beforehand:
      mask   `search(filter=, filter_route="mask")`: the scan, msim_filter_mask, the top-k;
      list   `search(filter=, filter_route="list")`: msim_filter_list, the rerank of the list, the top-k;
    each as a fraction of the unfiltered time, and the list route also as a fraction of the HBM bound of the allowed pages' bytes
    (every allowed page read once at 8 TB/s).
  * labels: a label filter of --tenants equal tenants (page c belongs to tenant c % tenants, query q to tenant q % tenants), the same
    three figures.
`crossover`: per batch size the largest measured selectivity at which the list route is faster than the mask route, and the smallest
of those over the batch sizes, capped at 1/5 -- what colpali_amd/filter.py ships as LIST_ROUTE_MAX_FRACTION.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=125_000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--queries", default="4,1000")
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--selectivity", default="0.001,0.01,0.05,0.2,0.5")
    ap.add_argument("--tenants", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_filter.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    t0 = time.perf_counter()
    n, k = args.docs, args.k
    corpus = make_shard(n, args.doc_len, dev, seed=1234)
    retriever = amd.ShardedRetriever(corpus)
    page_bytes = args.doc_len * corpus.blob.shape[1] * corpus.blob.element_size()
    order = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    res = {"tool": "bench_filter", "docs": n, "doc_len": args.doc_len, "q_len": args.q_len, "k": k, "tenants": args.tenants,
           "hbm_peak_GBps": HBM_PEAK_GBS, "batches": {}}
    fractions = [float(s) for s in args.selectivity.split(",")]
    per_batch_cross = []
    for n_q in (int(x) for x in args.queries.split(",")):
        pq = amd.pack_queries(make_queries(n_q, args.q_len, dev, seed=99), dev, compact=False)
        out = {"unfiltered": timed(lambda: retriever.search(pq, k), args.steps, args.warmup), "shared": [], "labels": None}
        base_ms = out["unfiltered"]["median_ms"]

        def legs(flt, allowed_pages):
            flt.prepare()
            leg = {"max_allowed": flt.max_allowed}
            for route in ("mask", "list"):
                t = timed(lambda: retriever.search(pq, k, filter=flt, filter_route=route), args.steps, args.warmup)
                t["of_unfiltered"] = t["median_ms"] / base_ms
                leg[route] = t
            bound_ms = allowed_pages * page_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
            leg["list"]["bound_ms"] = bound_ms
            leg["list"]["share_of_bound"] = bound_ms / leg["list"]["median_ms"]
            leg["list_faster"] = leg["list"]["median_ms"] < leg["mask"]["median_ms"]
            return leg

        cross = 0.0
        for s in fractions:
            m = max(1, round(s * n))
            mask = torch.zeros(n, dtype=torch.bool)
            mask[order[:m]] = True
            leg = legs(amd.PageFilter.from_mask(mask.to(dev)), m)
            leg["selectivity"] = s
            out["shared"].append(leg)
            if leg["list_faster"]:
                cross = max(cross, s)
        page_labels = (torch.arange(n, dtype=torch.int32) % args.tenants).to(dev)
        query_labels = (torch.arange(n_q, dtype=torch.int32) % args.tenants).to(dev)
        distinct = min(n_q, args.tenants) * ((n + args.tenants - 1) // args.tenants)          # pages some query may return
        out["labels"] = legs(amd.PageFilter.from_labels(page_labels, query_labels), min(distinct, n))
        out["list_faster_up_to"] = cross
        per_batch_cross.append(cross)
        res["batches"][str(n_q)] = out
    res["crossover"] = {"per_batch": per_batch_cross, "list_route_max_fraction": min(min(per_batch_cross), 0.2),
                        "shipped": amd.filter.LIST_ROUTE_MAX_FRACTION}
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
