"""Hard-negative mining and the page gather (msim_mine_*, msim_gather_pages; colpali_amd.mine_hard_negatives / gather_pages) on
the headline shard; one JSON object on stdout (not part of bench.py).

    python tools/bench_mine.py [--out FILE] [--steps 10 --warmup 3] [--docs 125000 --doc-len 1024] [--queries 1000 --q-len 32]
                               [--n-neg 8 --max-ratio 0.95]

Each leg is timed with device events after a warm-up (median of --steps):
  * scan_topk: maxsim_scores + topk(n_neg), the bare search that mining wraps.
  * mine: mine_hard_negatives (the same scan, msim_mine_bounds, msim_mine_mask, topk).  `added_share` = (mine - scan_topk) / scan_topk:
    what the bounds and mask launches add.
  * mask_only: msim_mine_bounds + msim_mine_mask on a resident [n_q, n] matrix, beside its byte bound (the matrix read once,
    n_q x n x 4 B, at 8 TB/s; few columns are stored).
  * gather: gather_pages of the mined [n_q, n_neg] ids into a preallocated box; bound = (the box written + the same rows read + 12 B
    per slot) / 8 TB/s.
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
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--n-neg", type=int, default=8)
    ap.add_argument("--max-ratio", type=float, default=0.95)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mine.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd
    from colpali_amd.mine import mine_bounds, mine_mask, positives_csr

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    t0 = time.perf_counter()
    n_q, n, k = args.queries, args.docs, args.n_neg
    corpus = make_shard(n, args.doc_len, dev, seed=1234)
    pq = amd.pack_queries(make_queries(n_q, args.q_len, dev, seed=99), dev, compact=False)
    pos = torch.randint(0, n, (n_q,), generator=torch.Generator().manual_seed(7)).to(dev)
    res = {"tool": "bench_mine", "docs": n, "doc_len": args.doc_len, "queries": n_q, "q_len": args.q_len, "n_neg": k,
           "max_ratio": args.max_ratio, "hbm_peak_GBps": HBM_PEAK_GBS}
    res["scan_topk"] = timed(lambda: amd.topk(amd.maxsim_scores(pq, corpus), k), args.steps, args.warmup)
    res["mine"] = timed(lambda: amd.mine_hard_negatives(pq, corpus, pos, k, max_ratio=args.max_ratio), args.steps, args.warmup)
    res["mine"]["added_share"] = (res["mine"]["median_ms"] - res["scan_topk"]["median_ms"]) / res["scan_topk"]["median_ms"]

    scores = amd.maxsim_scores(pq, corpus)
    csr = positives_csr(pos, n_q, dev)
    work = torch.empty_like(scores)

    def mask_only():
        mine_mask(work, csr, 0, mine_bounds(work, csr, 0), args.max_ratio)

    def fresh_then_mask():              # the mask is in place: every timed call starts from the scan's matrix
        work.copy_(scores)
        mask_only()

    copy = timed(lambda: work.copy_(scores), args.steps, args.warmup)
    both = timed(fresh_then_mask, args.steps, args.warmup)
    res["mask_only"] = {"median_ms": both["median_ms"] - copy["median_ms"], "with_refill_ms": both["median_ms"],
                        "refill_ms": copy["median_ms"], "bound_ms": n_q * n * 4 / (HBM_PEAK_GBS * 1e9) * 1e3}
    del work, scores

    _, neg_ids = amd.mine_hard_negatives(pq, corpus, pos, k, max_ratio=args.max_ratio)
    row_bytes = corpus.blob.shape[1] * corpus.blob.element_size()
    box = torch.empty((n_q, k, args.doc_len, corpus.blob.shape[1]), dtype=corpus.blob.dtype, device=dev)
    g = timed(lambda: amd.gather_pages(corpus, neg_ids, out=box), args.steps, args.warmup)
    slots = n_q * k
    g["bytes"] = 2 * slots * args.doc_len * row_bytes + 12 * slots
    g["bound_ms"] = g["bytes"] / (HBM_PEAK_GBS * 1e9) * 1e3
    g["share_of_bound"] = g["bound_ms"] / g["median_ms"]
    g["GBps"] = g["bytes"] / g["median_ms"] / 1e6
    res["gather"] = g
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
