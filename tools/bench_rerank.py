"""Candidate reranking (msim_fwd_candidates, kernel K1c; --dim 320: msim_fwd_candidates_wide, kernel K1cP) on the headline shard; one
JSON object on stdout (not part of bench.py).

    python tools/bench_rerank.py [--out FILE] [--steps 10 --warmup 3] [--dim 128 --docs 125000 --doc-len 1024 --nq 1000 --q-len 32 --m 100]

--dim 320 (ColQwen3) uses a shard of the same bytes by default (50 000 documents x 1024 rows x 640 B = 30.5 GiB), has no pair-kernel
leg (msim_pairs_argmax is width 128 only) and adds the largest |rerank - full scan| (a scan of one query length and at most four
32-token tiles runs K1sP, whose token sum is a butterfly: equal to fp32 summation order, not bit for bit).

Legs, each timed with device events after a warm-up:
  * distributions U (every query draws m distinct documents uniformly) and C (clusters of 10 queries share a pool of 200 documents,
    each query draws m of them): rerank call time; its share of the bound max(distinct documents' bytes / 8 TB/s, entries x
    2 Lq rows 128 / 2.5 PFLOP/s); the bytes the plan requests (work items of <= 8 units split documents listed by many queries); the
    same list through msim_pairs_argmax (no arg-max output); the full maxsim_scores followed by a gather.  Outputs are checked against
    the full-scan gather (every entry, bit for bit).
  * two-stage: ShardedRetriever.search(prefilter=coarse shard of 343 rows per document, n_candidates=m) against the exact full search.
  * recall@10 of the two-stage search against the exact one on a planted 10k-document set really pooled by
    HierarchicalTokenPooler(pool_factor=3) (reported, not gated).
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


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    torch.cuda.synchronize()
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in evs)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def uniform_candidates(n_q, n_docs, m, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.rand((n_q, n_docs), generator=g, device=dev).topk(m, dim=1).indices.to(torch.int64)


def clustered_candidates(n_q, n_docs, m, dev, seed, cluster=10, pool=200):
    g = torch.Generator(device=dev).manual_seed(seed)
    n_cl = (n_q + cluster - 1) // cluster
    pools = torch.rand((n_cl, n_docs), generator=g, device=dev).topk(pool, dim=1).indices               # distinct per cluster
    pick = torch.rand((n_cl * cluster, pool), generator=g, device=dev).topk(m, dim=1).indices           # m of the pool per query
    rows = pools.repeat_interleave(cluster, dim=0)
    return torch.gather(rows, 1, pick)[:n_q].to(torch.int64)


def make_shard_dim(n_docs, doc_len, dim, device, seed):
    """bench_legs.common.make_shard at another width: unit-norm bf16 rows generated on the device in chunks."""
    from colpali_amd.corpus import PackedCorpus

    g = torch.Generator(device=device).manual_seed(seed)
    blob = torch.empty((n_docs * doc_len, dim), dtype=torch.bfloat16, device=device)
    chunk = 256
    for d0 in range(0, n_docs, chunk):
        n = min(chunk, n_docs - d0)
        x = torch.randn((n * doc_len, dim), generator=g, device=device, dtype=torch.float32)
        blob[d0 * doc_len:(d0 + n) * doc_len] = torch.nn.functional.normalize(x, dim=-1).to(torch.bfloat16)
    lengths = torch.full((n_docs,), doc_len, dtype=torch.int64)
    offsets = (torch.arange(n_docs + 1, dtype=torch.int64) * doc_len).to(torch.int32).to(device)
    return PackedCorpus(blob=blob, offsets=offsets, clamp0=None, lengths=lengths)


def make_queries_dim(n_q, q_len, dim, device, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(n_q, q_len, dim, generator=g), dim=-1).to(torch.bfloat16).to(device)


def plan_numbers(cand, n_docs, doc_len, q_lens, dim=128):
    """Distinct documents, and the work items msim_fwd_candidates makes (classes = 16-token units of the query)."""
    units = torch.tensor([(ln + 15) // 16 for ln in q_lens], device=cand.device)
    per = torch.tensor([0, 8, 4, 2, 2, 1, 1, 1, 1], device=cand.device)
    cls = units.unsqueeze(1).expand_as(cand)
    counts = torch.zeros((n_docs, 9), dtype=torch.int64, device=cand.device)
    counts.index_put_((cand.reshape(-1), cls.reshape(-1)), torch.ones(cand.numel(), dtype=torch.int64, device=cand.device), accumulate=True)
    items = ((counts[:, 1:] + per[1:] - 1) // per[1:]).sum(dim=1)
    distinct = int((counts.sum(dim=1) > 0).sum())
    doc_bytes = doc_len * dim * 2
    return {"distinct_docs": distinct, "work_items": int(items.sum()), "ideal_bytes": distinct * doc_bytes,
            "plan_bytes": int(items.sum()) * doc_bytes}


def distribution_leg(amd, pq, qbox, corpus, cand, q_len, doc_len, steps, warmup, dim=128):
    n_q, m = cand.shape
    out = plan_numbers(cand, len(corpus), doc_len, pq.lengths.tolist(), dim)
    entries = n_q * m
    flops = entries * 2.0 * q_len * doc_len * dim
    bound_s = max(out["ideal_bytes"] / (HBM_PEAK_GBS * 1e9), flops / (MFMA_PEAK_TFLOPS * 1e12))
    out["bound_ms"] = bound_s * 1e3
    out["bound_by"] = "HBM" if out["ideal_bytes"] / (HBM_PEAK_GBS * 1e9) >= flops / (MFMA_PEAK_TFLOPS * 1e12) else "MFMA"
    scores = torch.empty((n_q, m), dtype=torch.float32, device=cand.device)
    out["rerank"] = timed(lambda: amd.rerank(pq, corpus, cand, out=scores), steps, warmup)
    out["rerank"]["share_of_bound"] = out["bound_ms"] / out["rerank"]["median_ms"]
    out["rerank"]["plan_TBps"] = out["plan_bytes"] / (out["rerank"]["median_ms"] * 1e-3) / 1e12

    # the training pair kernel on the same list (queries as a padded box, one document read per entry, no arg-max output)
    L = amd._lib.lib()
    pair_scores = None
    if dim == 128:
        pair_scores = pairs_leg(amd, L, out, qbox, corpus, cand, q_len, doc_len, steps)

    full = torch.empty((n_q, len(corpus)), dtype=torch.float32, device=cand.device)

    def full_then_gather():
        amd.maxsim_scores(pq, corpus, out=full)
        return torch.gather(full, 1, cand)

    out["full_scan_gather"] = timed(full_then_gather, max(3, steps // 2), 1)
    out["full_scan_gather"]["rerank_speedup"] = out["full_scan_gather"]["median_ms"] / out["rerank"]["median_ms"]
    want = full_then_gather()
    got = amd.rerank(pq, corpus, cand)
    torch.cuda.synchronize()
    out["bit_identical_to_full_scan"] = bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
    if pair_scores is not None:
        out["pairs_argmax_max_abs_diff"] = float((pair_scores.view(n_q, m) - want).abs().max())
    else:
        out["max_abs_diff_to_full_scan"] = float((got - want).abs().max())
    return out


def pairs_leg(amd, L, out, qbox, corpus, cand, q_len, doc_len, steps):
    n_q, m = cand.shape
    entries = n_q * m
    pairs = torch.stack([torch.arange(n_q, device=cand.device).unsqueeze(1).expand_as(cand).reshape(-1), cand.reshape(-1)], 1)
    pairs = pairs.to(torch.int32).contiguous()
    pair_scores = torch.empty((entries,), dtype=torch.float32, device=cand.device)

    def pairs_call():
        rc = L.msim_pairs_argmax(0, amd._lib.ptr(qbox), n_q, q_len, amd._lib.ptr(corpus.blob), amd._lib.ptr(corpus.offsets), None,
                                 len(corpus), 128, doc_len, amd._lib.ptr(pairs), entries, amd._lib.ptr(pair_scores), None,
                                 amd._lib.current_stream_handle(cand.device))
        amd._lib.check(rc, "msim_pairs_argmax")

    out["pairs_argmax"] = timed(pairs_call, max(3, steps // 2), 1)
    out["pairs_argmax"]["rerank_speedup"] = out["pairs_argmax"]["median_ms"] / out["rerank"]["median_ms"]
    return pair_scores


def planted_recall(amd, dev, n_docs=10_000, doc_len=1024, n_q=100, q_len=32, m=100, k=10, seed=5, dim=128):
    """Pages made of 48 topic directions each (rows = topic + noise), queries drawn from one target page's topics: pooling by
    HierarchicalTokenPooler(pool_factor=3) keeps the structure the exact score sees, as it does on real pages."""
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
    pq = amd.pack_queries(torch.nn.functional.normalize(q, dim=-1).to(torch.bfloat16), dev, compact=False)
    r = amd.ShardedRetriever(full)
    _, exact = r.search(pq, k=k)
    _, two = r.search(pq, k=k, prefilter=pooled, n_candidates=m)
    hits = sum(len(set(a) & set(b)) for a, b in zip(exact.tolist(), two.tolist()))
    return {"docs": n_docs, "pooled_rows_per_doc": float(pooled.blob.shape[0]) / n_docs, "queries": n_q, "k": k, "n_candidates": m,
            "recall_at_10": hits / (n_q * k)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=128, choices=(128, 320))
    ap.add_argument("--docs", type=int, default=None, help="default: 125 000 at width 128, 50 000 at width 320 (the same bytes)")
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--coarse-len", type=int, default=343)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--m", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="U,C,two_stage,recall")
    ap.add_argument("--recall-docs", type=int, default=10_000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rerank.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    legs = set(args.legs.split(","))
    wide = args.dim != 128
    if args.docs is None:
        args.docs = 50_000 if wide else 125_000
    t0 = time.perf_counter()
    if wide:
        corpus = make_shard_dim(args.docs, args.doc_len, args.dim, dev, seed=1234)
        qbox = make_queries_dim(args.nq, args.q_len, args.dim, dev, seed=99)
    else:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        qbox = make_queries(args.nq, args.q_len, dev, seed=99)
    pq = amd.pack_queries(qbox, dev, compact=False)
    res = {"tool": "bench_rerank", "docs": args.docs, "doc_len": args.doc_len, "n_queries": args.nq, "q_len": args.q_len, "m": args.m,
           "hbm_peak_GBps": HBM_PEAK_GBS, "mfma_peak_TFLOPs": MFMA_PEAK_TFLOPS}
    if wide:
        res["dim"] = args.dim
    kw = {"dim": args.dim} if wide else {}
    if "U" in legs:
        res["U"] = distribution_leg(amd, pq, qbox, corpus, uniform_candidates(args.nq, args.docs, args.m, dev, 1), args.q_len, args.doc_len,
                                    args.steps, args.warmup, **kw)
    if "C" in legs:
        res["C"] = distribution_leg(amd, pq, qbox, corpus, clustered_candidates(args.nq, args.docs, args.m, dev, 2), args.q_len,
                                    args.doc_len, args.steps, args.warmup, **kw)
    if "two_stage" in legs:
        coarse = (make_shard_dim(args.docs, args.coarse_len, args.dim, dev, seed=4321) if wide
                  else make_shard(args.docs, args.coarse_len, dev, seed=4321))
        r = amd.ShardedRetriever(corpus)
        res["two_stage"] = {
            "coarse_rows_per_doc": args.coarse_len,
            "exact_search": timed(lambda: r.search(pq, k=10), max(3, args.steps // 2), 1),
            "two_stage_search": timed(lambda: r.search(pq, k=10, prefilter=coarse, n_candidates=args.m), args.steps, args.warmup),
        }
        res["two_stage"]["speedup"] = res["two_stage"]["exact_search"]["median_ms"] / res["two_stage"]["two_stage_search"]["median_ms"]
        del coarse
    del corpus
    torch.cuda.empty_cache()
    if "recall" in legs:
        res["recall"] = planted_recall(amd, dev, n_docs=args.recall_docs, **kw)
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
