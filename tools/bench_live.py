"""The live corpus (colpali_amd.LiveCorpus, msim_live_*) on the headline shard; one JSON object on stdout (not part of bench.py).

    python tools/bench_live.py [--out FILE] [--docs 125000 --doc-len 1024] [--steps 5] [--bounce-mb 256] [--legs compact,search,add]

Legs, each timed with device events (compact: one call per fresh set of deletions; the others after a warm-up):
  * stream: a device-to-device copy of 4 GiB, the run's own ceiling for a read + write stream (bytes read + written / time).
  * compact: compact() after deleting 1 %, 10 % and 50 % of the pages uniformly at random.  Bound = the bytes the bounce scheme
    must move (2 reads + 2 writes of every row that changes place; rows below the first deleted page do not move) / 8 TB/s.  Beside
    it: pack_passages of the surviving pages from host memory (the only alternative without a live corpus), on a sample of
    --repack-docs pages and scaled by bytes.  The result is checked: offsets and a sample of pages against the survivors.
  * search: LiveCorpus.search with nothing deleted against ShardedRetriever.search on the same rows, alternating, at 4 and 1000
    queries of 32 tokens; the mask's estimate is n_q x n x 8 B / 8 TB/s plus one launch.
  * add: add() of 1000 pages of --doc-len rows from a host list against the H2D floor of their bytes at 56 GB/s.
search and add report the median over --steps and, as *_spread_ms, max - min of those identical calls.

    python tools/bench_live.py --fp4 [--dim 320] [--out FILE] [--summary FILE] [--docs N] [--steps 5] [--bounce-mb 256]

The live FP4 index (LiveCorpus.fp4_index, msim_f4_live_compact) instead of the legs above; every comparison alternates its two
variants in one loop and reports the median with min and max:
  * compact() with the index on after deleting 1 %, 10 % and 50 % of the pages, beside compact() with no index followed by
    Fp4Index.build(live.view()) (Fp4WideIndex at --dim 320): what keeping the same state took before the index was kept in step.
    The first trial is checked (the index against a build over the view), not timed.
  * add() of 1000 host pages with the index on and off.
  * search(prefilter=live.fp4_index(), n_candidates=100) with nothing deleted against ShardedRetriever.search over the same rows
    and a built index, at 4 and 1000 queries of 32 tokens; the results are compared first.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_legs.common import HBM_PEAK_GBS, make_queries, make_shard  # noqa: E402
from tools.bench_rerank import timed  # noqa: E402

H2D_GBS = 56.0


def once_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def stream_leg(dev):
    n = 4 << 30
    src, dst = torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    t = timed(lambda: dst.copy_(src), 5, 2)
    t["GBps_read_plus_write"] = 2 * n / t["median_ms"] / 1e6
    return t


def compact_leg(amd, corpus, frac, bounce_bytes, repack_docs, seed):
    n, doc_len = len(corpus), int(corpus.lengths[0])
    row_bytes = corpus.blob.shape[1] * corpus.blob.element_size()
    live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=bounce_bytes)
    g = torch.Generator().manual_seed(seed)
    gone = torch.randperm(n, generator=g)[:max(1, int(n * frac))].sort().values
    alive = np.ones(n, dtype=bool)
    alive[gone.numpy()] = False
    sample = torch.from_numpy(np.flatnonzero(alive)[:: max(1, n // 64)])
    keep = [corpus.blob[int(s) * doc_len:(int(s) + 1) * doc_len].clone() for s in sample]
    live.delete(gone.tolist())
    ms = once_ms(live.compact)
    live.check()
    new_off = np.concatenate([[0], np.cumsum(np.where(alive, doc_len, 0))])
    assert np.array_equal(live.view().offsets.cpu().numpy(), new_off) and live.rows_used == int(new_off[-1])
    for s, page in zip(sample.tolist(), keep):
        assert torch.equal(live.blob[new_off[s]:new_off[s + 1]], page), f"page {s} differs after compaction"
    moved_rows = int(alive[int(gone[0]):].sum()) * doc_len
    bound_ms = 4.0 * moved_rows * row_bytes / (HBM_PEAK_GBS * 1e9) * 1e3
    out = {"deleted": int(gone.numel()), "first_deleted": int(gone[0]), "moved_rows": moved_rows, "compact_ms": ms,
           "bound_ms": bound_ms, "share_of_bound": bound_ms / ms, "moved_GBps": 4.0 * moved_rows * row_bytes / ms / 1e6}
    del live
    torch.cuda.empty_cache()
    # the alternative at the parent commit: pack the survivors again from host memory (a sample, scaled by bytes)
    k = min(repack_docs, int(alive.sum()))
    host = [torch.empty((doc_len, corpus.blob.shape[1]), dtype=corpus.blob.dtype).normal_() for _ in range(k)]
    amd.pack_passages(host, corpus.device, batch_size=None)
    t0 = time.perf_counter()
    amd.pack_passages(host, corpus.device, batch_size=None)
    torch.cuda.synchronize()
    sample_ms = (time.perf_counter() - t0) * 1e3
    out["repack_sample_docs"], out["repack_sample_ms"] = k, sample_ms
    out["repack_scaled_ms"] = sample_ms * int(alive.sum()) / k
    return out


def search_leg(amd, corpus, n_q, q_len, dev, steps):
    live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=1 << 20)
    ref = amd.ShardedRetriever(corpus)
    pq = amd.pack_queries(make_queries(n_q, q_len, dev, seed=99), dev, compact=False)
    a, b = live.search(pq, 10), ref.search(pq, 10)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    lv, rf = [], []
    for _ in range(steps):                               # alternating, same run
        lv.append(once_ms(lambda: live.search(pq, 10)))
        rf.append(once_ms(lambda: ref.search(pq, 10)))
    scores = torch.zeros((n_q, len(corpus)), dtype=torch.float32, device=dev)
    mask = timed(lambda: amd.live.mask_scores(scores, live.alive[:len(live)]), 10, 3)
    lv.sort(), rf.sort()
    est = n_q * len(corpus) * 8 / (HBM_PEAK_GBS * 1e9) * 1e3
    return {"live_ms": lv[len(lv) // 2], "static_ms": rf[len(rf) // 2], "difference_ms": lv[len(lv) // 2] - rf[len(rf) // 2],
            "live_spread_ms": lv[-1] - lv[0], "static_spread_ms": rf[-1] - rf[0], "mask_alone_ms": mask["median_ms"],
            "mask_estimate_ms": est}


def add_leg(amd, dev, n_pages, doc_len, steps):
    pages = [torch.empty((doc_len, 128), dtype=torch.bfloat16).normal_() for _ in range(n_pages)]
    nbytes = n_pages * doc_len * 256
    live = amd.LiveCorpus((steps + 2) * n_pages * doc_len, (steps + 2) * n_pages, dev)
    ms = []
    for i in range(steps + 2):
        t0 = time.perf_counter()
        live.add(pages)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[2:])
    floor = nbytes / (H2D_GBS * 1e9) * 1e3
    return {"pages": n_pages, "bytes": nbytes, "add_ms": ms[len(ms) // 2], "add_spread_ms": ms[-1] - ms[0], "h2d_floor_ms": floor,
            "share_of_floor": floor / ms[len(ms) // 2]}


def _stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def fp4_compact_leg(amd, corpus, cls, frac, bounce_bytes, steps, seed):
    """compact() with the FP4 index on, beside what the parent commit needs for the same state: compact() with no index, then a
    build over the view.  Alternating in one loop; every trial starts from a fresh copy of the shard with the same deletions."""
    n = len(corpus)
    g = torch.Generator().manual_seed(seed)
    gone = torch.randperm(n, generator=g)[:max(1, int(n * frac))].sort().values.tolist()

    def fresh(index):
        live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=bounce_bytes)
        if index:
            live.fp4_index()
        live.delete(gone)
        return live

    kept, rebuilt = [], []
    for s in range(steps + 1):                           # trial 0 warms both variants up and is checked, not timed
        live = fresh(True)
        ms = once_ms(live.compact)
        live.check()
        if s == 0:
            idx, want = live.fp4_index(), cls.build(live.view())
            r = live.rows_used
            assert torch.equal(idx.codes[:r], want.codes[:r]) and torch.equal(idx.scales[:r], want.scales[:r]), "index differs from a build"
            del idx, want
        else:
            kept.append(ms)
        del live
        live = fresh(False)
        ms = once_ms(lambda: (live.compact(), cls.build(live.view())))
        if s:
            rebuilt.append(ms)
        del live
    return {"deleted": len(gone), "first_deleted": gone[0], "kept_in_step": _stats(kept), "compact_then_build": _stats(rebuilt)}


def fp4_add_leg(amd, dev, dim, n_pages, doc_len, steps):
    """add() of host pages with the FP4 index on and off, alternating"""
    pages = [torch.empty((doc_len, dim), dtype=torch.bfloat16).normal_() for _ in range(n_pages)]
    lives = {"index_on": amd.LiveCorpus((steps + 2) * n_pages * doc_len, (steps + 2) * n_pages, dev, width=dim),
             "index_off": amd.LiveCorpus((steps + 2) * n_pages * doc_len, (steps + 2) * n_pages, dev, width=dim)}
    lives["index_on"].fp4_index()
    ms = {name: [] for name in lives}
    for _ in range(steps + 2):
        for name, live in lives.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            live.add(pages)
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {name: _stats(v[2:]) for name, v in ms.items()}
    out["pages"], out["bytes"] = n_pages, n_pages * doc_len * dim * 2
    return out


def fp4_search_leg(amd, corpus, cls, pq, steps):
    """search(prefilter=live.fp4_index()) with nothing deleted against the frozen two-stage search on the same rows, alternating"""
    from tools.bench_binary import alternating

    live = amd.LiveCorpus.from_packed(corpus, 0, 0, bounce_bytes=1 << 20)
    live.fp4_index()
    ref, ref_idx = amd.ShardedRetriever(corpus), cls.build(corpus)
    a = live.search(pq, 10, prefilter=live.fp4_index(), n_candidates=100)
    b = ref.search(pq, 10, prefilter=ref_idx, n_candidates=100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    return alternating({"live": lambda: live.search(pq, 10, prefilter=live.fp4_index(), n_candidates=100),
                        "frozen": lambda: ref.search(pq, 10, prefilter=ref_idx, n_candidates=100)}, steps, 1)


def _mmm(t):
    return f"{t['median_ms']:.2f} ms ({t['min_ms']:.2f}–{t['max_ms']:.2f})"


def fp4_summary(res):
    """the markdown section of profiles/live_summary.md for one --fp4 run"""
    L = [f"`tools/bench_live.py --fp4 --dim {res['dim']}` on {res['docs']} pages × {res['doc_len']} rows × {res['dim']} bf16 "
         f"({res['shard_bytes'] / 2**30:.1f} GiB, FP4 index {res['index_bytes'] / 2**30:.1f} GiB), bounce {res['bounce_mb']} MiB; "
         f"medians of {res['steps']} alternating trials with min–max.", "",
         "| deleted | `compact()` with the index kept in step | `compact()` then a build over the view |", "|---|---|---|"]
    for f, r in res["compact"].items():
        L.append(f"| {f} ({r['deleted']}) | {_mmm(r['kept_in_step'])} | {_mmm(r['compact_then_build'])} |")
    a = res["add"]
    L += ["", f"`add` of {a['pages']} host pages ({a['bytes'] / 1e6:.0f} MB): {_mmm(a['index_on'])} with the index on, "
          f"{_mmm(a['index_off'])} with it off.", "",
          "| queries | `live.search(prefilter=live.fp4_index(), n_candidates=100)` | frozen `ShardedRetriever` + built index |", "|---|---|---|"]
    for n, r in res["search"].items():
        L.append(f"| {n} × {res['q_len']} | {_mmm(r['live'])} | {_mmm(r['frozen'])} |")
    return "\n".join(L) + "\n"


def main_fp4(args, amd, dev):
    """--fp4: the live FP4 index on the headline shard (--dim 320: 50 000 pages by default, the shard every other width-320
    measurement uses -- tools/bench_fp4.py --dim 320 -- so that the shard, its live copy and both indexes fit beside each other)"""
    from tools.bench_rerank import make_queries_dim, make_shard_dim

    dim = args.dim
    docs = args.docs if args.docs is not None else (125_000 if dim == 128 else 50_000)
    cls = amd.Fp4WideIndex if dim == 320 else amd.Fp4Index
    mb = int(args.bounce_mb.split(",")[0])
    t0 = time.perf_counter()
    res = {"tool": "bench_live", "leg": "fp4", "dim": dim, "docs": docs, "doc_len": args.doc_len, "q_len": args.q_len, "steps": args.steps,
           "bounce_mb": mb}
    res["add"] = fp4_add_leg(amd, dev, dim, 1000, args.doc_len, args.steps)
    torch.cuda.empty_cache()
    corpus = make_shard_dim(docs, args.doc_len, dim, dev, seed=1234)
    res["shard_bytes"], res["index_bytes"] = corpus.nbytes, docs * args.doc_len * (dim // 2 + 1)
    res["search"] = {}
    for n in (4, 1000):
        pq = amd.pack_queries(make_queries_dim(n, args.q_len, dim, dev, seed=99), dev, compact=False)
        res["search"][str(n)] = fp4_search_leg(amd, corpus, cls, pq, args.steps if n <= 8 else 3)
        torch.cuda.empty_cache()
    res["compact"] = {f"{int(f * 100)} %": fp4_compact_leg(amd, corpus, cls, f, mb << 20, args.steps, 7) for f in (0.01, 0.10, 0.50)}
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.summary:
        with open(args.summary, "w") as f:
            f.write(fp4_summary(res))
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fp4", action="store_true", help="the live FP4 index legs (compact, add, search) instead of --legs")
    ap.add_argument("--dim", type=int, default=128, choices=(128, 320), help="with --fp4: the shard's width")
    ap.add_argument("--summary", default=None, help="with --fp4: write the markdown section for profiles/live_summary.md here")
    ap.add_argument("--docs", type=int, default=None, help="125 000; with --fp4 --dim 320: 50 000")
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--bounce-mb", default="256")
    ap.add_argument("--repack-docs", type=int, default=2000)
    ap.add_argument("--legs", default="stream,compact,search,add")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    if args.fp4:
        return main_fp4(args, amd, dev)
    args.docs = 125_000 if args.docs is None else args.docs
    legs = set(args.legs.split(","))
    t0 = time.perf_counter()
    res = {"tool": "bench_live", "docs": args.docs, "doc_len": args.doc_len, "hbm_peak_GBps": HBM_PEAK_GBS}
    if "stream" in legs:
        res["stream"] = stream_leg(dev)
        torch.cuda.empty_cache()
    if "add" in legs:
        res["add"] = add_leg(amd, dev, 1000, args.doc_len, args.steps)
        torch.cuda.empty_cache()
    if legs & {"compact", "search"}:
        corpus = make_shard(args.docs, args.doc_len, dev, seed=1234)
        if "search" in legs:
            res["search"] = {str(n): search_leg(amd, corpus, n, args.q_len, dev, args.steps if n <= 8 else 3) for n in (4, 1000)}
            torch.cuda.empty_cache()
        if "compact" in legs:
            res["compact"] = {}
            for mb in [int(x) for x in args.bounce_mb.split(",")]:
                res["compact"][f"bounce_{mb}MiB"] = {f"{int(f * 100)}%": compact_leg(amd, corpus, f, mb << 20, args.repack_docs, 7)
                                                    for f in (0.01, 0.10, 0.50)}
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
