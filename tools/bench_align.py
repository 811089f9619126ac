"""Token-to-patch alignment of search hits (msim_align_candidates, kernel K1a); one JSON object on stdout (not part of bench.py).

    python tools/bench_align.py [--out FILE] [--steps 20 --warmup 5] [--dim 128 --docs 2000 --doc-len 1024 --nq 4 --q-len 32 --hits 10]

Legs, each timed with device events after a warm-up:
  * align(queries, corpus, ids) and align(..., maps=True) for nq queries x `hits` listed pages of doc-len rows;
  * the loop a caller writes without the entry: per hit, slice the page out of the blob (offsets read back to the host once, outside
    the timed region) and call similarity_matrix(query, page), then max / argmax over the rows in torch.
The maps of both are compared (largest |difference|) before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--docs", type=int, default=2000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=4)
    ap.add_argument("--q-len", type=int, default=32)
    ap.add_argument("--hits", type=int, default=10)
    a = ap.parse_args()

    import colpali_amd as amd

    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)

    def unit(*shape):
        return torch.nn.functional.normalize(torch.randn(*shape, generator=g, device=dev), dim=-1).to(torch.bfloat16)

    corpus = amd.pack_passages(unit(a.docs, a.doc_len, a.dim), dev, batch_size=None)
    box = unit(a.nq, a.q_len, a.dim)
    pq = amd.pack_queries(box, dev, layout="flat")
    ids = torch.rand((a.nq, a.docs), generator=g, device=dev).topk(a.hits, dim=1).indices.to(torch.int64)
    ids_host = ids.cpu().tolist()
    off = corpus.offsets.cpu().tolist()

    def loop():
        out = []
        for q in range(a.nq):
            for c in ids_host[q]:
                sim = amd.similarity_matrix(box[q], corpus.blob[off[c]:off[c + 1]])
                out.append((sim, sim.max(dim=1)))
        return out

    al = amd.align(pq, corpus, ids, maps=True)
    ref = loop()
    diff = max(float((al.sims[q, j, :, :a.doc_len] - ref[q * a.hits + j][0].float()).abs().max())
               for q in range(a.nq) for j in range(a.hits))
    rows_equal = all(bool((al.best_row[q, j].long() == ref[q * a.hits + j][1].indices).all()) for q in range(a.nq) for j in range(a.hits))
    res = {
        "shape": {"dim": a.dim, "docs": a.docs, "doc_len": a.doc_len, "nq": a.nq, "q_len": a.q_len, "hits": a.hits},
        "max_abs_diff_vs_similarity_matrix": diff,
        "best_rows_equal_torch_argmax": rows_equal,
        "align": timed(lambda: amd.align(pq, corpus, ids), a.steps, a.warmup),
        "align_maps": timed(lambda: amd.align(pq, corpus, ids, maps=True), a.steps, a.warmup),
        "similarity_matrix_loop": timed(loop, a.steps, a.warmup),
        "page_bytes_listed": a.nq * a.hits * a.doc_len * a.dim * 2,
        "map_bytes_written": a.nq * a.hits * a.q_len * a.doc_len * 4,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
