"""The embedding head at width 320 (msim_embed_head_wide, colpali_amd.embedding_head / CorpusWriter(width=320)) beside the reference's
lines run by torch on the same GPU; one JSON object on stdout, optionally a markdown summary (not part of bench.py).

    python tools/bench_head_wide.py [--out FILE] [--md FILE] [--steps 10 --warmup 3] [--pages 1000 --seq 779] [--hidden 2048,2560,4096]

Per hidden size, bf16, pages x seq positions (left padded: the first tenth of every other page is masked), two legs; the variants of
a leg ALTERNATE call by call inside one timed loop (device events), every figure is the median with its range:
  * head:   colpali_amd.embedding_head(hidden, W, b, mask) beside the reference's four lines
                proj = F.linear(hidden, W, b); proj = proj / proj.norm(dim=-1, keepdim=True); proj = proj * mask.unsqueeze(-1)
  * writer: CorpusWriter(width=320).append(hidden, W, b, mask) beside those lines plus the boolean-mask copy of the kept rows into a
            packed buffer (what stays on the GPU of the reference's road; its unbind / .cpu() / pad_sequence / H2D are not timed).
Bound of either: max(bytes / 8 TB/s, 2 M H 320 / 2.5 PFLOP/s), bytes = hidden states + weight read once, output written once.
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

from bench_legs.common import HBM_PEAK_GBS, MFMA_PEAK_TFLOPS  # noqa: E402
from tools.bench_binary import alternating  # noqa: E402

WIDTH = 320


def reference_lines(hidden, weight, bias, mask):
    proj = torch.nn.functional.linear(hidden, weight, bias)
    proj = proj / proj.norm(dim=-1, keepdim=True)
    return proj * mask.unsqueeze(-1)


def bound_ms(M, H, rows_out):
    nbytes = (M * H + WIDTH * H + rows_out * WIDTH) * 2
    return {"memory_ms": nbytes / (HBM_PEAK_GBS * 1e9) * 1e3, "matrix_ms": 2.0 * M * H * WIDTH / (MFMA_PEAK_TFLOPS * 1e12) * 1e3}


def fmt(leg):
    return f"{leg['median_ms']:.3f} ({leg['min_ms']:.3f} – {leg['max_ms']:.3f})"


def one_size(amd, pages, seq, H, dev, steps, warmup):
    g = torch.Generator(device=dev).manual_seed(H)
    hidden = torch.empty((pages, seq, H), dtype=torch.bfloat16, device=dev)
    for p0 in range(0, pages, 100):                                            # filled in pieces: no fp32 copy of the whole batch
        n = min(100, pages - p0)
        hidden[p0:p0 + n] = (torch.randn((n, seq, H), generator=g, device=dev) * 2.0).to(torch.bfloat16)
    weight = (torch.randn((WIDTH, H), generator=g, device=dev) / H**0.5).to(torch.bfloat16)
    bias = (torch.randn((WIDTH,), generator=g, device=dev) * 0.1).to(torch.bfloat16)
    mask = torch.ones((pages, seq), dtype=torch.long, device=dev)
    mask[1::2, : seq // 10] = 0
    M, kept = pages * seq, int(mask.sum())
    packed = torch.empty((kept, WIDTH), dtype=torch.bfloat16, device=dev)
    keep = mask != 0

    def writer():
        w = amd.CorpusWriter(M, dev, width=WIDTH)
        w.append(hidden, weight, bias, mask)
        return w

    def reference_road():
        packed.copy_(reference_lines(hidden, weight, bias, mask)[keep])

    with torch.no_grad():
        same = float((amd.embedding_head(hidden[:8], weight, bias, mask[:8]) == reference_lines(hidden[:8], weight, bias, mask[:8]))
                     .float().mean())
        head = alternating({"fused": lambda: amd.embedding_head(hidden, weight, bias, mask),
                            "torch": lambda: reference_lines(hidden, weight, bias, mask)}, steps, warmup)
        wr = alternating({"fused": writer, "torch": reference_road}, steps, warmup)
    res = {"H": H, "M": M, "kept_rows": kept, "bit_equal_share_8_pages": same, "head": head, "writer": wr,
           "head_bound": bound_ms(M, H, M), "writer_bound": bound_ms(M, H, kept)}
    for leg, bound in (("head", "head_bound"), ("writer", "writer_bound")):
        res[leg]["speedup"] = res[leg]["torch"]["median_ms"] / res[leg]["fused"]["median_ms"]
        res[leg]["ranges_apart"] = res[leg]["fused"]["max_ms"] < res[leg]["torch"]["min_ms"]
        res[leg]["share_of_bound"] = max(res[bound].values()) / res[leg]["fused"]["median_ms"]
    return res


def markdown(res):
    lines = ["# Embedding head at width 320: measured on one MI355X", "",
             f"`tools/bench_head_wide.py --steps {res['steps']} --warmup {res['warmup']}`: {res['pages']} pages × {res['seq']} positions, bf16, "
             "every other page left padded by a tenth.  The two variants of a leg alternate call by call in one timed loop; median ms, with "
             "the range in brackets.  Bound: max(bytes / 8 TB/s, 2·M·H·320 / 2.5 PFLOP/s).", ""]
    for leg, title in (("head", "`embedding_head` beside the reference's four lines run by torch"),
                       ("writer", "`CorpusWriter(width=320).append` beside those lines + the boolean-mask copy into a packed buffer")):
        lines += [f"## {title}", "", "| H | fused | torch | torch / fused | bound (memory, matrix) | share of the bound |", "|---|---|---|---|---|---|"]
        for s in res["sizes"]:
            b = s[leg + "_bound"]
            lines.append(f"| {s['H']} | {fmt(s[leg]['fused'])} | {fmt(s[leg]['torch'])} | {s[leg]['speedup']:.2f} × "
                         f"({'ranges apart' if s[leg]['ranges_apart'] else 'ranges overlap'}) | {b['memory_ms']:.3f}, {b['matrix_ms']:.3f} | "
                         f"{s[leg]['share_of_bound']:.2f} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pages", type=int, default=1000)
    ap.add_argument("--seq", type=int, default=779)
    ap.add_argument("--hidden", default="2048,2560,4096")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_head_wide.py needs an MI355X (there is no CPU fallback)")
    import colpali_amd as amd

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    amd._lib.lib()
    t0 = time.perf_counter()
    res = {"tool": "bench_head_wide", "pages": args.pages, "seq": args.seq, "steps": args.steps, "warmup": args.warmup,
           "hbm_peak_GBps": HBM_PEAK_GBS, "mfma_peak_TFLOPs": MFMA_PEAK_TFLOPS, "sizes": []}
    for H in (int(h) for h in args.hidden.split(",")):
        res["sizes"].append(one_size(amd, args.pages, args.seq, H, dev, args.steps, args.warmup))
        torch.cuda.empty_cache()
    res["wall_s"] = time.perf_counter() - t0
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(res) + "\n")
    print(line)


if __name__ == "__main__":
    main()
