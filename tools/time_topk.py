"""Time the selection kernels on one GPU.  No pass/fail: it prints numbers.

    tools/time_topk.py [--rounds 15] [--skip-deep]

First the many-query scan shape at small k (msim_topk_f32's streaming filter).  Then the deep shapes (msim_topk_deep_f32, 1024 < k <=
8192): for each, `topk` at that k, `torch.topk(sorted=True)` at that k on the same matrix (which has neither the project's tie
order nor explicit ids), and `topk` at k = 1024 (msim_topk_f32, the neighbouring point) -- the variants ALTERNATE inside one loop, and
every figure is the median of the rounds with its min-max.  The bound printed per shape is (digit passes + 1) x n_q x n x 4 B at
8 TB/s: four reads for the key digits and one for the gather."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
import torch  # noqa: E402

import colpali_amd as amd  # noqa: E402


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(variants, rounds):
    """{name: [ms per round]} with the variants taking turns inside one loop (after one untimed turn each)"""
    times = {name: [] for name in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_time(fn))
    return times


def show(label, ms):
    return f"{label} {statistics.median(ms):8.3f} ms ({min(ms):.3f}-{max(ms):.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--skip-deep", action="store_true")
    args = ap.parse_args()

    s = torch.randn(1000, 125000, device="cuda") * 0.1 + 9.3
    for k in (10, 100):
        ms = alternate({"topk": lambda: amd.topk(s, k)}, args.rounds)["topk"]
        print(f"topk k={k} 1000x125000: {show('', ms)} = {s.numel() * 4 / statistics.median(ms) / 1e6:.0f} GB/s of score reads")
    if args.skip_deep:
        return

    g = torch.Generator(device="cuda").manual_seed(0)
    shapes = [(4, 125000, 4096, False), (1000, 125000, 1025, False), (1000, 125000, 4096, False), (1000, 125000, 8192, False),
              (1000, 4096, 2048, True)]
    print("| shape | k | ids | topk (deep) | torch.topk(sorted) | topk k=1024 | bound |")
    print("|---|---|---|---|---|---|---|")
    for n_q, n, k, explicit in shapes:
        scores = s[:n_q, :n] if n == s.shape[1] else s[:n_q, :n].contiguous()
        ids = None
        if explicit:
            ids = torch.stack([torch.randperm(n, device="cuda", generator=g) for _ in range(n_q)]) + (1 << 33)
        variants = {
            "deep": lambda: amd.topk(scores, k, 0, ids),
            "torch": lambda: torch.topk(scores, k, dim=1, sorted=True),
            "k1024": lambda: amd.topk(scores, 1024, 0, ids),
        }
        t = alternate(variants, args.rounds)
        bound = 5 * n_q * n * 4 / 8e12 * 1e3
        print(f"| {n_q} x {n} | {k} | {'explicit' if explicit else 'implicit'} | {show('', t['deep'])} | {show('', t['torch'])} | "
              f"{show('', t['k1024'])} | {bound:.3f} ms |")


if __name__ == "__main__":
    main()
