"""Shared helpers of the embedding-head GPU tests (tests/test_gpu_head.py, tests/test_gpu_head_edges.py): random cases, the
element-wise comparison of a head output with oracle/head_oracle.py (literal tier and float64 truth tier) and the float64 autograd
truth of the three gradients with their error bounds.  Independent of colpali_amd.

Tolerances: the kernel reproduces the reference's rounding chain in the model dtype (Linear output, norm, quotient each
rounded once), so outputs are compared element-wise with the literal tier (the reference's own lines evaluated on CPU in
that dtype): >= 99.5 % of the elements bit-equal, at most 1e-4 of them more than one ulp of the 16-bit dtype apart, none
more than two (2e-6 absolute floor for outputs that cancelled to almost nothing) -- the fp32 accumulation order of the
K = hidden-size dot product differs from the CPU GEMM's, which occasionally flips a rounding;
against the float64 truth tier: 2^-6 relative for bf16, 2^-9 for fp16, on |value| >= 1e-3.
"""
import numpy as np
import torch

from oracle import head_oracle as ho


def _bf16(bits: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def grid_distance(got: torch.Tensor, want: torch.Tensor, atol: float = 2e-6):
    """Per-element distance in ulps of the 16-bit dtype (0 where |diff| <= atol), and the bit-equal fraction.
    The absolute floor covers outputs that are tiny because the K-long dot product cancelled: there the fp32
    accumulation-order error (~1e-7 of the sum of |products|, ~4e-7 after the normalisation) spans several grid steps of
    a number that small -- for the CPU GEMM too."""
    g, w = got.cpu().float(), want.cpu().float()
    mant = 7 if got.dtype == torch.bfloat16 else 10
    ulp = torch.exp2(torch.floor(torch.log2(w.abs().clamp_min(1e-30))) - mant)
    diff = (g - w).abs()
    d = torch.where(diff <= atol, torch.zeros_like(diff), diff / ulp)
    return d, float((g == w).float().mean())


def assert_same_rounding_chain(got, want):
    """One rounding where torch has one: >= 99.5 % of the elements bit-equal, at most 1e-4 of them more than one ulp
    apart and none more than two (a flipped rounding of the Linear output moves the quotient by up to one ulp before ITS
    rounding).  The reference's own CPU output sits exactly this far from the exactly-accumulated chain
    (measured: 99.99 % equal, 1 element of 527 360 at two ulps)."""
    d, same = grid_distance(got, want)
    assert same >= 0.995, same
    assert float((d > 1).float().mean()) <= 1e-4 and float(d.max()) <= 2.0, (float((d > 1).float().mean()), float(d.max()))


def check(got, hidden, weight, bias, mask, extra=None):
    assert_same_rounding_chain(got, ho.head_literal(hidden, weight, bias, mask, extra))
    truth = ho.head_truth(hidden, weight, bias, mask, extra)
    big = truth.abs() >= 1e-3
    rel = 2.0**-6 if got.dtype == torch.bfloat16 else 2.0**-9
    assert torch.all(((got.cpu().double() - truth).abs() <= rel * truth.abs())[big])
    keep = (mask != 0) if extra is None else ((mask != 0) & (extra.reshape(mask.shape) != 0))
    assert torch.count_nonzero(got.cpu()[~keep]) == 0                      # masked positions are exactly zero


def _case(seed, B, S, H, dtype, pad="right"):
    g = torch.Generator().manual_seed(seed)
    hidden = (torch.randn(B, S, H, generator=g) * 2.0).to(dtype)
    weight = (torch.randn(128, H, generator=g) / H**0.5).to(dtype)
    bias = (torch.randn(128, generator=g) * 0.1).to(dtype)
    mask = torch.ones(B, S, dtype=torch.long)
    for b in range(1, B):
        n = int(torch.randint(1, S, (1,), generator=g))
        if pad == "left":
            mask[b, : S - n] = 0          # ColQwen2 pads on the left (modeling_colqwen2.py:36)
        else:
            mask[b, n:] = 0
    return hidden, weight, bias, mask


# ---------------------------------------------------------------------------------------------------------------------------
# The head inside a training graph (modeling_colpali.py:65-78 is part of what the reference trainers back-propagate through).

def _truth_grads(hidden, weight, bias, mask, G, extra=None):
    """float64 autograd through oracle/head_oracle.py's restatement of the reference lines: the three gradients, and for each
    the sum of the ABSOLUTE terms of the product that forms it (|dproj| |W|, |dproj|^T |X|, sum |dproj|): dproj is rounded
    to the 16-bit model dtype before the products, so the error of a gradient scales with that sum, not with the (possibly
    cancelled) value."""
    h = hidden.double().requires_grad_(True)
    w = weight.double().requires_grad_(True)
    b = None if bias is None else bias.double().requires_grad_(True)
    cap = {}
    orig = torch.nn.functional.linear

    def linear_keep(x, ww, bb=None):
        y = orig(x, ww, bb)
        y.retain_grad()
        cap["proj"] = y
        return y

    ho.F.linear = linear_keep
    try:
        y = ho.head_literal(h, w, b, mask, extra)
    finally:
        ho.F.linear = orig
    (y * G.double()).sum().backward()
    dproj = cap["proj"].grad.abs()
    flat = dproj.reshape(-1, dproj.shape[-1])
    bounds = ((dproj @ w.detach().abs()), flat.t() @ h.detach().abs().reshape(-1, h.shape[-1]), flat.sum(0))
    return (h.grad, w.grad, None if b is None else b.grad), bounds


def _grad_close(got, want, bound, dtype):
    """|error| <= ulp-of-the-result + one 16-bit rounding per term of the product (worst case, see _truth_grads)."""
    rel = 2.0**-8 if dtype == torch.bfloat16 else 2.0**-11
    err = (got.cpu().double() - want).abs()
    return bool(torch.all(err <= rel * want.abs() + rel * bound + 1e-30))
