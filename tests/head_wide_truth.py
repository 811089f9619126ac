"""Shared helpers of the 320-wide embedding-head tests (tests/test_head_wide_host.py, tests/test_gpu_head_wide.py): the cases, the
exactly-accumulated chain, the three literal norm candidates and the comparison rule.  Independent of colpali_amd.

Why width 320 has a rule of its own.  The literal tier of tests/head_truth.py (>= 99.5 % bit-equal, <= 1e-4 of the elements more
than one ulp apart) is a per-element share.  When the rounded norm `n` of a row lands one grid step away, up to 320 elements of
that row move at once; in fp16 the reference's own CPU chain, compared with the same chain accumulated exactly, is at 4e-5 .. 6e-4
by that measure -- on either side of the 1e-4 cap by the seed.  So a kept row is compared with the BEST of three literal candidates:
the reference's lines with the norm left alone, moved one grid step down and one up (fewest elements more than one ulp apart, then
most equal, ties to the unmoved norm), and the shares are calibrated by the reference itself on the same input:

  1. hard bound: masked positions exactly zero; per kept row against its best candidate no element more than two ulps apart
     (grid_distance's 2e-6 absolute floor);
  2. truth tier: 2^-6 (bf16) / 2^-9 (fp16) relative against the float64 evaluation on |value| >= 1e-3;
  3. shares: with u_ref / g_ref / r_ref = the unequal share, the more-than-one-ulp share and the share of rows with a moved norm of
     the EXACTLY-ACCUMULATED chain (float64 Linear output, rounded at the same three places) against the candidates, the output
     under test stays within 3 u_ref + 5 / n_elements, 3 g_ref + 5 / n_elements and 3 r_ref + 2 / n_rows.  (The distance of the
     kernel from the literal chain is at most its own distance from the exact chain plus the reference's: 2x if its fp32
     accumulation is no worse than the CPU GEMM's; the third factor covers counting noise on a few dozen elements, the additive
     floors keep a 12 800-element case from hinging on one element);
  4. bf16 outputs of 100 000 or more elements also pass tests/head_truth.py::assert_same_rounding_chain unchanged.

tests/test_head_wide_host.py asserts, without a GPU, that rule 3 is meaningful for every case used on the GPU: the exact chain
meets rule 1, u_ref <= 5e-3 and r_ref <= 2 %.
"""
import functools

import torch

from oracle import head_oracle as ho
from tests.head_truth import assert_same_rounding_chain, grid_distance

WIDTH = 320
ROW_TILE = 128          # rows per tile of embed_head_wide_kernel

# (name, seed, B, S, H, dtype, padding): the forward cases of tests/test_gpu_head_wide.py
FORWARD_CASES = (
    ("a_fewer_rows_than_a_wave", 11, 1, 17, 128, torch.bfloat16, "right"),
    ("b_one_chunk", 12, 3, 50, 64, torch.bfloat16, "right"),
    ("c_two_chunks_weight_ring_depth", 13, 2, 60, 128, torch.bfloat16, "right"),
    ("c_three_chunks_hidden_ring_depth", 14, 2, 60, 192, torch.bfloat16, "right"),
    ("c_four_chunks_one_past_the_rings", 15, 2, 60, 256, torch.bfloat16, "right"),
    ("d_qwen3vl_left_padded", 16, 2, 300, 2048, torch.bfloat16, "left"),
    ("e_forty_chunks_left_padded", 17, 2, 70, 2560, torch.bfloat16, "left"),
    ("f_largest_hidden_size", 18, 1, 40, 4096, torch.bfloat16, "right"),
    ("g_fp16_model_width", 19, 3, 200, 2048, torch.float16, "right"),
    ("h_fp16_largest_hidden_size", 20, 1, 40, 4096, torch.float16, "right"),
    ("rows_one_below_the_tile", 21, 1, ROW_TILE - 1, 64, torch.bfloat16, "right"),
    ("rows_at_the_tile", 22, 1, ROW_TILE, 64, torch.bfloat16, "right"),
    ("rows_one_above_the_tile", 23, 1, ROW_TILE + 1, 64, torch.bfloat16, "right"),
    ("more_tiles_than_cus_partial_last", 24, 5, (300 * ROW_TILE + 5) // 5, 64, torch.bfloat16, "right"),   # 38 405 rows = 300 tiles + 5 rows
)
assert 5 * ((300 * ROW_TILE + 5) // 5) == 300 * ROW_TILE + 5


def case(seed, B, S, H, dtype, pad="right", bias=True):
    """tests/head_truth.py::_case with a [320, H] weight and a [320] bias."""
    g = torch.Generator().manual_seed(seed)
    hidden = (torch.randn(B, S, H, generator=g) * 2.0).to(dtype)
    weight = (torch.randn(WIDTH, H, generator=g) / H**0.5).to(dtype)
    b = (torch.randn(WIDTH, generator=g) * 0.1).to(dtype)
    mask = torch.ones(B, S, dtype=torch.long)
    for i in range(1, B):
        n = int(torch.randint(1, S, (1,), generator=g))
        if pad == "left":
            mask[i, : S - n] = 0          # ColQwen3 pads on the left
        else:
            mask[i, n:] = 0
    return hidden, weight, (b if bias else None), mask


def image_mask_case():
    """(3, 90, 512) bf16 without a bias, with an image-token mask [B, S, 1] (bool) next to the attention mask."""
    hidden, weight, _, mask = case(31, 3, 90, 512, torch.bfloat16, "right", bias=False)
    extra = torch.rand(3, 90, 1, generator=torch.Generator().manual_seed(32)) < 0.7
    return hidden, weight, None, mask, extra


def single_row_case():
    """One kept row in a batch of (2, 9, 64)."""
    hidden, weight, bias, mask = case(33, 2, 9, 64, torch.bfloat16)
    mask.zero_()
    mask[1, 4] = 1
    return hidden, weight, bias, mask


def _step(n: torch.Tensor, by: int) -> torch.Tensor:
    """A positive 16-bit float moved `by` grid steps (its bit pattern as an integer)."""
    return (n.view(torch.int16) + by).view(n.dtype)


def literal_candidates(hidden, weight, bias):
    """[3, M, 320]: the reference's lines on the CPU in the model dtype with the norm unmoved, one grid step down, one up."""
    proj = ho.F.linear(hidden.reshape(-1, hidden.shape[-1]), weight, bias)      # :67
    n = proj.norm(dim=-1, keepdim=True)                                          # :70, the norm
    return torch.stack([proj / n, proj / _step(n, -1), proj / _step(n, +1)])


def exact_chain(hidden, weight, bias):
    """[M, 320]: the same chain with a float64-accumulated Linear output, rounded at the same three places."""
    dtype = hidden.dtype
    y64 = hidden.reshape(-1, hidden.shape[-1]).double() @ weight.double().t()
    if bias is not None:
        y64 = y64 + bias.double()
    y = y64.to(dtype)
    n = y.double().pow(2).sum(-1, keepdim=True).sqrt().to(dtype)
    return (y.double() / n.double()).to(dtype)


def compare_rows(rows: torch.Tensor, cands: torch.Tensor, block: int = 4096):
    """`rows` [R, 320] against `cands` [3, R, 320], each row with its best candidate.
    Returns (unequal share, more-than-one-ulp share, moved-norm row share, largest distance in ulps, R)."""
    R = rows.shape[0]
    unequal = over = moved = 0
    dmax = 0.0
    for s in range(0, R, block):
        r, c = rows[s:s + block], cands[:, s:s + block]
        d, _ = grid_distance(r.unsqueeze(0).expand_as(c), c)
        n_over = (d > 1).sum(-1)                                         # [3, r]
        n_uneq = (r.float().unsqueeze(0) != c.float()).sum(-1)
        best = (n_over * (WIDTH + 1) + n_uneq).argmin(0)                  # first minimum: ties go to the unmoved norm
        pick = best.unsqueeze(0)
        over += int(n_over.gather(0, pick).sum())
        unequal += int(n_uneq.gather(0, pick).sum())
        moved += int((best != 0).sum())
        dmax = max(dmax, float(d.max(-1).values.gather(0, pick).max()) if r.shape[0] else 0.0)
    n_el = max(R * WIDTH, 1)
    return unequal / n_el, over / n_el, moved / max(R, 1), dmax, R


def keep_of(mask, extra=None):
    keep = mask != 0
    if extra is not None:
        keep = keep & (extra.reshape(mask.shape) != 0)
    return keep.reshape(-1)


@functools.lru_cache(maxsize=None)
def reference(seed, B, S, H, dtype, pad="right", bias=True):
    """The case, its candidates over the kept rows, and the reference's own shares: computed once, shared, never modified."""
    hidden, weight, b, mask = case(seed, B, S, H, dtype, pad, bias)
    return (hidden, weight, b, mask) + reference_of(hidden, weight, b, mask)


def reference_of(hidden, weight, bias, mask, extra=None):
    keep = keep_of(mask, extra)
    cands = literal_candidates(hidden, weight, bias)[:, keep]
    ref = compare_rows(exact_chain(hidden, weight, bias)[keep], cands)
    return cands, ref


def check_wide(got, hidden, weight, bias, mask, extra=None, cands=None, ref=None, label=""):
    """Rules 1-4 of the module docstring for a dense [B, S, 320] head output."""
    got = got.cpu()
    assert got.shape == (*mask.shape, WIDTH) and got.dtype == hidden.dtype
    if cands is None:
        cands, ref = reference_of(hidden, weight, bias, mask, extra)
    keep = keep_of(mask, extra)
    flat = got.reshape(-1, WIDTH)
    u, g, r, dmax, R = compare_rows(flat[keep], cands)
    u_ref, g_ref, r_ref, dmax_ref, _ = ref
    n_el = max(R * WIDTH, 1)
    print(f"head_wide {label}: rows {R}  unequal {u:.3e} (ref {u_ref:.3e})  >1ulp {g:.3e} (ref {g_ref:.3e})  "
          f"moved rows {r:.3e} (ref {r_ref:.3e})  max ulps {dmax:.2f} (ref {dmax_ref:.2f})")
    # 1. hard bound
    assert torch.count_nonzero(flat[~keep]) == 0
    assert dmax <= 2.0, dmax
    # 2. truth tier
    truth = ho.head_truth(hidden, weight, bias, mask, extra)
    big = truth.abs() >= 1e-3
    rel = 2.0**-6 if got.dtype == torch.bfloat16 else 2.0**-9
    assert torch.all(((got.double() - truth).abs() <= rel * truth.abs())[big])
    # 3. shares, calibrated by the reference on the same input
    assert u <= 3 * u_ref + 5 / n_el, (u, u_ref)
    assert g <= 3 * g_ref + 5 / n_el, (g, g_ref)
    assert r <= 3 * r_ref + 2 / max(R, 1), (r, r_ref)
    # 4. large bf16 outputs: the project's literal tier, unchanged
    if got.dtype == torch.bfloat16 and got.numel() >= 100_000:
        assert_same_rounding_chain(got, ho.head_literal(hidden, weight, bias, mask, extra))
    return u, g, r, dmax
