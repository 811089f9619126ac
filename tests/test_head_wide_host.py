"""The 320-wide embedding head without a GPU: the comparison rule of tests/head_wide_truth.py calibrated on the reference alone for
every case tests/test_gpu_head_wide.py uses, the two prototypes of include/maxsim.h with their bindings, every refusal of
msim_embed_head_wide / msim_embed_head_wide_bwd (no device work), and the Python-side width checks."""
import os
import re

import pytest
import torch

from tests import head_wide_truth as wt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------------ the rule
def _assert_rule_is_meaningful(ref, label):
    u_ref, g_ref, r_ref, dmax_ref, rows = ref
    print(f"{label}: rows {rows}  u_ref {u_ref:.3e}  g_ref {g_ref:.3e}  r_ref {r_ref:.3e}  max ulps {dmax_ref:.2f}")
    assert dmax_ref <= 2.0, (label, dmax_ref)           # rule 1 holds for the reference alone
    assert u_ref <= 5e-3, (label, u_ref)
    assert r_ref <= 0.02, (label, r_ref)


@pytest.mark.parametrize("name,seed,B,S,H,dtype,pad", wt.FORWARD_CASES, ids=[c[0] for c in wt.FORWARD_CASES])
def test_reference_alone_meets_the_rule(name, seed, B, S, H, dtype, pad):
    hidden, weight, bias, mask, cands, ref = wt.reference(seed, B, S, H, dtype, pad)
    assert weight.shape == (320, H) and bias.shape == (320,) and cands.shape == (3, int(mask.sum()), 320)
    _assert_rule_is_meaningful(ref, name)


def test_reference_alone_meets_the_rule_on_the_masked_and_single_row_cases():
    hidden, weight, bias, mask, extra = wt.image_mask_case()
    _assert_rule_is_meaningful(wt.reference_of(hidden, weight, bias, mask, extra)[1], "image mask, no bias")
    hidden, weight, bias, mask = wt.single_row_case()
    _assert_rule_is_meaningful(wt.reference_of(hidden, weight, bias, mask)[1], "single kept row")


def test_the_exact_chain_passes_its_own_check_and_a_broken_output_does_not():
    """check_wide on the CPU: the exactly-accumulated chain is inside its own shares; an output with one row's norm two grid steps
    off, or one element three ulps off, is refused."""
    seed, B, S, H, dtype, pad = wt.FORWARD_CASES[1][1:]
    hidden, weight, bias, mask, cands, ref = wt.reference(seed, B, S, H, dtype, pad)
    good = (wt.exact_chain(hidden, weight, bias) * mask.reshape(-1, 1).to(dtype)).reshape(B, S, 320)
    wt.check_wide(good, hidden, weight, bias, mask, cands=cands, ref=ref, label="exact chain")
    bad = good.clone()
    bad[0, 3, 7] = (bad[0, 3, 7].view(torch.int16) + 3).view(dtype)
    with pytest.raises(AssertionError):
        wt.check_wide(bad, hidden, weight, bias, mask, cands=cands, ref=ref)
    bad = good.clone()
    bad[0, 5] = (bad[0, 5].float() * 1.03).to(dtype)                       # a norm several grid steps away
    with pytest.raises(AssertionError):
        wt.check_wide(bad, hidden, weight, bias, mask, cands=cands, ref=ref)
    bad = good.clone()
    bad[1, S - 1, 0] = 1.0                                                 # a masked position that is not zero
    assert mask[1, S - 1] == 0
    with pytest.raises(AssertionError):
        wt.check_wide(bad, hidden, weight, bias, mask, cands=cands, ref=ref)


# ------------------------------------------------------------------------------------------------------------------ header, bindings
def test_header_declares_the_two_entries_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "maxsim.h")) as f:
        text = re.sub(r"\s+", " ", f.read())
    assert ("int msim_embed_head_wide(int dtype, const void *X, int64_t M, int H, const void *W, const void *bias, int n_out, "
            "const int32_t *row_map, void *out, int64_t ld_out, void *stream);") in text
    assert ("int msim_embed_head_wide_bwd(int dtype, const void *proj, const void *grad_out, const int32_t *row_map, int64_t M, "
            "int n_out, void *dproj, void *stream);") in text
    assert "#define MSIM_ABI_VERSION 22" in text


def test_bindings():
    import ctypes

    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert L.msim_embed_head_wide.argtypes == [i32, vp, i64, i32, vp, vp, i32, vp, vp, i64, vp] and L.msim_embed_head_wide.restype is i32
    assert L.msim_embed_head_wide_bwd.argtypes == [i32, vp, vp, vp, i64, i32, vp, vp] and L.msim_embed_head_wide_bwd.restype is i32
    assert colpali_amd.embed.HEAD_DIM == 128 and colpali_amd.embed.HEAD_DIMS == (128, 320)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _head(L, entry="msim_embed_head_wide", dtype=0, X=FAKE, M=300, H=128, W=FAKE, b=FAKE, n_out=320, rm=FAKE, out=FAKE, ld=320):
    return getattr(L, entry)(dtype, X, M, H, W, b, n_out, rm, out, ld, None)


def _bwd(L, entry="msim_embed_head_wide_bwd", dtype=0, pr=FAKE, g=FAKE, rm=FAKE, M=300, n_out=320, dp=FAKE):
    return getattr(L, entry)(dtype, pr, g, rm, M, n_out, dp, None)


def test_forward_entry_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert _head(L, M=0) == 0
    assert _head(L, M=0, X=None, W=None, rm=None, out=None) == 0           # nothing to do: no pointer is looked at
    for kw in (dict(X=None), dict(W=None), dict(rm=None), dict(out=None), dict(M=-1), dict(H=0), dict(H=-64), dict(X=FAKE + 2),
               dict(X=FAKE + 8), dict(W=FAKE + 2), dict(out=FAKE + 8), dict(ld=319), dict(ld=128), dict(ld=324), dict(ld=0)):
        assert _head(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=3), dict(n_out=128), dict(n_out=64), dict(n_out=321), dict(H=96), dict(H=4160), dict(H=8192),
               dict(M=0x7FFFFFFE)):
        assert _head(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    assert _head(L, n_out=128) == EUNSUPPORTED and b"msim_embed_head" in L.msim_last_error() and b"128" in L.msim_last_error()


def test_backward_entry_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert _bwd(L, M=0) == 0
    assert _bwd(L, M=0, pr=None, g=None, rm=None, dp=None) == 0
    for kw in (dict(pr=None), dict(g=None), dict(rm=None), dict(dp=None), dict(M=-1), dict(pr=FAKE + 2), dict(g=FAKE + 8),
               dict(dp=FAKE + 2)):
        assert _bwd(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=3), dict(n_out=128), dict(n_out=64), dict(M=0x7FFFFFFE)):
        assert _bwd(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    assert _bwd(L, n_out=128) == EUNSUPPORTED and b"msim_embed_head" in L.msim_last_error()


def test_the_128_wide_entries_still_refuse_width_320():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert _head(L, entry="msim_embed_head", n_out=320) == EUNSUPPORTED
    assert b"n_out=320: the embedding head is built for 128 output columns" in L.msim_last_error()
    assert _bwd(L, entry="msim_embed_head_bwd", n_out=320) == EUNSUPPORTED
    assert b"n_out=320: the embedding head is built for 128 output columns" in L.msim_last_error()


# ------------------------------------------------------------------------------------------------------------------ Python
def test_embedding_head_names_both_widths_for_any_other():
    import colpali_amd

    hidden = torch.zeros(1, 4, 64, dtype=torch.bfloat16)
    for rows in (64, 127, 321):
        with pytest.raises(ValueError) as e:
            colpali_amd.embedding_head(hidden, torch.zeros(rows, 64, dtype=torch.bfloat16), None, torch.ones(1, 4, dtype=torch.long))
        assert "[128, hidden]" in str(e.value) and "[320, hidden]" in str(e.value) and str(rows) in str(e.value)
    for rows in (128, 320):            # a width that exists gets as far as the device check
        with pytest.raises(RuntimeError, match="MI355X only"):
            colpali_amd.embedding_head(hidden, torch.zeros(rows, 64, dtype=torch.bfloat16), None, torch.ones(1, 4, dtype=torch.long))


def test_corpus_writer_refuses_other_widths():
    import colpali_amd

    with pytest.raises(ValueError) as e:
        colpali_amd.CorpusWriter(16, "cpu", width=96)
    assert "96" in str(e.value) and "128" in str(e.value) and "320" in str(e.value)
    for width in (128, 320):
        w = colpali_amd.CorpusWriter(16, "cpu", width=width)
        assert w.blob.shape == (16, width) and w.width == width
    assert colpali_amd.CorpusWriter(16, "cpu").blob.shape == (16, 128)
