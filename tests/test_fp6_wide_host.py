"""E2M3 (FP6) query tokens against the 320-wide FP4 index, without a GPU: the truth helper (tests/fp6_wide_truth.py) on its own edge
cases -- the 240-byte row and the per-lane byte ranges the kernels load, every tie and binade edge of the grid, the m = 1.875
threshold, zero rows, the exponent clamp, the exactness bound --, the ABI's argument checks (no device work) and the Python surface:
query_code, the [T, 240] shape check, the error texts that send a 128-wide caller to fp6_scores / fp6_rerank_scores, exports, and
ShardedRetriever / LiveCorpus taking fp6_wide_scores and fp6_wide_rerank_scores as their hooks."""
import os
import re

import numpy as np
import pytest
import torch

from tests import fp4_wide_truth as wt
from tests import fp6_truth as f6
from tests import fp6_wide_truth as f6w
from tests import live_truth as lt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")
W = 320
ENTRIES = ("msim_f6w_encode_rows", "msim_f4w_scores_q6", "msim_f4w_candidates_q6")


def _bf16(v):
    return int(wt.raw_bits(torch.tensor([[v] * W], dtype=torch.bfloat16))[0, 0])


TIES = [(f6.GRID[c] + f6.GRID[c + 1]) / 2 for c in range(31)]          # every midpoint of neighbouring codes, exact in bf16
EVEN = [c if c % 2 == 0 else c + 1 for c in range(31)]                 # the tie between codes c and c + 1 goes to the even one


def edge_rows():
    """raw bf16 rows for the encoder's edges, shared with the GPU test: (raw uint16 [n, 320], {name: row}).  The edges sit in all
    three K blocks: a row's maximum in block 2 only must set the exponent of the fields in blocks 0 and 1."""
    raw = np.zeros((16, W), dtype=np.uint16)
    raw[0, 319] = _bf16(7.5)                                                    # the maximum in the row's last dimension
    raw[0, 1:32] = [_bf16(t) for t in TIES]                                     # every tie in block 0 ...
    raw[0, 260:291] = [_bf16(-t) for t in TIES]                                 # ... and, negative, in block 2
    raw[1, 100] = _bf16(7.5 * 2.0 ** -9)                                        # the same ties at e = -9, across blocks 1 and 2
    raw[1, 240:271] = [_bf16(t * 2.0 ** -9) for t in TIES]
    raw[2] = 0                                                                  # a row of +0.0
    raw[3] = 0x8000                                                             # a row of -0.0
    raw[4, 300] = _bf16(7.5 * 2.0 ** 3)                                         # the maximum exactly 7.5 * 2^3 ...
    raw[4, 8] = _bf16(2.0 ** 3)
    raw[5] = raw[4]
    raw[5, 300] += 1                                                            # ... and one bf16 ulp above
    raw[6, 256] = _bf16(1.875 * 2.0 ** -4)                                      # m = 1.875 exactly ...
    raw[6, 10] = _bf16(-(2.0 ** -6))
    raw[7] = raw[6]
    raw[7, 256] += 1                                                            # ... and one ulp above
    raw[8, 0], raw[8, 319] = 0x0001, 0x8001                                     # bf16 subnormals only: far below 7.5 * 2^-32
    raw[9, 0], raw[9, 1], raw[9, 290] = _bf16(2.0 ** -31), _bf16(-(2.0 ** -36)), _bf16(2.0 ** -35)   # e clamps at -32; 1/16 ties to 0
    raw[10, 0], raw[10, 301] = _bf16(-(2.0 ** 40)), _bf16(2.0 ** 33)            # e clamps at +32: saturates at -7.5
    raw[11, 5] = _bf16(7.5 * 2.0 ** 32)
    rows = dict(ties=0, ties_small=1, zero=2, neg_zero=3, max_exact=4, max_above=5, m_exact=6, m_above=7, subnormal=8, clamp_lo=9,
                clamp_hi=10, max_at_clamp=11)
    return raw, rows


def edge_rows_f16():
    """raw f16 rows, shared with the GPU test: the largest finite value beside the smallest subnormal, subnormals only, the smallest
    normal beside the largest subnormal, and every tie at e = 0 in blocks 1 and 2"""
    raw16 = np.zeros((4, W), dtype=np.uint16)
    raw16[0, 300], raw16[0, 1] = 0x7bff, 0x0001
    raw16[1, 0], raw16[1, 257], raw16[1, 2] = 0x03ff, 0x8200, 0x0001            # subnormals only: 1023, -512 and 1 times 2^-24
    raw16[2, 0], raw16[2, 319] = 0x0400, 0x03ff                                 # 2^-14 and the largest subnormal
    ties = np.array([7.5] + TIES, dtype=np.float16)
    raw16[3, 200:232] = ties.view(np.uint16)
    raw16[3, 270:302] = (-ties).view(np.uint16)
    return raw16


# ------------------------------------------------------------------------------------------------------------ the truth helper
def test_truth_grid_and_row_size():
    assert f6w.GRID is f6.GRID and len(f6w.GRID) == 32 and f6w.GRID[31] == 7.5
    assert f6w.DIM == 320 and f6w.ROW_BYTES == 240 and (f6w.E_MIN, f6w.E_MAX) == (-32, 32)


def test_truth_pack_and_unpack_every_field_value_at_every_position():
    for k in range(W):
        fields = np.zeros((64, W), dtype=np.uint8)
        fields[:, k] = np.arange(64)
        codes = f6w.pack_fields(fields)
        assert codes.shape == (64, 240) and codes.dtype == np.uint8
        np.testing.assert_array_equal(f6w.unpack_fields(codes), fields)
        word = sum(codes[:, b].astype(object) << (8 * b) for b in range(240))    # the little-endian row as an integer
        assert [int(w) for w in word] == [v << (6 * k) for v in range(64)]       # field k at bit 6 k
    rng = np.random.default_rng(0)
    fields = rng.integers(0, 64, (50, W), dtype=np.uint8)
    np.testing.assert_array_equal(f6w.unpack_fields(f6w.pack_fields(fields)), fields)
    np.testing.assert_array_equal(f6w.decode(f6w.pack_fields(fields)), np.where(fields >> 5, -1.0, 1.0) * f6.GRID[fields & 31])


def test_the_lane_byte_ranges_hold_exactly_the_dimensions_claimed():
    """include/maxsim.h: lane group l4 loads 24 bytes at 96 b + 24 l4 for K block b = 0, 1 -- dimensions 128 b + 32 l4 .. + 31, field
    j of the operand being dimension 128 b + 32 l4 + j -- and 12 bytes at 192 + 12 l4 for block 2 -- dimensions 256 + 16 l4 .. + 15
    as fields 0 .. 15.  A range holds those dimensions whole and no bit of any other; the ranges tile the row."""
    covered = np.zeros(240, dtype=int)
    for b, nbytes, per_lane, base in ((0, 24, 32, 0), (1, 24, 32, 96), (2, 12, 16, 192)):
        for l4 in range(4):
            lo = base + nbytes * l4
            dims = list(range(128 * b + per_lane * l4, 128 * b + per_lane * (l4 + 1)))
            covered[lo:lo + nbytes] += 1
            fields = np.zeros((W, W), dtype=np.uint8)
            fields[np.arange(W), np.arange(W)] = 63                              # row k: all six bits of dimension k
            codes = f6w.pack_fields(fields)
            inside = codes[:, lo:lo + nbytes].any(axis=1)
            outside = np.delete(codes, np.s_[lo:lo + nbytes], axis=1).any(axis=1)
            assert np.flatnonzero(inside).tolist() == dims                       # these dimensions and no other touch the range
            assert not outside[dims].any()                                       # and they lie in it whole
            # field j of the lane's little-endian operand is dimension dims[j]
            rng = np.random.default_rng(lo)
            f = rng.integers(0, 64, (3, W), dtype=np.uint8)
            c = f6w.pack_fields(f)[:, lo:lo + nbytes]
            word = [int(sum(int(c[r, i]) << (8 * i) for i in range(nbytes))) for r in range(3)]
            for j, k in enumerate(dims):
                assert [(w >> (6 * j)) & 63 for w in word] == f[:, k].tolist()
    assert (covered == 1).all()
    # the partners on the page side (tests/fp4_wide_truth.py): 16 bytes at 64 b + 16 l4, 8 bytes at 128 + 8 l4 -- the same dimensions
    for b, nbytes, per_lane, base in ((0, 16, 32, 0), (1, 16, 32, 64), (2, 8, 16, 128)):
        for l4 in range(4):
            nib = np.zeros((W, W), dtype=np.uint8)
            nib[np.arange(W), np.arange(W)] = 15
            lo = base + nbytes * l4
            inside = wt.pack_nibbles(nib)[:, lo:lo + nbytes].any(axis=1)
            assert np.flatnonzero(inside).tolist() == list(range(128 * b + per_lane * l4, 128 * b + per_lane * (l4 + 1)))


def test_truth_every_tie_goes_to_the_even_code_in_every_block():
    raw, rows = edge_rows()
    codes, scales = f6w.encode(raw[:2])
    assert scales.tolist() == [127, 127 - 9]
    f = f6w.unpack_fields(codes)
    assert f[0, 319] == 31 and f[0, 1:32].tolist() == EVEN
    assert f[0, 260:291].tolist() == [0] + [32 | c for c in EVEN[1:]]            # -1/16 rounds to code 0: the field is 0, not 32
    assert f[1, 100] == 31 and f[1, 240:271].tolist() == EVEN
    # just off a tie, the nearer value wins
    eps = 2.0 ** -10
    x = np.zeros((1, W))
    x[0, 0] = 7.5
    x[0, 130:161] = [t + eps for t in TIES]
    x[0, 280:311] = [t - eps for t in TIES]
    f = f6w.unpack_fields(f6w.encode_values(x)[0])
    assert f[0, 130:161].tolist() == list(range(1, 32)) and f[0, 280:311].tolist() == list(range(31))


def test_truth_every_binade_edge_of_the_grid():
    """the values where the grid's step changes (1, 2, 4), the subnormal edge (7/8 | 1) and the top (7.5), each exact, and the
    neighbours half a lower step and half an upper step away"""
    x = np.zeros((1, W))
    x[0, 319] = 7.5
    probe = {0.875: 7, 1.0: 8, 1.875: 15, 2.0: 16, 2.125: 16, 2.25: 17, 3.75: 23, 3.875: 24, 4.0: 24, 4.25: 24, 4.5: 25, 7.0: 30, 7.25: 30,
             7.5: 31, 1.9375: 16, 0.9375: 8, 0.0625: 0, 0.1875: 2}
    for j, v in enumerate(probe):
        x[0, 3 * j] = v
    f = f6w.unpack_fields(f6w.encode_values(x)[0])
    assert [int(f[0, 3 * j]) for j in range(len(probe))] == list(probe.values())
    np.testing.assert_array_equal(f6w.nearest_codes(f6.GRID), np.arange(32))


@pytest.mark.parametrize("e", [-32, -7, 0, 3, 32])
@pytest.mark.parametrize("k", [3, 200, 319])
def test_truth_exponent_at_a_maximum_of_seven_and_a_half_and_one_ulp_above(e, k):
    raw = np.zeros((2, W), dtype=np.uint16)
    raw[0, k] = _bf16(7.5 * 2.0 ** e)
    raw[1, k] = raw[0, k] + 1                                     # one bf16 ulp above 7.5 * 2^e: 7.53125 * 2^e
    raw[:, 4] = _bf16(2.0 ** e)
    codes, scales = f6w.encode(raw)
    f = f6w.unpack_fields(codes)
    assert scales[0] == e + 127 and f[0, k] == 31 and f[0, 4] == 8             # a == 7.5 * 2^e: e, code 31; 2^e is 1.0
    if e < 32:
        assert scales[1] == e + 128 and f[1, k] == 23 and f[1, 4] == 4         # above: e + 1, 3.765625 -> 3.75; 2^e is 0.5
    else:
        assert scales[1] == 32 + 127 and f[1, k] == 31 and f[1, 4] == 8        # the clamp: y = min(., 7.5)


def test_truth_mantissa_threshold_zero_rows_and_the_exponent_clamps():
    raw, rows = edge_rows()
    codes, scales = f6w.encode(raw)
    f = f6w.unpack_fields(codes)
    assert scales[rows["m_exact"]] == 127 - 4 - 2 and f[rows["m_exact"], 256] == 31 and f[rows["m_exact"], 10] == 32 | 8     # 7.5, -1.0
    assert scales[rows["m_above"]] == 127 - 4 - 1 and f[rows["m_above"], 256] == 23 and f[rows["m_above"], 10] == 32 | 4    # 3.75, -0.5
    assert scales[rows["max_exact"]] == 130 and scales[rows["max_above"]] == 131
    assert scales[rows["zero"]] == 127 and scales[rows["neg_zero"]] == 127 and not codes[[rows["zero"], rows["neg_zero"]]].any()
    assert scales[rows["subnormal"]] == 127 - 32 and not codes[rows["subnormal"]].any()
    r = rows["clamp_lo"]
    assert scales[r] == 127 - 32 and [int(f[r, k]) for k in (0, 1, 290)] == [16, 0, 1]     # 2.0; -1/16 ties to 0; 1/8
    r = rows["clamp_hi"]
    assert scales[r] == 127 + 32 and [int(f[r, k]) for k in (0, 301)] == [32 | 31, 16]     # saturates at -7.5; 2^33 = 2 * 2^32
    assert scales[rows["max_at_clamp"]] == 127 + 32 and f[rows["max_at_clamp"], 5] == 31
    raw16 = edge_rows_f16()
    c16, s16 = f6w.encode(raw16, f16=True)
    f = f6w.unpack_fields(c16)
    assert s16[0] == 127 + 14 and [int(f[0, k]) for k in (300, 1)] == [24, 0]
    assert s16[1] == 127 - 16 and [int(f[1, k]) for k in (0, 257, 2)] == [24, 32 | 16, 0]
    assert s16[2] == 127 - 16 and [int(f[2, k]) for k in (0, 319)] == [24, 24]
    assert s16[3] == 127 and f[3, 200:232].tolist() == [31] + EVEN and f[3, 270:302].tolist() == [63, 0] + [32 | c for c in EVEN[1:]]


def test_the_exactness_bound_at_the_extreme_row():
    """|I| * 16 < 2^24 where it is largest: every field 7.5 against every nibble 6 (and the negative one), and the truth's float32
    check passes there."""
    qc, qs = f6w.encode_values(np.stack([np.full(W, 7.5), np.full(W, -7.5)]))
    dc, ds = wt.encode_values(np.full((1, W), 6.0))
    assert (f6w.unpack_fields(qc)[0] == 31).all() and (f6w.unpack_fields(qc)[1] == 63).all() and (wt.unpack_nibbles(dc) == 7).all()
    I = f6w.decode(qc) @ wt.decode(dc).T
    assert I.ravel().tolist() == [14400.0, -14400.0] and abs(I).max() * 16 == 230400 < 2 ** 24
    assert np.array_equal(I * 16, np.round(I * 16))
    M = f6w.maxima(qc, qs, dc, ds, np.array([0, 1]))
    assert M.ravel().tolist() == [14400.0, -14400.0]
    # every partial sum of any order is a multiple of 1/16 no larger than the full sum of magnitudes
    rng = np.random.default_rng(1)
    fq = rng.integers(0, 64, (8, W), dtype=np.uint8)
    nd = rng.integers(0, 16, (8, W), dtype=np.uint8)
    P = np.abs(f6w.decode(f6w.pack_fields(fq)))[:, None, :] * np.abs(wt.decode(wt.pack_nibbles(nd)))[None, :, :]
    assert P.sum(axis=2).max() <= 14400 and np.array_equal(P * 16, np.round(P * 16))


def test_truth_scores_order_clamp_and_empty_pages():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, W)) * np.exp2(rng.integers(-6, 6, (40, 1)))
    dc, ds = wt.encode_values(x)
    qc, qs = f6w.encode_values(rng.standard_normal((9, W)))
    d_off = np.array([0, 0, 7, 7, 23, 40, 40])
    q_off = np.array([0, 0, 4, 9])
    clamp0 = np.array([1, 0, 0, 1, 0, 1], dtype=np.uint8)
    M = f6w.maxima(qc, qs, dc, ds, d_off, clamp0)
    vq = f6w.decode(qc) * np.exp2(qs.astype(np.int64) - 127)[:, None]
    vd = wt.decode(dc) * np.exp2(ds.astype(np.int64) - 127)[:, None]
    Z = vq @ vd.T
    for c in (1, 3, 4):
        m = Z[:, d_off[c]:d_off[c + 1]].max(axis=1)
        np.testing.assert_array_equal(M[:, c].astype(np.float64), np.maximum(m, 0) if clamp0[c] else m)
    S = f6w.scores(qc, qs, q_off, dc, ds, d_off, clamp0)
    assert np.isneginf(S[:, [0, 2, 5]]).all()
    assert (S[0, [1, 3, 4]] == 0).all()                           # a query without tokens
    t = np.float32(0)
    for k in range(4, 9):
        t = np.float32(t + M[k, 4])
    assert S[2, 4] == t
    # a row in blocks 0 and 1 only scores as the 128-wide truth does on each half
    blocks = [wt.raw_bits(torch.randn(3, W).to(torch.bfloat16))]
    assert f6w.score_blocks(blocks, wt.raw_bits(torch.randn(5, W).to(torch.bfloat16)), np.array([0, 2, 5])).shape == (1, 2)


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_header_binding_and_exports():
    import colpali_amd
    from colpali_amd import fp4_wide_index, retrieval

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    assert re.search(r"msim_f6w_encode_rows\(int dtype, const void \*X, int64_t n_rows, int dim, uint8_t \*codes /\* \[n_rows, 240\] \*/", header)
    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    assert L.msim_f6w_encode_rows.argtypes == L.msim_f4w_encode_rows.argtypes
    assert L.msim_f4w_scores_q6.argtypes == L.msim_f4w_scores.argtypes
    assert L.msim_f4w_candidates_q6.argtypes == L.msim_f4w_candidates.argtypes
    assert fp4_wide_index.Q6_ROW_BYTES == 240 and fp4_wide_index.QUERY_CODES == {"e2m1": 160, "e2m3": 240}
    for name in ("fp6_wide_scores", "fp6_wide_rerank_scores", "fp6_wide_quantize_queries"):
        assert name in colpali_amd.__all__ and hasattr(colpali_amd, name)
    assert "fp6_wide_scores" in colpali_amd.__doc__ and "fp6_wide_rerank_scores" in colpali_amd.__doc__
    assert colpali_amd.fp6_wide_scores in retrieval._KERNELS and colpali_amd.fp6_wide_rerank_scores in retrieval._KERNELS


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def rows(dtype=0, x=FAKE, n=40, dim=W, codes=FAKE, scales=FAKE + 3):
        return L.msim_f6w_encode_rows(dtype, x, n, dim, codes, scales, None)

    def score(q6=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90,
              dim=W, out=FAKE, ld=10):
        return L.msim_f4w_scores_q6(q6, qs, qo, n_q, q_rows, maxq, d4, ds, do, c0, n_d, d_rows, dim, out, ld, None)

    def cand(q=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90,
             dim=W, cand=FAKE, m=6, ld_cand=6, id_base=0, out=FAKE, ld=6, ids=FAKE):
        return L.msim_f4w_candidates_q6(q, qs, qo, n_q, q_rows, maxq, d4, ds, do, c0, n_d, d_rows, dim, cand, m, ld_cand, id_base, out,
                                        ld, ids, None)

    assert rows(n=0) == 0 and rows(n=0, x=None, codes=None, scales=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, q6=None, d4=None, out=None) == 0
    for kw in (dict(n=-1), dict(x=None), dict(codes=None), dict(scales=None), dict(x=FAKE + 8), dict(codes=FAKE + 4)):
        assert rows(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(dtype=2), dict(dtype=7)):
        assert rows(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q6=None), dict(qs=None),
               dict(qo=None), dict(d4=None), dict(ds=None), dict(do=None), dict(out=None), dict(q6=FAKE + 4), dict(d4=FAKE + 8),
               dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(maxq=(1 << 20) + 1)):
        assert score(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    assert cand(n_q=0) == 0 and cand(m=0, ld_cand=0, ld=0) == 0
    assert cand(n_q=0, q=None, d4=None, cand=None, out=None) == 0 and cand(m=0, q=None, qo=None, do=None, cand=None, out=None) == 0
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(m=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q=None), dict(qs=None),
               dict(qo=None), dict(d4=None), dict(ds=None), dict(do=None), dict(cand=None), dict(out=None), dict(q=FAKE + 8),
               dict(d4=FAKE + 4), dict(qo=FAKE + 2), dict(do=FAKE + 1), dict(out=FAKE + 2), dict(cand=FAKE + 4), dict(ids=FAKE + 4),
               dict(ld_cand=5), dict(ld=5)):
        assert cand(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(maxq=129), dict(n_q=1 << 30, m=1 << 4, ld_cand=16, ld=16)):
        assert cand(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    # the 128-wide e2m3 entries keep refusing width 320
    assert L.msim_f6_encode_rows(0, FAKE, 40, W, FAKE, FAKE, None) == EUNSUPPORTED
    assert L.msim_f4_scores_q6(FAKE, FAKE, FAKE, 4, 40, 32, FAKE, FAKE, FAKE, None, 10, 90, W, FAKE, 10, None) == EUNSUPPORTED


# ------------------------------------------------------------------------------------------------------------ the Python layer
def _page(g, n, dim=W, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _index(shard):
    from colpali_amd import Fp4WideIndex

    codes, scales = wt.encode(wt.raw_bits(shard.blob))
    return Fp4WideIndex(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                        shard.id_base)


def _shard(n=6, rows=4, id_base=7, dim=W):
    import colpali_amd

    g = torch.Generator().manual_seed(3)
    return colpali_amd.pack_passages([_page(g, rows, dim) for _ in range(n)], CPU, batch_size=None, id_base=id_base)


def test_query_code_and_shape_refusals_without_a_gpu():
    import colpali_amd

    idx = _index(_shard())
    q = torch.randn(2, 4, W).to(torch.bfloat16)
    off = torch.tensor([0, 4, 8], dtype=torch.int32)
    scales = torch.zeros(8, dtype=torch.uint8)
    cands = torch.zeros((2, 3), dtype=torch.int64)
    for bad in ("e3m2", "fp6", "", None):
        with pytest.raises(ValueError, match="query_code must be 'e2m1' or 'e2m3'"):
            colpali_amd.fp4_wide_scores(q, idx, query_code=bad)
        with pytest.raises(ValueError, match="query_code must be 'e2m1' or 'e2m3'"):
            colpali_amd.fp4_wide_scores_from_codes(torch.zeros(8, 240, dtype=torch.uint8), scales, off, 4, idx, query_code=bad)
        with pytest.raises(ValueError, match="query_code must be 'e2m1' or 'e2m3'"):
            colpali_amd.fp4_wide_rerank_scores(q, idx, cands, query_code=bad)
    with pytest.raises(ValueError, match=r"e2m3 query codes must be a contiguous uint8 \[tokens, 240\]"):
        colpali_amd.fp4_wide_scores_from_codes(torch.zeros(8, 160, dtype=torch.uint8), scales, off, 4, idx, query_code="e2m3")
    with pytest.raises(ValueError, match=r"e2m3 query codes must be a contiguous uint8 \[tokens, 240\]"):
        colpali_amd.fp4_wide_scores_from_codes(torch.zeros(8, 96, dtype=torch.uint8), scales, off, 4, idx, query_code="e2m3")
    with pytest.raises(ValueError, match=r"e2m1 query codes must be a contiguous uint8 \[tokens, 160\]"):
        colpali_amd.fp4_wide_scores_from_codes(torch.zeros(8, 240, dtype=torch.uint8), scales, off, 4, idx)
    with pytest.raises(TypeError):
        colpali_amd.fp4_wide_scores(q, idx, None, "e2m3")          # query_code is keyword-only
    with pytest.raises(TypeError):
        colpali_amd.fp6_wide_scores(q, idx, query_code="e2m1")     # and the e2m3 functions have none


def test_a_128_wide_caller_is_sent_to_the_128_wide_functions():
    import colpali_amd
    from tests import fp4_truth as ft

    idx = _index(_shard())
    narrow = _shard(dim=128)
    nc, ns = ft.encode(ft.raw_bits(narrow.blob))
    narrow_idx = colpali_amd.Fp4Index(torch.from_numpy(nc), torch.from_numpy(ns), narrow.offsets.clone(), None, narrow.lengths.clone(), 7)
    q128 = torch.randn(2, 4, 128).to(torch.bfloat16)
    q320 = torch.randn(2, 4, W).to(torch.bfloat16)
    cands = torch.full((2, 3), 7, dtype=torch.int64)
    # the width check of the query tokens (on a GPU the packed queries reach it; tests/test_gpu_fp6_wide.py goes through the functions)
    from colpali_amd import fp4_wide_index as mod

    with pytest.raises(NotImplementedError, match=r"queries of width 320 \(got torch.bfloat16, width 128\).*Fp4Index / fp6_scores"):
        mod._check_format(q128.dtype, 128, "queries", "e2m3")
    with pytest.raises(NotImplementedError, match=r"queries of width 320 \(got torch.bfloat16, width 128\).*Fp4Index / fp4_scores"):
        mod._check_format(q128.dtype, 128, "queries")
    with pytest.raises(NotImplementedError, match=r"queries of width 320 \(got torch.float32, width 320\)$"):
        mod._check_format(torch.float32, W, "queries", "e2m3")
    with pytest.raises(TypeError, match=r"takes an Fp4WideIndex \(got Fp4Index\).*fp6_scores"):
        colpali_amd.fp6_wide_scores(q320, narrow_idx)
    with pytest.raises(NotImplementedError, match=r"Fp4WideIndex of a 320-wide shard \(got Fp4Index\); an Fp4Index of a 128-wide shard takes "
                                                  r"fp6_rerank_scores"):
        colpali_amd.fp6_wide_rerank_scores(q320, narrow_idx, cands)
    with pytest.raises(NotImplementedError, match=r"\(got Fp4Index\); an Fp4Index of a 128-wide shard takes fp4_rerank_scores"):
        colpali_amd.fp4_wide_rerank_scores(q320, narrow_idx, cands)
    with pytest.raises(NotImplementedError, match=r"Fp4WideIndex of a 320-wide shard \(got PackedCorpus\)$"):
        colpali_amd.fp6_wide_rerank_scores(q320, _shard(), cands)


# ----------------------------------------------------------------------------------------------------------------- the hooks
def _gather(full, candidates, id_base):
    n = full.shape[1]
    d = candidates - id_base
    ok = (candidates >= 0) & (d >= 0) & (d < n)
    got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0))) if n else torch.zeros(candidates.shape)
    return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))


def _blocks(queries):
    """host bf16 blocks of what a retriever hands a kernel hook: a PackedQueries (flat) or the caller's tensor"""
    if hasattr(queries, "offsets_host"):
        o = queries.offsets_host.tolist()
        return [queries.tokens[o[i]:o[i + 1]].cpu() for i in range(len(o) - 1)]
    return list(queries)


@pytest.fixture()
def stubbed(monkeypatch):
    """fp6_wide_scores / fp6_wide_rerank_scores as they stand, with the two functions they call replaced by the e2m3 truth: the
    hooks under test are the package's own function objects, only the device work is stubbed.  `calls` records (name, query_code)."""
    from colpali_amd import fp4_wide_index as mod

    calls = []

    def scores(queries, index, out=None, *, query_code="e2m1"):
        calls.append(("scores", query_code))
        assert query_code == "e2m3" and isinstance(index, mod.Fp4WideIndex)
        qb = [wt.raw_bits(x.to(torch.bfloat16)) for x in _blocks(queries)]
        qc, qs = f6w.encode(np.concatenate(qb))
        q_off = np.cumsum([0] + [len(x) for x in qb])
        c0 = None if index.clamp0 is None else index.clamp0.numpy()
        return torch.from_numpy(f6w.scores(qc, qs, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), c0))

    def rerank(queries, index, candidates, *, query_code="e2m1", out=None):
        calls.append(("rerank", query_code))
        return _gather(scores(queries, index, query_code=query_code), candidates, index.id_base)

    monkeypatch.setattr(mod, "fp4_wide_scores", scores)
    monkeypatch.setattr(mod, "fp4_wide_rerank_scores", rerank)
    return calls


def _host_hooks():
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    def score_fn(queries, corpus):
        qb = torch.stack(_blocks(queries)) if not isinstance(queries, torch.Tensor) else queries
        return torch.from_numpy(mo.maxsim_f32(qb.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        return _gather(score_fn(queries, corpus), candidates, corpus.id_base)

    return dict(score_fn=score_fn, rerank_fn=rerank_fn, select=topk_oracle.torch_select)


def test_sharded_retriever_takes_the_two_functions_as_hooks(stubbed):
    import colpali_amd
    from oracle import topk_oracle

    g = torch.Generator().manual_seed(5)
    pages = [_page(g, int(n)) for n in torch.randint(1, 30, (23,), generator=g)]
    q = torch.nn.functional.normalize(torch.randn(4, 8, W, generator=g), dim=-1).to(torch.bfloat16)
    shard = colpali_amd.pack_passages(pages, CPU, batch_size=None, id_base=7)
    idx = _index(shard)
    r = colpali_amd.ShardedRetriever(shard, fp4_wide_score_fn=colpali_amd.fp6_wide_scores,
                                     fp4_wide_rerank_fn=colpali_amd.fp6_wide_rerank_scores, **_host_hooks())
    s, i = r.search(q, 4, prefilter=idx, n_candidates=9)
    assert stubbed == [("scores", "e2m3")] and i.shape == (4, 4) and (i >= 7).all()
    # the list the exact rerank saw is the e2m3 truth's top 9
    qb = [wt.raw_bits(x) for x in q]
    want = topk_oracle.topk(f6w.score_blocks(qb, wt.raw_bits(shard.blob), shard.offsets.numpy()), 9, 7)[1]
    exact = _host_hooks()["rerank_fn"](q, shard, torch.from_numpy(want))
    ws, wi = topk_oracle.topk(exact[0].numpy(), 4, 0, exact[1].numpy())
    np.testing.assert_array_equal(i.numpy(), wi)
    np.testing.assert_array_equal(s.numpy().view(np.int32), ws.view(np.int32))
    del stubbed[:]
    all_ids = torch.arange(7, 30, dtype=torch.int64).expand(4, 23)
    a = r.search(q, 4, candidates=all_ids, refine=idx, n_refine=9)              # refining every page is the e2m3 first stage
    assert stubbed == [("rerank", "e2m3"), ("scores", "e2m3")]
    np.testing.assert_array_equal(a[1].numpy(), i.numpy())
    np.testing.assert_array_equal(a[0].numpy().view(np.int32), s.numpy().view(np.int32))


def test_live_corpus_takes_the_two_functions_as_hooks(stubbed):
    import colpali_amd

    g = torch.Generator().manual_seed(6)
    pages = [_page(g, int(n)) for n in torch.randint(1, 20, (20,), generator=g)]
    q = torch.nn.functional.normalize(torch.randn(3, 8, W, generator=g), dim=-1).to(torch.bfloat16)
    live = colpali_amd.LiveCorpus(sum(len(p) for p in pages) + 3, 22, CPU, width=W, id_base=11,
                                  fp4_wide_score_fn=colpali_amd.fp6_wide_scores, fp4_wide_rerank_fn=colpali_amd.fp6_wide_rerank_scores,
                                  mask_fn=lambda scores, alive: torch.from_numpy(lt.mask(scores.numpy(), alive.numpy())), **_host_hooks())
    live.add(pages)
    idx = _index(live.view())
    deleted = [11 + c for c in range(1, 20, 3)]
    live.delete(deleted)
    all_ids = torch.arange(11, 31, dtype=torch.int64).expand(3, 20)
    s, i = live.search(q, 5, candidates=all_ids, refine=idx, n_refine=6)
    assert ("rerank", "e2m3") in stubbed and not np.isin(i.numpy(), deleted).any() and (i >= 11).all()
    del stubbed[:]
    s2, i2 = live.search(q, 5, prefilter=idx, n_candidates=6)
    assert ("scores", "e2m3") in stubbed and not np.isin(i2.numpy(), deleted).any()
    np.testing.assert_array_equal(i2.numpy(), i.numpy())
    np.testing.assert_array_equal(s2.numpy().view(np.int32), s.numpy().view(np.int32))
