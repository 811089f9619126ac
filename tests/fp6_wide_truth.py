"""Numpy restatement of e2m3 (FP6) query tokens against the FP4 index at width 320 (include/maxsim.h: msim_f6w_encode_rows,
msim_f4w_scores_q6), independent of colpali_amd.  The page side is tests/fp4_wide_truth.py; the e2m3 grid and its nearest-code
search are those of tests/fp6_truth.py.

Query row code, on the stored bf16 / f16 values: msim_f6_encode_rows' rule over 320 dimensions.  a = max over all 320 |x_k|; a == 0:
every field 0, scale byte 127; otherwise e = the smallest integer with a <= 7.5 * 2^e, clamped to [-32, 32]; y_k = min(|x_k| * 2^-e,
7.5); the code is the nearest of the 32 e2m3 magnitudes, a tie going to the even code; field = sign << 5 | code (0 when the code is
0); scale byte = e + 127.  A token is 240 code bytes: dimension k is the 6-bit field at bit 6 k of the little-endian row.  NaN
elements are unspecified.
Score: I_ij = sum_{k<320} v(q_ik) v(d_jk) (a multiple of 1/16, |I| <= 14 400); Z_ij = I_ij * 2^(eq_i + ed_j); M_ic = max_j Z_ij over
a page's rows, max(M_ic, 0) under clamp0; score = the sequential float32 sum of M_ic in token order.  A page of 0 rows scores -inf.
Everything up to M is computed in float64, where it is exact, and every M is asserted to be a float32.
"""
import numpy as np

from tests import fp4_wide_truth as fw
from tests import fp6_truth as f6

GRID = f6.GRID                                           # code -> magnitude, 32 values
E_MIN, E_MAX = fw.E_MIN, fw.E_MAX
DIM = fw.DIM
ROW_BYTES = DIM * 6 // 8                                 # 240
raw_bits, values = fw.raw_bits, fw.values
nearest_codes = f6.nearest_codes


def row_exponents(x):
    """int64 [n]: e of every row of x float64 [n, 320] (0 for a zero row): the smallest integer with max |x| <= 7.5 * 2^e, clamped"""
    a = np.abs(x).max(axis=1) if x.shape[0] else np.zeros(0)
    f, p = np.frexp(a)                                   # a = f * 2^p, 0.5 <= f < 1, exact; 7.5 * 2^e = 0.9375 * 2^(e + 3)
    e = np.where(f <= 0.9375, p - 3, p - 2).astype(np.int64)
    e = np.clip(e, E_MIN, E_MAX)
    return np.where(a == 0, 0, e)


def pack_fields(fields):
    """codes uint8 [n, 240] of 6-bit fields [n, 320]: field k at bit 6 k of the little-endian row"""
    f = np.asarray(fields, dtype=np.uint8).reshape(-1, DIM)
    assert (f < 64).all()
    bits = (f[..., None] >> np.arange(6, dtype=np.uint8)) & 1                       # [n, 320, 6]: bit b of field k is bit 6 k + b
    return np.packbits(bits.reshape(-1, DIM * 6), axis=-1, bitorder="little").reshape(-1, ROW_BYTES)


def unpack_fields(codes):
    """6-bit fields uint8 [n, 320] of codes uint8 [n, 240]"""
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, ROW_BYTES)
    bits = np.unpackbits(c, axis=-1, bitorder="little").reshape(-1, DIM, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)


def encode_values(x):
    """(codes uint8 [n, 240], scales uint8 [n]) of x float64 [n, 320] (values a bf16 / f16 tensor stores)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, DIM)
    e = row_exponents(x)
    y = np.minimum(np.ldexp(np.abs(x), -e[:, None]), 7.5)
    code = nearest_codes(y)
    field = np.where(code > 0, code | (np.signbit(x).astype(np.int64) << 5), 0).astype(np.uint8)
    return pack_fields(field), (e + 127).astype(np.uint8)


def encode(raw16, f16=False):
    """(codes, scales) of the raw 16-bit patterns of bf16 / f16 query tokens"""
    return encode_values(values(raw16, f16))


def decode(codes):
    """float64 [n, 320]: the grid values (with sign) of codes uint8 [n, 240]"""
    f = unpack_fields(codes)
    return np.where(f >> 5, -1.0, 1.0) * GRID[f & 31]


def maxima(qc, qs, dc, ds, d_off, clamp0=None, block=64, row_block=1 << 16):
    """float32 [T, n]: M_ic of e2m3 tokens (qc [T, 240], qs [T]) against FP4 pages (dc [R, 160], ds [R], offsets d_off); -inf for a
    page of 0 rows (0 under clamp0).  Asserts that every maximum is a float32.  The pages are decoded `row_block` rows at a time
    (whole pages)."""
    d_off = np.asarray(d_off, dtype=np.int64)
    n, T = len(d_off) - 1, len(qs)
    vq = decode(qc)
    eq, ed = np.asarray(qs, dtype=np.int64) - 127, np.asarray(ds, dtype=np.int64) - 127
    M32 = np.full((T, n), -np.inf, dtype=np.float32)
    c0 = None if clamp0 is None else np.asarray(clamp0).astype(bool)
    p0 = 0
    while p0 < n and T:
        p1 = max(int(np.searchsorted(d_off, d_off[p0] + row_block, side="right")) - 1, p0 + 1)   # pages p0 .. p1 - 1: whole pages
        p1 = min(p1, n)
        r0, r1 = int(d_off[p0]), int(d_off[p1])
        full = p0 + np.flatnonzero(d_off[p0 + 1:p1 + 1] > d_off[p0:p1])
        if len(full):
            vd = fw.decode(dc[r0:r1])
            for t0 in range(0, T, block):
                I = vq[t0:t0 + block] @ vd.T                                          # multiples of 1/16 below 2^14: exact
                Z = np.ldexp(I, eq[t0:t0 + block, None] + ed[None, r0:r1])            # exact
                M = np.maximum.reduceat(Z, d_off[full] - r0, axis=1)                  # a page's rows end where the next one with rows starts
                if c0 is not None:
                    M = np.where(c0[full][None, :], np.maximum(M, 0.0), M)
                m32 = M.astype(np.float32)
                assert np.array_equal(m32.astype(np.float64), M), "a maximum is not representable in fp32"
                M32[t0:t0 + block, full] = m32
        p0 = p1
    if clamp0 is not None:
        empty = np.flatnonzero((d_off[1:] == d_off[:-1]) & np.asarray(clamp0).astype(bool))
        M32[:, empty] = 0.0
    return M32


def scores(qc, qs, q_off, dc, ds, d_off, clamp0=None):
    """fp32 [n_q, n] in the documented order"""
    return fw.sum_tokens(maxima(qc, qs, dc, ds, d_off, clamp0), q_off, d_off)


def score_blocks(q_blocks, page_raw, d_off, clamp0=None, f16=False):
    """Scores of a host list of query blocks (raw 16-bit patterns [L_q, 320]) against the raw 16-bit rows of packed pages."""
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    qr = (np.concatenate([np.asarray(q, np.uint16).reshape(-1, DIM) for q in q_blocks]) if len(q_blocks)
          else np.zeros((0, DIM), np.uint16))
    qc, qs = encode(qr, f16)
    dc, ds = fw.encode(page_raw, f16)
    return scores(qc, qs, q_off, dc, ds, d_off, clamp0)
