"""Numpy restatement of the FP4 index at width 320 (include/maxsim.h: msim_f4w_*), independent of colpali_amd.

Row code (pages and query tokens alike), on the stored bf16 / f16 values: msim_f4_encode_rows' rule over 320 dimensions with ONE
scale per row.  a = max over all 320 |x_k|; a == 0: nibbles 0, scale byte 127; otherwise e = the smallest integer with
a <= 6 * 2^e, clamped to [-32, 32]; y_k = min(|x_k| * 2^-e, 6); the code is the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, a tie going
to the even code; nibble = sign << 3 | code (0 when the code is 0); dimension k is nibble (k & 1) of byte (k >> 1) of a 160-byte
row, the low nibble the even k; scale byte = e + 127.  NaN elements are unspecified.
Score: I_ij = sum_{k<320} v(q_ik) v(d_jk) (a multiple of 1/4 with |I| <= 11 520); Z_ij = I_ij * 2^(eq_i + ed_j); M_ic = max_j Z_ij
over a page's rows, max(M_ic, 0) under clamp0; score = the sequential float32 sum of M_ic in token order.  A page of 0 rows scores
-inf.  Everything up to M is computed in float64, where it is exact, and every M is asserted to be a float32.

The grid is that of tests/fp4_truth.py and is taken from there.  The rounding rule is restated by the grid's midpoints (a row is 2 1/2
times as long and the large cases of the GPU tests code a quarter of a million rows): `codes_of` is asserted equal to
fp4_truth.nearest_codes, the search for the nearest grid value, in tests/test_fp4_wide_host.py.
"""
import numpy as np

from tests.fp4_truth import E_MAX, E_MIN, GRID

MIDS = (GRID[:-1] + GRID[1:]) / 2                       # 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0: midpoint i lies between codes i and i + 1

DIM = 320
ROW_BYTES = DIM // 2


def raw_bits(t):
    """the stored 16-bit patterns (uint16 numpy) of a bf16 / f16 torch tensor [n, 320]"""
    import torch

    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def values(raw16, f16=False):
    """float64 [n, 320]: the values the raw 16-bit patterns uint16 [n, 320] store (bf16, or f16 with f16=True)"""
    raw16 = np.ascontiguousarray(np.asarray(raw16, dtype=np.uint16).reshape(-1, DIM))
    if f16:
        return raw16.view(np.float16).astype(np.float64)
    return (raw16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def row_exponents(x):
    """int64 [n]: e of every row of x float64 [n, 320] (0 for a zero row): the smallest integer with max |x| <= 6 * 2^e, clamped"""
    a = np.abs(x).max(axis=1) if x.shape[0] else np.zeros(0)
    f, p = np.frexp(a)                                   # a = f * 2^p, 0.5 <= f < 1, exact; 6 * 2^e = 0.75 * 2^(e + 3)
    e = np.where(f <= 0.75, p - 3, p - 2).astype(np.int64)
    e = np.clip(e, E_MIN, E_MAX)
    return np.where(a == 0, 0, e)


def codes_of(y):
    """int8 codes 0 .. 7 of y float64 in [0, 6]: the nearest grid value, a tie to the even code -- y passes midpoint i to code i + 1
    when it is above it, or on it with i + 1 even"""
    code = np.zeros(np.shape(y), dtype=np.int8)
    for i, m in enumerate(MIDS):
        code += (y >= m) if (i + 1) % 2 == 0 else (y > m)
    return code


def pack_nibbles(nib):
    """codes uint8 [n, 160] of nibbles [n, 320]"""
    nib = np.asarray(nib, dtype=np.uint8).reshape(-1, DIM)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def unpack_nibbles(codes):
    """nibbles uint8 [n, 320] of codes uint8 [n, 160]"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, ROW_BYTES)
    nib = np.empty((codes.shape[0], DIM), dtype=np.uint8)
    nib[:, 0::2], nib[:, 1::2] = codes & 0xF, codes >> 4
    return nib


def encode_values(x):
    """(codes uint8 [n, 160], scales uint8 [n]) of x float64 [n, 320] (values a bf16 / f16 tensor stores)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, DIM)
    e = row_exponents(x)
    y = np.minimum(np.ldexp(np.abs(x), -e[:, None]), 6.0)
    code = codes_of(y).astype(np.int64)
    nib = np.where(code > 0, code | (np.signbit(x).astype(np.int64) << 3), 0).astype(np.uint8)
    return pack_nibbles(nib), (e + 127).astype(np.uint8)


def encode(raw16, f16=False):
    """(codes, scales) of the raw 16-bit patterns of a bf16 / f16 blob"""
    return encode_values(values(raw16, f16))


_NIBBLE_VALUES = np.where(np.arange(16) >> 3, -1.0, 1.0) * GRID[np.arange(16) & 7]
_BYTE_VALUES = np.stack([_NIBBLE_VALUES[np.arange(256) & 0xF], _NIBBLE_VALUES[np.arange(256) >> 4]], axis=1)   # [256, 2]: even k, odd k


def decode(codes):
    """float64 [n, 320]: the grid values (with sign) of codes uint8 [n, 160]"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, ROW_BYTES)
    return _BYTE_VALUES[codes].reshape(codes.shape[0], DIM)


def maxima(qc, qs, dc, ds, d_off, clamp0=None, block=64, row_block=1 << 16):
    """float32 [T, n]: M_ic of coded tokens (qc [T, 160], qs [T]) against coded pages (dc [R, 160], ds [R], offsets d_off); -inf for
    a page of 0 rows (0 under clamp0).  Asserts that every maximum is a float32.  The pages are decoded `row_block` rows at a
    time (whole pages), so a large index never stands decoded as a whole."""
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
            vd = decode(dc[r0:r1])
            for t0 in range(0, T, block):
                I = vq[t0:t0 + block] @ vd.T                                          # multiples of 1/4 below 2^14: exact
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
    return sum_tokens(maxima(qc, qs, dc, ds, d_off, clamp0), q_off, d_off)


def sum_tokens(M, q_off, d_off):
    """fp32 [n_q, n]: the sequential float32 sum in token order of the maxima M [T, n] (`maxima`); -inf for a page of 0 rows"""
    d_off = np.asarray(d_off, dtype=np.int64)
    n, n_q = len(d_off) - 1, len(q_off) - 1
    out = np.zeros((n_q, n), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for i in range(n_q):
            t = np.zeros(n, dtype=np.float32)
            for k in range(int(q_off[i]), int(q_off[i + 1])):
                t = (t + M[k]).astype(np.float32)
            out[i] = t
    out[:, d_off[1:] == d_off[:-1]] = -np.inf
    return out


def score_blocks(q_blocks, page_raw, d_off, clamp0=None, f16=False):
    """Scores of a host list of query blocks (raw 16-bit patterns [L_q, 320]) against the raw 16-bit rows of packed pages."""
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    qr = (np.concatenate([np.asarray(q, np.uint16).reshape(-1, DIM) for q in q_blocks]) if len(q_blocks)
          else np.zeros((0, DIM), np.uint16))
    qc, qs = encode(qr, f16)
    dc, ds = encode(page_raw, f16)
    return scores(qc, qs, q_off, dc, ds, d_off, clamp0)
