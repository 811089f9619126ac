"""Numpy restatement of e2m3 (FP6) query tokens against the FP4 index (include/maxsim.h: msim_f6_encode_rows, msim_f4_scores_q6),
independent of colpali_amd.  The page side is tests/fp4_truth.py.

Query row code, on the stored bf16 / f16 values: a = max |x_k|; a == 0: every field 0, scale byte 127; otherwise e = the smallest
integer with a <= 7.5 * 2^e, clamped to [-32, 32]; y_k = min(|x_k| * 2^-e, 7.5); the code is the nearest of the 32 e2m3 magnitudes
(codes 0 .. 7: i/8; code 8 (j + 1) + i: (1 + i/8) * 2^j, j = 0 .. 2), a tie going to the even code; field = sign << 5 | code (0 when
the code is 0); scale byte = e + 127.  A token is 96 code bytes: dimension k is the 6-bit field at bit 6 (k mod 32) of the
little-endian 24-byte group k // 32.  NaN elements are unspecified.
Score: I_ij = sum_k v(q_ik) v(d_jk) (a multiple of 1/16, |I| <= 5760); Z_ij = I_ij * 2^(eq_i + ed_j); M_ic = max_j Z_ij over a page's
rows, max(M_ic, 0) under clamp0; score = the sequential float32 sum of M_ic in token order.  A page of 0 rows scores -inf.
Everything up to M is computed in float64, where it is exact, and every M is asserted to be a float32.
"""
import numpy as np

from tests import fp4_truth as ft

GRID = np.array([i / 8 for i in range(8)] + [(1 + i / 8) * 2.0 ** j for j in range(3) for i in range(8)])     # code -> magnitude
E_MIN, E_MAX = ft.E_MIN, ft.E_MAX
raw_bits, values = ft.raw_bits, ft.values


def row_exponents(x):
    """int64 [n]: e of every row of x float64 [n, 128] (0 for a zero row): the smallest integer with max |x| <= 7.5 * 2^e, clamped"""
    a = np.abs(x).max(axis=1) if x.shape[0] else np.zeros(0)
    f, p = np.frexp(a)                                   # a = f * 2^p, 0.5 <= f < 1, exact; 7.5 * 2^e = 0.9375 * 2^(e + 3)
    e = np.where(f <= 0.9375, p - 3, p - 2).astype(np.int64)
    e = np.clip(e, E_MIN, E_MAX)
    return np.where(a == 0, 0, e)


def nearest_codes(y):
    """int64 codes 0 .. 31 of y float64 in [0, 7.5]: the nearest grid value, a tie to the even code"""
    lo = np.clip(np.searchsorted(GRID, y, side="right") - 1, 0, 31)
    hi = np.minimum(lo + 1, 31)
    dl, dh = y - GRID[lo], GRID[hi] - y
    up = (hi > lo) & ((dh < dl) | ((dh == dl) & (hi % 2 == 0)))
    return np.where(up, hi, lo).astype(np.int64)


def pack_fields(fields):
    """codes uint8 [n, 96] of 6-bit fields [n, 128]: field k at bit 6 (k mod 32) of the little-endian 24-byte group k // 32"""
    f = np.asarray(fields, dtype=np.uint8).reshape(-1, 4, 32)
    assert (f < 64).all()
    bits = (f[..., None] >> np.arange(6, dtype=np.uint8)) & 1                       # [n, 4, 32, 6]: bit b of field j is bit 6 j + b
    return np.packbits(bits.reshape(-1, 4, 192), axis=-1, bitorder="little").reshape(-1, 96)


def unpack_fields(codes):
    """6-bit fields uint8 [n, 128] of codes uint8 [n, 96]"""
    c = np.asarray(codes, dtype=np.uint8).reshape(-1, 4, 24)
    bits = np.unpackbits(c, axis=-1, bitorder="little").reshape(-1, 4, 32, 6)
    return (bits << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8).reshape(-1, 128)


def encode_values(x):
    """(codes uint8 [n, 96], scales uint8 [n]) of x float64 [n, 128] (values a bf16 / f16 tensor stores)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 128)
    e = row_exponents(x)
    y = np.minimum(np.ldexp(np.abs(x), -e[:, None]), 7.5)
    code = nearest_codes(y)
    field = np.where(code > 0, code | (np.signbit(x).astype(np.int64) << 5), 0).astype(np.uint8)
    return pack_fields(field), (e + 127).astype(np.uint8)


def encode(raw16, f16=False):
    """(codes, scales) of the raw 16-bit patterns of bf16 / f16 query tokens"""
    return encode_values(values(raw16, f16))


def decode(codes):
    """float64 [n, 128]: the grid values (with sign) of codes uint8 [n, 96]"""
    f = unpack_fields(codes)
    return np.where(f >> 5, -1.0, 1.0) * GRID[f & 31]


def maxima(qc, qs, dc, ds, d_off, clamp0=None, block=64):
    """float32 [T, n]: M_ic of e2m3 tokens (qc [T, 96], qs [T]) against FP4 pages (dc [R, 64], ds [R], offsets d_off); -inf for a
    page of 0 rows (0 under clamp0).  Asserts that every maximum is a float32."""
    d_off = np.asarray(d_off, dtype=np.int64)
    n, T = len(d_off) - 1, len(qs)
    vq, vd = decode(qc), ft.decode(dc)
    eq, ed = np.asarray(qs, dtype=np.int64) - 127, np.asarray(ds, dtype=np.int64) - 127
    M32 = np.full((T, n), -np.inf, dtype=np.float32)
    full = np.flatnonzero(d_off[1:] > d_off[:-1])
    c0 = None if clamp0 is None else np.asarray(clamp0).astype(bool)[full]
    for t0 in range(0, T, block):
        if not len(full):
            break
        I = vq[t0:t0 + block] @ vd.T                                              # multiples of 1/16 below 2^13: exact
        Z = np.ldexp(I, eq[t0:t0 + block, None] + ed[None, :])                    # exact
        M = np.maximum.reduceat(Z, d_off[full], axis=1)                           # a page's rows end where the next one with rows starts
        if c0 is not None:
            M = np.where(c0[None, :], np.maximum(M, 0.0), M)
        m32 = M.astype(np.float32)
        assert np.array_equal(m32.astype(np.float64), M), "a maximum is not representable in fp32"
        M32[t0:t0 + block, full] = m32
    if clamp0 is not None:
        empty = np.flatnonzero((d_off[1:] == d_off[:-1]) & np.asarray(clamp0).astype(bool))
        M32[:, empty] = 0.0
    return M32


def scores(qc, qs, q_off, dc, ds, d_off, clamp0=None):
    """fp32 [n_q, n] in the documented order"""
    d_off = np.asarray(d_off, dtype=np.int64)
    n, n_q = len(d_off) - 1, len(q_off) - 1
    M = maxima(qc, qs, dc, ds, d_off, clamp0)
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
    """Scores of a host list of query blocks (raw 16-bit patterns [L_q, 128]) against the raw 16-bit rows of packed pages."""
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    qr = (np.concatenate([np.asarray(q, np.uint16).reshape(-1, 128) for q in q_blocks]) if len(q_blocks)
          else np.zeros((0, 128), np.uint16))
    qc, qs = encode(qr, f16)
    dc, ds = ft.encode(page_raw, f16)
    return scores(qc, qs, q_off, dc, ds, d_off, clamp0)
