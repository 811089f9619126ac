"""Numpy restatement of the FP4 index (include/maxsim.h: msim_f4_*), independent of colpali_amd.

Row code (pages and query tokens alike), on the stored bf16 / f16 values: a = max |x_k|; a == 0: nibbles 0, scale byte 127; otherwise
e = the smallest integer with a <= 6 * 2^e, clamped to [-32, 32]; y_k = min(|x_k| * 2^-e, 6); the code is the nearest of
{0, 0.5, 1, 1.5, 2, 3, 4, 6}, a tie going to the even code; nibble = sign << 3 | code (0 when the code is 0); dimension k is nibble
(k & 1) of byte (k >> 1), the low nibble the even k; scale byte = e + 127.  NaN elements are unspecified.
Score: I_ij = sum_k v(q_ik) v(d_jk); Z_ij = I_ij * 2^(eq_i + ed_j); M_ic = max_j Z_ij over a page's rows, max(M_ic, 0) under clamp0;
score = the sequential float32 sum of M_ic in token order.  A page of 0 rows scores -inf.  Everything up to M is computed in float64,
where it is exact, and every M is asserted to be a float32.
"""
import numpy as np

GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
E_MIN, E_MAX = -32, 32


def raw_bits(t):
    """the stored 16-bit patterns (uint16 numpy) of a bf16 / f16 torch tensor [n, 128]"""
    import torch

    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def values(raw16, f16=False):
    """float64 [n, 128]: the values the raw 16-bit patterns uint16 [n, 128] store (bf16, or f16 with f16=True)"""
    raw16 = np.ascontiguousarray(np.asarray(raw16, dtype=np.uint16).reshape(-1, 128))
    if f16:
        return raw16.view(np.float16).astype(np.float64)
    return (raw16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def row_exponents(x):
    """int64 [n]: e of every row of x float64 [n, 128] (0 for a zero row): the smallest integer with max |x| <= 6 * 2^e, clamped"""
    a = np.abs(x).max(axis=1) if x.shape[0] else np.zeros(0)
    f, p = np.frexp(a)                                   # a = f * 2^p, 0.5 <= f < 1, exact; 6 * 2^e = 0.75 * 2^(e + 3)
    e = np.where(f <= 0.75, p - 3, p - 2).astype(np.int64)
    e = np.clip(e, E_MIN, E_MAX)
    return np.where(a == 0, 0, e)


def nearest_codes(y):
    """int64 codes 0 .. 7 of y float64 in [0, 6]: the nearest grid value, a tie to the even code"""
    lo = np.clip(np.searchsorted(GRID, y, side="right") - 1, 0, 7)
    hi = np.minimum(lo + 1, 7)
    dl, dh = y - GRID[lo], GRID[hi] - y
    up = (hi > lo) & ((dh < dl) | ((dh == dl) & (hi % 2 == 0)))
    return np.where(up, hi, lo).astype(np.int64)


def encode_values(x):
    """(codes uint8 [n, 64], scales uint8 [n]) of x float64 [n, 128] (values a bf16 / f16 tensor stores)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 128)
    e = row_exponents(x)
    y = np.minimum(np.ldexp(np.abs(x), -e[:, None]), 6.0)
    code = nearest_codes(y)
    nib = np.where(code > 0, code | (np.signbit(x).astype(np.int64) << 3), 0).astype(np.uint8)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8), (e + 127).astype(np.uint8)


def encode(raw16, f16=False):
    """(codes, scales) of the raw 16-bit patterns of a bf16 / f16 blob"""
    return encode_values(values(raw16, f16))


def pack_nibbles(nib):
    """codes uint8 [n, 64] of nibbles [n, 128]"""
    nib = np.asarray(nib, dtype=np.uint8).reshape(-1, 128)
    return (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8)


def decode(codes):
    """float64 [n, 128]: the grid values (with sign) of codes uint8 [n, 64]"""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, 64)
    nib = np.empty((codes.shape[0], 128), dtype=np.uint8)
    nib[:, 0::2], nib[:, 1::2] = codes & 0xF, codes >> 4
    return np.where(nib >> 3, -1.0, 1.0) * GRID[nib & 7]


def maxima(qc, qs, dc, ds, d_off, clamp0=None, block=64):
    """float32 [T, n]: M_ic of coded tokens (qc [T, 64], qs [T]) against coded pages (dc [R, 64], ds [R], offsets d_off); -inf for a
    page of 0 rows (0 under clamp0).  Asserts that every maximum is a float32."""
    d_off = np.asarray(d_off, dtype=np.int64)
    n, T = len(d_off) - 1, len(qs)
    vq, vd = decode(qc), decode(dc)
    eq, ed = np.asarray(qs, dtype=np.int64) - 127, np.asarray(ds, dtype=np.int64) - 127
    M32 = np.full((T, n), -np.inf, dtype=np.float32)
    full = np.flatnonzero(d_off[1:] > d_off[:-1])
    c0 = None if clamp0 is None else np.asarray(clamp0).astype(bool)[full]
    for t0 in range(0, T, block):
        if not len(full):
            break
        I = vq[t0:t0 + block] @ vd.T                                              # multiples of 1/4 below 2^13: exact
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
    dc, ds = encode(page_raw, f16)
    return scores(qc, qs, q_off, dc, ds, d_off, clamp0)
