"""Numpy restatement of the int8 token-level index (include/maxsim.h: msim_i8_*), independent of colpali_amd.

Quantization, in float32 on the bf16 / f16 values: a = max |x| (a page's rows, or one query token row), inv = float32(127) / a,
code = 0 where x == 0, else clip(rint(x * inv), -127, 127) (rint: half to even); scale = a / float32(127).  a == 0: codes 0, scale 0.
Score: I = q8 . d8^T exactly; M_i = max_j I_ij, max(M_i, 0) under clamp0; T = the sequential float32 sum in token order of
float32(M_i) * sq_i; score = float32(sd * T).  A page of 0 rows scores -inf.
"""
import numpy as np

F32 = np.float32


def quantize(X):
    """codes int8 [n, 128] and the scale (float32) of one block of rows X (float32-representable values)."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 128)
    a = np.abs(X).max() if X.size else F32(0)
    a = F32(a)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F32(127) / a
        p = (X * inv).astype(np.float32)
    c = np.clip(np.rint(p), -127, 127)
    c = np.where(X == 0, 0, c)
    return c.astype(np.int8), F32(a / F32(127))


def quantize_pages(rows, offsets):
    """codes [rows, 128] and scales [n] of packed pages."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 128)
    off = np.asarray(offsets, dtype=np.int64)
    codes = np.zeros(rows.shape, dtype=np.int8)
    scales = np.zeros(len(off) - 1, dtype=np.float32)
    for i in range(len(off) - 1):
        codes[off[i]:off[i + 1]], scales[i] = quantize(rows[off[i]:off[i + 1]])
    return codes, scales


def quantize_tokens(rows):
    """per-row codes [T, 128] and scales [T]."""
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 128)
    codes = np.zeros(rows.shape, dtype=np.int8)
    scales = np.zeros(rows.shape[0], dtype=np.float32)
    for i in range(rows.shape[0]):
        codes[i], scales[i] = quantize(rows[i:i + 1])
    return codes, scales


def maxima(q8, d8, d_off, clamp0=None):
    """M int64 [T, n] of token codes q8 [T, 128] against packed page codes; an empty page: the int64 minimum."""
    off = np.asarray(d_off, dtype=np.int64)
    n = len(off) - 1
    I = q8.astype(np.int64) @ d8.astype(np.int64).T if q8.shape[0] and d8.shape[0] else np.zeros((q8.shape[0], d8.shape[0]), np.int64)
    M = np.full((q8.shape[0], n), np.iinfo(np.int64).min, dtype=np.int64)
    for c in range(n):
        if off[c + 1] > off[c]:
            M[:, c] = I[:, off[c]:off[c + 1]].max(axis=1)
            if clamp0 is not None and clamp0[c]:
                M[:, c] = np.maximum(M[:, c], 0)
    return M


def scores(q8, sq, q_off, d8, sd, d_off, clamp0=None):
    """fp32 [n_q, n] in the documented order."""
    M = maxima(q8, d8, d_off, clamp0)
    qo = np.asarray(q_off, dtype=np.int64)
    do = np.asarray(d_off, dtype=np.int64)
    n = len(do) - 1
    empty = do[1:] == do[:-1]
    out = np.zeros((len(qo) - 1, n), dtype=np.float32)
    Mf = np.where(M == np.iinfo(np.int64).min, 0, M).astype(np.float32)
    for q in range(len(qo) - 1):
        a, b = qo[q], qo[q + 1]
        T = np.zeros(n, dtype=np.float32)
        for i in range(a, b):                       # sequential, in token order
            T = (T + (Mf[i] * sq[i]).astype(np.float32)).astype(np.float32)
        out[q] = (sd.astype(np.float32) * T).astype(np.float32)
    out[:, empty] = -np.inf
    return out


def score_blocks(q_blocks, page_blocks, clamp0=None):
    """Scores of host lists of float32 query [L_q, 128] and page [n_c, 128] blocks, quantized here."""
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    d_off = np.cumsum([0] + [len(p) for p in page_blocks])
    qr = np.concatenate([np.asarray(q, np.float32).reshape(-1, 128) for q in q_blocks]) if len(q_blocks) else np.zeros((0, 128), np.float32)
    dr = np.concatenate([np.asarray(p, np.float32).reshape(-1, 128) for p in page_blocks])
    q8, sq = quantize_tokens(qr)
    d8, sd = quantize_pages(dr, d_off)
    return scores(q8, sq, q_off, d8, sd, d_off, clamp0)


def scores_fast(q8, sq, q_off, d8, sd, d_off, clamp0=None, token_block=64):
    """`scores` for large page counts, in the same order: the exact maxima from float32 products (every partial sum is an integer
    below 2^24, so exact in any order) folded per page by maximum.reduceat, then the same sequential float32 token sum."""
    do = np.asarray(d_off, dtype=np.int64)
    qo = np.asarray(q_off, dtype=np.int64)
    n = len(do) - 1
    lens = do[1:] - do[:-1]
    live = np.nonzero(lens > 0)[0]
    D = d8[:do[-1]].astype(np.float32)
    M = np.zeros((q8.shape[0], n), dtype=np.int64)
    for t0 in range(0, q8.shape[0], token_block):
        I = q8[t0:t0 + token_block].astype(np.float32) @ D.T
        if len(live):
            M[t0:t0 + token_block, live] = np.maximum.reduceat(I, do[live], axis=1).astype(np.int64)
    if clamp0 is not None:
        c = np.asarray(clamp0).astype(bool)
        M[:, c] = np.maximum(M[:, c], 0)
    Mf = M.astype(np.float32)
    out = np.zeros((len(qo) - 1, n), dtype=np.float32)
    for q in range(len(qo) - 1):
        T = np.zeros(n, dtype=np.float32)
        for i in range(qo[q], qo[q + 1]):
            T = (T + (Mf[i] * sq[i]).astype(np.float32)).astype(np.float32)
        out[q] = (sd.astype(np.float32) * T).astype(np.float32)
    out[:, lens == 0] = -np.inf
    return out
