"""Numpy restatement of the compressed shard at width 320 (include/maxsim.h: msim_cent_wide_*, msim_res_wide_*), independent of
colpali_amd: tests/centroid_truth.py and tests/residual_truth.py with 320 for 128.

Encode:  code[r] = argmax_k <row_r, C_k>, the lowest k on equal values (here in float64: the kernel's fp32 chain may pick any k whose
         float64 similarity is within its rounding error of the maximum -- `encode_slack`).
Table:   S[i, k] = fp16(fl32 <q_i, C_k>); a page scores sum_i max_j S[i, code_j] (tests/centroid_truth.py: scores, which depends on
         the table and the codes alone and serves both widths).
Code:    e_k = fl32(float(x_k) - float(C[c]_k)); bucket b_k = the number of cutoffs t with t <= e_k.  A row whose code is >= K gets
         all-zero buckets.
Packing: uint8 [rows, 40 * bits]; dimension k occupies bits [k * bits, k * bits + bits) of its row read as a little-endian bit string.
Decode:  xhat_k = round_to_dtype(fl32(float(C[c]_k) + weights[b_k])): one float32 addition, one rounding, no renormalisation.
"""
import numpy as np

from tests.residual_truth import from_bits, to_bits  # noqa: F401  (the dtype conversions do not depend on the width)

F32 = np.float32
W = 320


# ------------------------------------------------------------------------------------------------------------------ the centroid index
def sims64(rows, C):
    """float64 [n, K] dot products of float32-representable rows [n, 320] and centroids [K, 320]."""
    return np.asarray(rows, dtype=np.float64).reshape(-1, W) @ np.asarray(C, dtype=np.float64).reshape(-1, W).T


def abs_sims64(rows, C):
    """float64 [n]: max over the centroids j of sum_k |row_k C_jk|."""
    return (np.abs(np.asarray(rows, dtype=np.float64).reshape(-1, W)) @ np.abs(np.asarray(C, dtype=np.float64).reshape(-1, W)).T).max(axis=1)


def encode_slack(rows, C):
    """float64 [n]: 320 * 2^-23 * max_k sum |row C_k| -- two fp32 chains of 320 products, each within 320 * 2^-24 of its float64 value."""
    return W * 2.0**-23 * abs_sims64(rows, C)


def score_tolerance(q_rows, C, q_off, score64):
    """float64 [n_q, n]: sum_i (2^-12 + 320 * 2^-24 * max_k sum |q_i C_k|) + Lq * 2^-24 * |score|."""
    qo = np.asarray(q_off, dtype=np.int64)
    per_tok = 2.0**-12 + W * 2.0**-24 * abs_sims64(q_rows, C) if len(np.asarray(q_rows).reshape(-1, W)) else np.zeros(0)
    tol = np.zeros(score64.shape, dtype=np.float64)
    for q in range(len(qo) - 1):
        lq = qo[q + 1] - qo[q]
        with np.errstate(invalid="ignore"):
            tol[q] = per_tok[qo[q]:qo[q + 1]].sum() + lq * 2.0**-24 * np.where(np.isfinite(score64[q]), np.abs(score64[q]), 0.0)
    return tol


def page_maxima(S, page_codes, d_off, clamp0=None):
    """M [T, n]: max over a page's rows of S[:, code]; an empty page: -inf."""
    off = np.asarray(d_off, dtype=np.int64)
    n = len(off) - 1
    M = np.full((S.shape[0], n), -np.inf, dtype=S.dtype)
    live = np.nonzero(off[1:] > off[:-1])[0]
    if len(live) and S.shape[0]:
        G = S[:, np.asarray(page_codes[:off[-1]], dtype=np.int64)]
        M[:, live] = np.maximum.reduceat(G, off[live], axis=1)
    if clamp0 is not None:
        c = np.asarray(clamp0).astype(bool) & (off[1:] > off[:-1])
        M[:, c] = np.maximum(M[:, c], 0)
    return M


def scores64(q_rows, C, q_off, page_codes, d_off, clamp0=None):
    """float64 [n_q, n]: sum_i max_j <q_i, C_code_j> without any rounding; an empty page: -inf; a query of 0 tokens: 0."""
    off = np.asarray(d_off, dtype=np.int64)
    qo = np.asarray(q_off, dtype=np.int64)
    S = sims64(q_rows, C)
    out = np.zeros((len(qo) - 1, len(off) - 1), dtype=np.float64)
    for q in range(len(qo) - 1):
        if qo[q + 1] > qo[q]:
            out[q] = page_maxima(S[qo[q]:qo[q + 1]], page_codes, off, clamp0).sum(axis=0)
    out[:, off[1:] == off[:-1]] = -np.inf
    return out


# ------------------------------------------------------------------------------------------------------------------ the codec
def buckets(rows, C, codes, cutoffs):
    """int64 [n, 320]: the bucket of every dimension."""
    rows, C = np.asarray(rows, dtype=F32).reshape(-1, W), np.asarray(C, dtype=F32).reshape(-1, W)
    codes = np.asarray(codes).astype(np.int64)
    ok = codes < C.shape[0]
    e = rows - C[np.where(ok, codes, 0)]                       # float32 - float32: one rounding
    assert e.dtype == F32
    b = np.searchsorted(np.asarray(cutoffs, dtype=F32), e, side="right")      # the number of cutoffs <= e
    b[~ok] = 0
    return b.astype(np.int64)


def pack(b, bits):
    """uint8 [n, 40 * bits] from buckets [n, 320]."""
    b = np.asarray(b, dtype=np.int64).reshape(-1, W)
    out = np.zeros((b.shape[0], W // 8 * bits), dtype=np.uint8)
    for k in range(W):
        pos = k * bits
        out[:, pos // 8] |= ((b[:, k] & ((1 << bits) - 1)) << (pos % 8)).astype(np.uint8)      # bits divides 8: a field never straddles a byte
    return out


def unpack(res, bits):
    """int64 [n, 320] from uint8 [n, 40 * bits]."""
    res = np.asarray(res, dtype=np.uint8).reshape(-1, W // 8 * bits)
    out = np.zeros((res.shape[0], W), dtype=np.int64)
    for k in range(W):
        pos = k * bits
        out[:, k] = (res[:, pos // 8].astype(np.int64) >> (pos % 8)) & ((1 << bits) - 1)
    return out


def encode(rows, C, codes, cutoffs, bits):
    """uint8 [n, 40 * bits]: the packed residuals of `rows` under the given codes."""
    return pack(buckets(rows, C, codes, cutoffs), bits)


def decode(C, codes, res, weights, bits, dtype):
    """uint16 [n, 320]: the bit patterns of xhat; a row whose code is >= K is NaN (0x7fc0 / 0x7e00)."""
    C = np.asarray(C, dtype=F32).reshape(-1, W)
    codes = np.asarray(codes).astype(np.int64)
    ok = codes < C.shape[0]
    w = np.asarray(weights, dtype=F32)[unpack(res, bits)]
    v = C[np.where(ok, codes, 0)] + w                          # float32 + float32: one rounding
    assert v.dtype == F32
    out = to_bits(v, dtype)
    out[~ok] = 0x7E00 if dtype == "f16" else 0x7FC0
    return out


def maxsim64(q_rows, q_off, xhat, d_off, clamp0=None):
    """(score float64 [n_q, n], tolerance float64 [n_q, n]) of float32 query rows against decoded rows xhat: the float64 MaxSim, and
    the bound an fp32 chain of 320 exact products plus an fp32 token sum stays within (tests/residual_truth.py: maxsim64 with 320
    for 128):
        sum_i 320 * 2^-24 * max_j sum_k |q_ik xhat_jk|   +   Lq * 2^-24 * sum_i |M_i|.
    A page without rows scores -inf (0 under clamp0)."""
    Q = np.asarray(q_rows, dtype=np.float64).reshape(-1, W)
    X = np.asarray(xhat, dtype=np.float64).reshape(-1, W)
    qo, do = np.asarray(q_off, dtype=np.int64), np.asarray(d_off, dtype=np.int64)
    n_q, n = len(qo) - 1, len(do) - 1
    score = np.zeros((n_q, n))
    tol = np.zeros((n_q, n))
    for c in range(n):
        rows = X[do[c]:do[c + 1]]
        flag = clamp0 is not None and bool(clamp0[c])
        if len(rows):
            M = (Q @ rows.T).max(axis=1)
            A = (np.abs(Q) @ np.abs(rows).T).max(axis=1)
        else:
            M, A = np.full(len(Q), -np.inf), np.zeros(len(Q))
        if flag:
            M = np.maximum(M, 0.0)
        for q in range(n_q):
            m = M[qo[q]:qo[q + 1]]
            score[q, c] = m.sum()
            lq = qo[q + 1] - qo[q]
            with np.errstate(invalid="ignore"):
                tol[q, c] = W * 2.0**-24 * A[qo[q]:qo[q + 1]].sum() + lq * 2.0**-24 * np.abs(np.where(np.isfinite(m), m, 0.0)).sum()
    return score, tol
