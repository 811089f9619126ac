"""Numpy restatement of the centroid-code index (include/maxsim.h: msim_cent_*), independent of colpali_amd.

Encode: code[r] = argmax_k <row_r, C_k>, the lowest k on equal values (here in float64: the kernel's fp32 chain may pick any k
whose float64 similarity is within its rounding error of the maximum -- `encode_slack`).
Table:  S[i, k] = fp16(fl32 <q_i, C_k>).
Score:  M_i = max_j S[i, code_j] over the page's rows (an exact max of fp16 values), max(M_i, 0) under clamp0; score = the
        sequential float32 sum in token order of float32(M_i).  A page of 0 rows scores -inf; a code >= K makes its page NaN.
"""
import numpy as np

F32 = np.float32


def sims64(rows, C):
    """float64 [n, K] dot products of float32-representable rows [n, 128] and centroids [K, 128]."""
    return np.asarray(rows, dtype=np.float64).reshape(-1, 128) @ np.asarray(C, dtype=np.float64).reshape(-1, 128).T


def abs_sims64(rows, C):
    """float64 [n]: max over the centroids j of sum_k |row_k C_jk|, the scale of the encode slack."""
    return (np.abs(np.asarray(rows, dtype=np.float64).reshape(-1, 128)) @ np.abs(np.asarray(C, dtype=np.float64).reshape(-1, 128)).T).max(axis=1)


def codes(rows, C):
    """uint16 [n]: the float64 argmax, lowest k first."""
    return np.argmax(sims64(rows, C), axis=1).astype(np.uint16)


def encode_slack(rows, C):
    """float64 [n]: how far below the float64 maximum a stored code's similarity may lie: 128 * 2^-23 * sum_k |row_k C_k| (two fp32
    chains of 128 products, each within 128 * 2^-24 of its float64 value; the sum taken at the centroid where it is largest)."""
    return 128 * 2.0**-23 * abs_sims64(rows, C)


def table(q_rows, C):
    """fp16 [T, K]: the float64 dot product rounded to float32, then to float16."""
    return sims64(q_rows, C).astype(np.float32).astype(np.float16)


def page_maxima(S, page_codes, d_off, clamp0=None):
    """M [T, n] in S's dtype; an empty page: -inf (before clamp0 as after: an empty page scores -inf anyway)."""
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


def scores(S16, q_off, page_codes, d_off, clamp0=None):
    """float32 [n_q, n] in the documented order from the fp16 table S16 [T, K]."""
    S16 = np.asarray(S16, dtype=np.float16)
    K = S16.shape[1]
    off = np.asarray(d_off, dtype=np.int64)
    qo = np.asarray(q_off, dtype=np.int64)
    n = len(off) - 1
    pc = np.asarray(page_codes[:off[-1]], dtype=np.int64)
    broken = np.zeros(n, dtype=bool)
    for c in range(n):
        broken[c] = bool((pc[off[c]:off[c + 1]] >= K).any())
    M = page_maxima(S16, np.where(pc >= K, 0, pc), off, clamp0).astype(np.float32)
    out = np.zeros((len(qo) - 1, n), dtype=np.float32)
    with np.errstate(invalid="ignore"):
        for q in range(len(qo) - 1):
            T = np.zeros(n, dtype=np.float32)
            for i in range(qo[q], qo[q + 1]):                # sequential, in token order
                T = (T + M[i]).astype(np.float32)
            out[q] = T
    out[:, off[1:] == off[:-1]] = -np.inf
    out[:, broken] = np.nan
    return out


def scores64(q_rows, C, q_off, page_codes, d_off, clamp0=None):
    """float64 [n_q, n]: sum_i max_j <q_i, C_code_j> without any rounding; an empty page: -inf."""
    off = np.asarray(d_off, dtype=np.int64)
    qo = np.asarray(q_off, dtype=np.int64)
    S = sims64(q_rows, C)
    out = np.zeros((len(qo) - 1, len(off) - 1), dtype=np.float64)
    for q in range(len(qo) - 1):                             # one query at a time: the gathered table is [tokens, rows]
        if qo[q + 1] > qo[q]:
            out[q] = page_maxima(S[qo[q]:qo[q + 1]], page_codes, off, clamp0).sum(axis=0)
    out[:, off[1:] == off[:-1]] = -np.inf
    return out


def score_tolerance(q_rows, C, q_off, score64):
    """float64 [n_q, n]: sum_i (2^-12 + 128 * 2^-24 * sum_k |q_ik C_k|) + Lq * 2^-24 * |score|; 2^-12 is the fp16 half-ulp below 1,
    the middle term the fp32 chain's error read as sum_k |q_ik| |C_jk| maximised over the centroids j a page can name."""
    qo = np.asarray(q_off, dtype=np.int64)
    per_tok = 2.0**-12 + 128 * 2.0**-24 * (np.abs(np.asarray(q_rows, np.float64).reshape(-1, 128))
                                          @ np.abs(np.asarray(C, np.float64).reshape(-1, 128)).T).max(axis=1)
    tol = np.zeros(score64.shape, dtype=np.float64)
    for q in range(len(qo) - 1):
        lq = qo[q + 1] - qo[q]
        with np.errstate(invalid="ignore"):
            tol[q] = per_tok[qo[q]:qo[q + 1]].sum() + lq * 2.0**-24 * np.where(np.isfinite(score64[q]), np.abs(score64[q]), 0.0)
    return tol
