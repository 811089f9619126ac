"""Numpy restatement of the residual codec (include/maxsim.h: msim_res_*), independent of colpali_amd.

Code:    e_k = fl32(float(x_k) - float(C[c]_k)) -- one float32 subtraction; bucket b_k = the number of cutoffs t with t <= e_k, so a
         value equal to a cutoff goes to the upper bucket.  A row whose code is >= K gets all-zero buckets.
Packing: uint8 [rows, 16 * bits]; dimension k occupies bits [k * bits, k * bits + bits) of its row read as a little-endian bit string
         (bit i of the row = bit i % 8 of byte i // 8).
Decode:  xhat_k = round_to_dtype(fl32(float(C[c]_k) + weights[b_k])): one float32 addition, one rounding to nearest even to bfloat16 /
         float16, no renormalisation.  Rows travel as float32 arrays of dtype-representable values, or as their uint16 bit patterns.
"""
import numpy as np

F32 = np.float32


def to_bits(x32, dtype):
    """uint16 bit patterns of float32 values rounded to nearest even to `dtype` ("bf16" | "f16")."""
    x32 = np.ascontiguousarray(x32, dtype=F32)
    if dtype == "f16":
        return x32.astype(np.float16).view(np.uint16)
    u = x32.view(np.uint32)
    return ((u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)).astype(np.uint16)


def from_bits(bits, dtype):
    """float32 values of uint16 bit patterns."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == "f16":
        return bits.view(np.float16).astype(F32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(F32)


def buckets(rows, C, codes, cutoffs):
    """int64 [n, 128]: the bucket of every dimension; rows float32 [n, 128], C float32 [K, 128], codes [n], cutoffs float32."""
    rows, C = np.asarray(rows, dtype=F32).reshape(-1, 128), np.asarray(C, dtype=F32).reshape(-1, 128)
    codes = np.asarray(codes).astype(np.int64)
    ok = codes < C.shape[0]
    e = rows - C[np.where(ok, codes, 0)]                       # float32 - float32: one rounding
    assert e.dtype == F32
    b = np.searchsorted(np.asarray(cutoffs, dtype=F32), e, side="right")      # the number of cutoffs <= e
    b[~ok] = 0
    return b.astype(np.int64)


def pack(b, bits):
    """uint8 [n, 16 * bits] from buckets [n, 128]."""
    b = np.asarray(b, dtype=np.int64).reshape(-1, 128)
    out = np.zeros((b.shape[0], 16 * bits), dtype=np.uint8)
    for k in range(128):
        pos = k * bits
        out[:, pos // 8] |= ((b[:, k] & ((1 << bits) - 1)) << (pos % 8)).astype(np.uint8)      # bits divides 8: a field never straddles a byte
    return out


def unpack(res, bits):
    """int64 [n, 128] from uint8 [n, 16 * bits]."""
    res = np.asarray(res, dtype=np.uint8).reshape(-1, 16 * bits)
    out = np.zeros((res.shape[0], 128), dtype=np.int64)
    for k in range(128):
        pos = k * bits
        out[:, k] = (res[:, pos // 8].astype(np.int64) >> (pos % 8)) & ((1 << bits) - 1)
    return out


def encode(rows, C, codes, cutoffs, bits):
    """uint8 [n, 16 * bits]: the packed residuals of `rows` under the given codes."""
    return pack(buckets(rows, C, codes, cutoffs), bits)


def decode(C, codes, res, weights, bits, dtype):
    """uint16 [n, 128]: the bit patterns of xhat; a row whose code is >= K is NaN (0x7fc0 / 0x7e00)."""
    C = np.asarray(C, dtype=F32).reshape(-1, 128)
    codes = np.asarray(codes).astype(np.int64)
    ok = codes < C.shape[0]
    w = np.asarray(weights, dtype=F32)[unpack(res, bits)]
    v = C[np.where(ok, codes, 0)] + w                          # float32 + float32: one rounding
    assert v.dtype == F32
    out = to_bits(v, dtype)
    out[~ok] = 0x7E00 if dtype == "f16" else 0x7FC0
    return out


def maxsim64(q_rows, q_off, xhat, d_off, clamp0=None):
    """(score float64 [n_q, n], tolerance float64 [n_q, n]) of float32 query rows against decoded rows xhat (float32): the float64
    MaxSim, and the bound an fp32 chain of 128 exact products plus an fp32 token sum stays within:
        sum_i 128 * 2^-24 * max_j sum_k |q_ik xhat_jk|   +   Lq * 2^-24 * sum_i |M_i|.
    A page without rows scores -inf (0 under clamp0)."""
    Q = np.asarray(q_rows, dtype=np.float64).reshape(-1, 128)
    X = np.asarray(xhat, dtype=np.float64).reshape(-1, 128)
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
                tol[q, c] = 128 * 2.0**-24 * A[qo[q]:qo[q + 1]].sum() + lq * 2.0**-24 * np.abs(np.where(np.isfinite(m), m, 0.0)).sum()
    return score, tol
