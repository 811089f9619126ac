"""Numpy restatement of the 1-bit sign index (include/maxsim.h: msim_bin_*), independent of colpali_amd.

Encode: s_k = -1 where the sign bit of the stored 16-bit element (bf16 or f16) is set -- -0.0 and negative NaNs included -- and +1
otherwise; a row is 16 bytes, dimension k is bit (k & 7) of byte (k >> 3), a set bit means +1.
Score: I = q8 . s^T exactly (the queries quantized by tests/int8_truth.py: quantize_tokens); M_i = max_j I_ij over a page's rows,
max(M_i, 0) under clamp0; score = the sequential float32 sum in token order of float32(M_i) * sq_i.  A page of 0 rows scores -inf.
"""
import numpy as np

from tests import int8_truth as it


def sign_bits(raw16):
    """+-1 int8 [n, 128] of the raw 16-bit patterns uint16 [n, 128] (bf16 or f16: the sign is bit 15 of both)."""
    raw16 = np.asarray(raw16, dtype=np.uint16).reshape(-1, 128)
    return np.where(raw16 >> 15, -1, 1).astype(np.int8)


def pack(signs):
    """codes uint8 [n, 16] of +-1 rows [n, 128]: dimension k is bit (k & 7) of byte (k >> 3), set = +1."""
    signs = np.asarray(signs).reshape(-1, 128)
    return np.packbits(signs > 0, axis=1, bitorder="little")


def unpack(codes):
    """+-1 int8 [n, 128] of codes uint8 [n, 16]."""
    codes = np.asarray(codes, dtype=np.uint8).reshape(-1, 16)
    return (np.unpackbits(codes, axis=1, bitorder="little").astype(np.int8) * 2 - 1).astype(np.int8)


def encode(raw16):
    """codes uint8 [n, 16] of the raw 16-bit patterns of a bf16 / f16 blob."""
    return pack(sign_bits(raw16))


def raw_bits(t):
    """the stored 16-bit patterns (uint16 numpy) of a bf16 / f16 torch tensor [n, 128]"""
    import torch

    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def scores(q8, sq, q_off, codes, d_off, clamp0=None):
    """fp32 [n_q, n] in the documented order: the int8 truth's maxima and token sum over the +-1 rows, every page scale 1."""
    n = len(d_off) - 1
    return it.scores_fast(q8, sq, q_off, unpack(codes), np.ones(n, dtype=np.float32), d_off, clamp0)


def score_blocks(q_blocks, page_raw, d_off, clamp0=None):
    """Scores of a host list of float32 query blocks [L_q, 128] (quantized here) against the raw 16-bit rows of packed pages."""
    q_off = np.cumsum([0] + [len(q) for q in q_blocks])
    qr = (np.concatenate([np.asarray(q, np.float32).reshape(-1, 128) for q in q_blocks]) if len(q_blocks)
          else np.zeros((0, 128), np.float32))
    q8, sq = it.quantize_tokens(qr)
    return scores(q8, sq, q_off, encode(page_raw), d_off, clamp0)
