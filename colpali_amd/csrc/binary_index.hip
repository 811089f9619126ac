// A 1-bit sign copy of a packed corpus for gfx950 (MI355X): a token-level first stage for two-stage search at 16 B per row, 1/16 of
// the bf16 shard.  Queries stay int8 (msim_i8_encode_queries, unchanged); a page row is its 128 sign bits, expanded to +-1 bytes in
// registers and scored on v_mfma_i32_16x16x64_i8.  Every per-token maximum is an exact integer, so a score's bits are fixed by the
// documented order below (include/maxsim.h: msim_bin_*).
//
// Encode: s_k = -1 where the sign bit of the stored 16-bit element is set (-0.0 and negative NaNs included), +1 otherwise.  A row is
//   16 bytes; dimension k is bit (k & 7) of byte (k >> 3), a set bit means +1 (the residual codec's little-endian bit string).
// Score:  I_ij = sum_k q8_ik s_jk (int32, exact, |I| <= 127 * 128);  M_ic = max_j I_ij (max(M_ic, 0) when clamp0[c]);
//         S_qc = the sequential fp32 sum, in token order, of float(M_ic) * sq_i.   0-row page: -inf.
//
// Kernels:
//   bin_encode_rows_kernel     16 lanes per row, 16 B (8 elements) each: a lane packs its 8 sign bits into one byte, the 16 lanes of
//                              a row store its 16 bytes side by side.  Integer work on the sign bit only.
//   bin_scores_kernel<NT,GW,D> the scorer of the int8 index (int8_index.hip: token_scores) over BinRows: one wave holds a GROUP of
//                              whole queries (NT 16-token tiles, the B operand) and streams a range of consecutive pages as ONE run
//                              of 16-row chunks, read by bounds-checked buffer loads D chunks ahead; two 16x16x64 MFMAs per (chunk,
//                              tile), v_max_i32 on the accumulators, only a chunk that holds a page boundary masked, one store per
//                              (query, page).  GW waves share a page range; consecutive workgroups of a range run on one XCD.
//                              New is the A operand: lane (row = lane & 15, l4 = lane >> 4) holds dimensions 16 l4 .. 16 l4 + 15 of
//                              each 64-dimension half, i.e. halfword l4 of bytes 0..7 and of bytes 8..15 of its row.  Each halfword
//                              becomes 16 bytes of +-1: per nibble one bit-field extract, one multiply that drops bit b into byte
//                              b, one mask and one v_perm_b32 that picks 0x01 or 0xff -- 32 VALU instructions per chunk and lane,
//                              paid once per row and shared by the NT tiles.
// THE PHANTOM ROW.  A row past the end of the stream comes back from the descriptor as zero bits, and zero bits are an all-(-1) row,
// not a zero row: it scores -sum_k q8_ik, which can beat every real row of a page.  Such rows sit only in the stream's last, partial
// chunk; that chunk holds the last page boundary (the stream's end), so token_scores takes its masked path, and rows past the
// boundary never reach a running max that is stored.
// Nothing allocates or synchronises.  Every address comes from a checked index: page offsets against the row count, query offsets
// against the token count and the caller's bound on a query's length.  A page range or a query whose offsets break them is
// written as NaN.
#pragma once
#include "int8_index.hip"

namespace msim {

constexpr int kBinRow = kDim / 8;            // bytes per sign-bit row

// the sign bits of one 16-byte piece (8 elements) as one byte: bit u set = element u is +1
__device__ __forceinline__ uint32_t bin_signs8(const bf16x8 &e) {
    uint32_t b = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) b |= ((((uint32_t)(uint16_t)e[u]) >> 15) ^ 1u) << u;
    return b;
}

// one row per 16 lanes: codes C [n_rows, 16] of X [n_rows, 128] (bf16 and f16 keep the sign in the same bit: one kernel body)
template <bool F16>
__global__ __launch_bounds__(256) void bin_encode_rows_kernel(const uint16_t *__restrict__ X, long long n_rows, uint8_t *__restrict__ C) {
    const int t = threadIdx.x, sub = t & 15;
    const long long r = (long long)blockIdx.x * 16 + (t >> 4);
    if (r >= n_rows) return;
    const bf16x8 e = *reinterpret_cast<const bf16x8 *>(X + r * kDim + sub * 8);
    C[r * kBinRow + sub] = (uint8_t)bin_signs8(e);
}

// 16 sign bits -> 16 bytes of +-1 (bit b -> byte b; set = 0x01, clear = 0xff)
__device__ __forceinline__ i32x4 bin_expand16(uint32_t h) {
    i32x4 out;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const uint32_t nib = (h >> (4 * n)) & 0xfu;                      // v_bfe_u32
        const uint32_t sel = (nib * 0x00204081u) & 0x01010101u;          // bit b of the nibble in byte b (the partial products do not overlap)
        out[n] = (int)__builtin_amdgcn_perm(0u, 0x000001ffu, sel);       // selector byte 0 -> 0xff (-1), 1 -> 0x01 (+1)
    }
    return out;
}

// The sign-bit rows as token_scores (int8_index.hip) reads them: 16 bytes per row, the lane keeps its two halfwords per chunk in
// flight and expands them to the two A operands when the chunk's turn comes; a page has no scale.
struct BinRows {
    const uint8_t *__restrict__ codes;
    static constexpr int kRowBytes = kBinRow;
    struct Chunk {
        uint32_t h[2];
    };
    __device__ __forceinline__ const void *row(long long r) const { return codes + r * kBinRow; }
    __device__ __forceinline__ static void load(const __amdgpu_buffer_rsrc_t &rs, int row, int l4, Chunk &c) {
        const int voff = row * kBinRow + l4 * 2;                     // past the stream's end: zero bits, i.e. the phantom all-(-1) row
        c.h[0] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, voff, 0, 0);
        c.h[1] = (uint16_t)__builtin_amdgcn_raw_buffer_load_b16(rs, voff + 8, 0, 0);
    }
    __device__ __forceinline__ static void operands(const Chunk &c, i32x4 &a0, i32x4 &a1) {
        a0 = bin_expand16(c.h[0]);
        a1 = bin_expand16(c.h[1]);
    }
    __device__ __forceinline__ float page_score(int, float T) const { return T; }
};

// NT, GW, D and the query plan (QG, TPQ, passes): as i8_scores_kernel
template <int NT, int GW, int D>
__global__ __launch_bounds__(256) void bin_scores_kernel(const int8_t *__restrict__ q8, const float *__restrict__ sq,
                                                         const int32_t *__restrict__ q_off, int n_q, long long q_rows, int QG, int TPQ,
                                                         int passes, const uint8_t *__restrict__ codes, const int32_t *__restrict__ d_off,
                                                         const uint8_t *__restrict__ clamp0, int n_d, long long d_rows, int ppw,
                                                         int n_groups, int n_gb, float *__restrict__ scores, long long ld) {
    token_scores<NT, GW, D>(q8, sq, q_off, n_q, q_rows, QG, TPQ, passes, BinRows{codes}, d_off, clamp0, n_d, d_rows, ppw, n_groups, n_gb,
                            scores, ld);
}

}  // namespace msim
