// The fused append-encode of a live residual-compressed shard for gfx950 (MI355X): bf16 / f16 pages -> centroid codes AND residual
// bytes at the tail of a larger pair of arrays, in one pass (include/maxsim.h: msim_res_append).  The bits are those of
// msim_cent_encode_docs followed by msim_res_encode_docs on the same rows; a row is read from memory once and its code never makes
// a round trip.
//
//   res_append_kernel   cent_encode_kernel's body (centroid_index.hip) with res_encode_kernel's arithmetic (residual_codec.hip) as
//                       its epilogue.  Workgroup (page, block of 256 rows): every wave keeps 4 tiles of 16 page rows in registers
//                       (the B operand, 64 VGPRs) and streams the K centroids from L2 in tiles of 16; one chain of 4
//                       v_mfma_f32_16x16x32 from zero per (centroid tile, row tile), k ascending, a running (max, first k) per lane,
//                       the four lane groups folded at the end -- after which all four lanes of a row know its code.  Lane
//                       (l16, l4) still holds chunks 4 ks + l4 (ks = 0 .. 3) of row l16 of every tile: it loads the same four
//                       16-byte chunks of the winning centroid row (from L2), runs the eight fp32 subtractions and cutoff counts
//                       per chunk and stores four 2- / 4-byte fields; lane group 0 stores the code.  Row r of the input goes to
//                       row dst_row0 + r of both arrays.  A row past its page's end is computed on a copy of the page's last row
//                       and never stored.
// Nothing allocates or synchronises.  A page whose offsets fall outside 0 .. n_rows, or that is longer than max_doc_rows, is
// flagged and writes nothing; every destination row is checked against dst_rows before it becomes an address.
#pragma once
#include "centroid_index.hip"
#include "residual_codec.hip"

namespace msim {

template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_append_kernel(const uint16_t *__restrict__ X,        // [n_rows, 128]
                                                         const int32_t *__restrict__ off,      // [n_d + 1]
                                                         int n_d, long long n_rows, int max_doc_rows,
                                                         const uint16_t *__restrict__ C,        // [K, 128]
                                                         int K, const float *__restrict__ cutoffs,
                                                         uint16_t *__restrict__ codes,          // [dst_rows]
                                                         uint8_t *__restrict__ res,             // [dst_rows, 16 BITS]
                                                         long long dst_row0, long long dst_rows,
                                                         int32_t *__restrict__ status) {        // [n_d] or null
    constexpr int KS = kKSteps16;
    constexpr int NC = (1 << BITS) - 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l16 = lane & 15, l4 = lane >> 4;
    const int p = blockIdx.x;
    if (p >= n_d) return;
    const long long r0 = off[p], r1 = off[p + 1];
    const bool bad = r0 < 0 || r1 < r0 || r1 > n_rows || r1 - r0 > max_doc_rows;      // never trust a device offset with an address
    if (blockIdx.y == 0 && threadIdx.x == 0 && status) status[p] = bad ? 1 : 0;
    if (bad) return;
    const int len = (int)(r1 - r0);
    const int row_base = blockIdx.y * kCentEncRows + wave * (kCentEncTiles * 16);
    if (row_base >= len) return;

    // the wave's rows: B operands of up to 4 tiles (a row past the page's end reads the page's last row and is never stored)
    bf16x8 xf[kCentEncTiles][KS];
    bool live[kCentEncTiles];
#pragma unroll
    for (int t = 0; t < kCentEncTiles; ++t) {
        live[t] = row_base + t * 16 < len;                             // wave-uniform
        int row = row_base + t * 16 + l16;
        row = row < len ? row : len - 1;
        const uint16_t *src = X + (size_t)(r0 + row) * kDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[t][ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
    }
    float bs[kCentEncTiles];
    int bk[kCentEncTiles];
#pragma unroll
    for (int t = 0; t < kCentEncTiles; ++t) {
        bs[t] = -INFINITY;
        bk[t] = -1;
    }

    auto load_tile = [&](bf16x8 (&cf)[KS], int c) {                     // centroids 16 c .. 16 c + 15 (K is a multiple of 16)
        const uint16_t *src = C + (size_t)(c * 16 + l16) * kDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cf[ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
    };
    auto tile = [&](const bf16x8 (&cf)[KS], int c) {
        const int k0 = c * 16 + 4 * l4;                                 // D: lane holds row l16 against centroids k0 .. k0 + 3
#pragma unroll
        for (int t = 0; t < kCentEncTiles; ++t) {
            if (!live[t]) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma16<F16>(cf[ks], xf[t][ks], acc);      // one chain, k ascending
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (bk[t] < 0 || acc[r] > bs[t]) {                      // ascending k: the first of equal values stays
                    bs[t] = acc[r];
                    bk[t] = k0 + r;
                }
        }
    };

    const int n_tiles = K / 16;
    bf16x8 c0[KS], c1[KS];
    load_tile(c0, 0);
    for (int c = 0; c < n_tiles; c += 2) {                              // n_tiles is even
        load_tile(c1, c + 1);
        tile(c0, c);
        if (c + 2 < n_tiles) load_tile(c0, c + 2);
        tile(c1, c + 1);
    }

    float cut[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) cut[i] = cutoffs[i];
#pragma unroll
    for (int t = 0; t < kCentEncTiles; ++t) {
        if (!live[t]) continue;
        // the four 16-lane groups hold the same row over different centroids: the larger similarity, then the lower k
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bs[t], o);
            const int ok = __shfl_xor(bk[t], o);
            if (ok >= 0 && (bk[t] < 0 || ov > bs[t] || (ov == bs[t] && ok < bk[t]))) {
                bs[t] = ov;
                bk[t] = ok;
            }
        }
        const int row = row_base + t * 16 + l16;
        const long long dst = dst_row0 + r0 + row;
        const int code = bk[t] < 0 ? 0 : bk[t];
        if (row >= len || dst < 0 || dst >= dst_rows || code >= K) continue;        // (a code is < K by construction)
        // the epilogue: this lane's four chunks of the row against the same chunks of its centroid
        const uint16_t *csrc = C + (size_t)code * kDim + l4 * 8;
        bf16x8 cc[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cc[ks] = *reinterpret_cast<const bf16x8 *>(csrc + ks * 32);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            uint32_t field = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float e = elem_to_float<F16>((uint16_t)xf[t][ks][j]) - elem_to_float<F16>((uint16_t)cc[ks][j]);
                uint32_t b = 0;
#pragma unroll
                for (int i = 0; i < NC; ++i) b += cut[i] <= e ? 1u : 0u;
                field |= b << (j * BITS);
            }
            const int chunk = 4 * ks + l4;
            if constexpr (BITS == 2) *reinterpret_cast<uint16_t *>(res + dst * 32 + chunk * 2) = (uint16_t)field;
            else *reinterpret_cast<uint32_t *>(res + dst * 64 + chunk * 4) = field;
        }
        if (l4 == 0) codes[dst] = (uint16_t)code;
    }
}

}  // namespace msim
