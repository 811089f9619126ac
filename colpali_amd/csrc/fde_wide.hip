// Fixed dimensional encodings (fde.hip) for rows of width 320 (ColQwen3) on gfx950 (MI355X): the encoder of pages and queries.
// The scorer depends on F alone, so fde_scores_kernel (msim_fde_scores) serves these encodings as it stands.
//
// The encoding is the one of fde.hip with 128 replaced by 320 (include/maxsim.h: msim_fdew_encode_docs): R reps, k_sim sign bits,
// d_proj projected values per bucket, B = 2^k_sim, F = R * B * d_proj, host-drawn G [R, k_sim, 320] (normal) and S [R, d_proj, 320]
// (+-1), both fp32:
//   bucket      phi_r(x) = sum_i 2^i [<G[r, i], x> > 0]
//   projection  psi_r(x) = S[r] x / sqrt(d_proj)
//   entry (r * B + b) * d_proj + j = psi_r(v)[j], v = the SUM of a query's tokens with phi_r = b, the MEAN of a page's rows with
//   phi_r = b; a page's empty bucket with fill_empty takes the row whose code is nearest to b in Hamming distance (lowest row
//   index on a tie); zeros otherwise, and for a 0-row item.
//
// fde_wide_encode_kernel: one 320-thread workgroup (5 waves) per item, rep by rep, all in fp32, rounded once on store.
//   1. codes: 80 rows per pass, 4 lanes per row, each an 80-column slice (ten 16-byte loads) of the k_sim dots against G[r] (fp32
//      from LDS; the four slices of a row sit 80 floats = 16 banks apart), folded by two xor-shuffles, (p0 + p1) + (p2 + p3) in
//      every lane.  Bucket counts and each bucket's first row are LDS integer atomics (add / min): order-free.
//   2. bucket sums: lane c owns column c of ONE copy of the sums, sums[b][c] for every b, and adds the pass's rows in row order:
//      sixteen values requested from L2 at a time, four rows per LDS round trip (a row that shares a bucket with an earlier row
//      of the four continues from that row's result).  The order depends on the item's rows only, so its bits do not depend on
//      the launch around it.
//   3. fill-empty: lane b < B searches the B codes' first rows once (an integer search), into fill[b]; then lane c turns every
//      bucket's sum into its mean (or keeps the sum), or copies the fill row.
//   4. projection: one output per lane and step, a 320-term dot with S[r] in a fixed order, S[r]^T staged in LDS at most 32
//      projected values at a time (two passes at d_proj = 64).
// LDS: the layout of fde.hip does not fit at width 320 -- two copies of the sums at k_sim = 6 alone are 164 352 B.  One lane per
// column needs one copy (82 176 B at a stride of 321 floats), and S[r]^T in slabs of 32 values at a stride of 33 floats is
// 42 240 B: 133 184 B at (k_sim, d_proj) = (6, 64) with G[r] and the small arrays, of the CU's 163 840 B.
// Nothing allocates or synchronises; every address comes from a checked index: an item whose offsets leave [0, n_rows] or run
// backwards gets NaN everywhere and reads nothing.  Row addresses are 64-bit (a row starts at row x 640 bytes).
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kFdwDim = 320;
constexpr int kFdwThreads = 320;            // one lane per column
constexpr int kFdwMaxKsim = 6;
constexpr int kFdwChunk = 80;               // rows per code pass (4 lanes per row)
constexpr int kFdwSlice = kFdwDim / 4;      // columns per code lane
constexpr int kFdwSumStride = kFdwDim + 1;  // LDS row stride of the bucket sums: the projection's lanes read 8 buckets conflict-free
constexpr int kFdwMaxSlab = 32;             // projected values of S[r]^T held in LDS at a time

__host__ __device__ constexpr int fde_wide_slab(int dproj) { return dproj < kFdwMaxSlab ? dproj : kFdwMaxSlab; }

// LDS bytes of fde_wide_encode_kernel for one configuration
__host__ __device__ constexpr int fde_wide_encode_lds_bytes(int ksim, int dproj) {
    return ((1 << ksim) * kFdwSumStride + ksim * kFdwDim + kFdwDim * (fde_wide_slab(dproj) + 1)) * 4 + (3 * 64 + kFdwChunk) * 4;
}

template <bool F16>
__device__ __forceinline__ uint16_t fde_wide_store_elem(float x) {
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)x);
    else return __builtin_bit_cast(uint16_t, (__bf16)x);
}

// one workgroup per item (page or query): rows off[item] .. off[item + 1] - 1 of X [n_rows, 320]
template <bool F16>
__global__ __launch_bounds__(kFdwThreads) void fde_wide_encode_kernel(const uint16_t *__restrict__ X, const int32_t *__restrict__ off,
                                                                      int n_items, long long n_rows, const float *__restrict__ G,
                                                                      const float *__restrict__ S, int R, int ksim, int dproj,
                                                                      int is_doc, int fill_empty, uint16_t *__restrict__ out,
                                                                      uint8_t *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int B = 1 << ksim;
    const int JP = fde_wide_slab(dproj), st_stride = JP + 1;
    float *Gs = reinterpret_cast<float *>(smem);                     // [ksim][320], first: read 16 bytes at a time
    float *sums = Gs + ksim * kFdwDim;                               // [B][kFdwSumStride]
    float *St = sums + B * kFdwSumStride;                            // [320][JP + 1]: St[c][jj] = S[r][j0 + jj][c]
    int *cnt = reinterpret_cast<int *>(St + kFdwDim * st_stride);    // [64]
    int *first = cnt + 64;                                           // [64]
    int *fill = first + 64;                                          // [64]: the row an empty bucket takes, or -1
    int *code_buf = fill + 64;                                       // [kFdwChunk]
    const int t = threadIdx.x;
    const int item = blockIdx.x;
    if (item >= n_items) return;
    const long long F = (long long)R * B * dproj;
    uint16_t *o = out + (size_t)item * F;
    const long long r0 = off[item], r1 = off[item + 1];
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {                          // never trust a device offset with an address
        const uint16_t nan = F16 ? 0x7e00 : 0x7fc0;
        for (long long f = t; f < F; f += kFdwThreads) o[f] = nan;
        return;
    }
    const int n = (int)(r1 - r0);
    const uint16_t *x = X + (size_t)r0 * kFdwDim;
    const float inv_sqrt = 1.0f / __builtin_sqrtf((float)dproj);
    const int c = t;                                                 // the bucket-sum lane's column
    const int crow = t >> 2, part = t & 3;                           // the code lane: row of the pass, 80-column slice

    for (int r = 0; r < R; ++r) {
        for (int i = t; i < ksim * kFdwDim; i += kFdwThreads) Gs[i] = G[(size_t)r * ksim * kFdwDim + i];
        for (int i = t; i < B * kFdwSumStride; i += kFdwThreads) sums[i] = 0.0f;
        if (t < 64) {
            cnt[t] = 0;
            first[t] = 0x7fffffff;
            fill[t] = -1;
        }
        __syncthreads();

        for (int c0 = 0; c0 < n; c0 += kFdwChunk) {
            // 1. codes of rows c0 .. c0 + 79
            const int row = c0 + crow;
            const bool live = row < n;
            float dot[kFdwMaxKsim];
#pragma unroll
            for (int k = 0; k < kFdwMaxKsim; ++k) dot[k] = 0.0f;
            if (live) {
                const bf16x8 *src = reinterpret_cast<const bf16x8 *>(x + (size_t)row * kFdwDim + part * kFdwSlice);
#pragma unroll 2
                for (int v = 0; v < kFdwSlice / 8; ++v) {
                    const bf16x8 e = src[v];
                    float xv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) xv[u] = elem_to_float<F16>((uint16_t)e[u]);
                    const float *g8 = Gs + part * kFdwSlice + v * 8;  // 32-byte aligned: two 16-byte LDS reads per sign bit
#pragma unroll
                    for (int k = 0; k < kFdwMaxKsim; ++k)
                        if (k < ksim) {
                            const f32x4 ga = *reinterpret_cast<const f32x4 *>(g8 + k * kFdwDim);
                            const f32x4 gb = *reinterpret_cast<const f32x4 *>(g8 + k * kFdwDim + 4);
#pragma unroll
                            for (int u = 0; u < 4; ++u) dot[k] = __builtin_fmaf(ga[u], xv[u], dot[k]);
#pragma unroll
                            for (int u = 0; u < 4; ++u) dot[k] = __builtin_fmaf(gb[u], xv[4 + u], dot[k]);
                        }
                }
            }
            int code = 0;
#pragma unroll
            for (int k = 0; k < kFdwMaxKsim; ++k) {
                float d = dot[k];
                d += __shfl_xor(d, 1);                               // (p0 + p1) + (p2 + p3) in every lane of the four
                d += __shfl_xor(d, 2);
                if (k < ksim && d > 0.0f) code |= 1 << k;
            }
            if (live && part == 0) {
                code_buf[crow] = code;
                atomicAdd(&cnt[code], 1);
                atomicMin(&first[code], row);
                if (codes) codes[(size_t)(r0 + row) * R + r] = (uint8_t)code;
            }
            __syncthreads();
            // 2. bucket sums: lane c adds column c of the pass's rows, in row order
            const int end = n - c0 < kFdwChunk ? n - c0 : kFdwChunk;
            // Sixteen rows a step: their sixteen values are requested together (one trip to L2, not sixteen), then four rows at a
            // time read their four sums together (one LDS round trip) and a row whose bucket an earlier row of the four shares
            // takes that row's result instead, so every bucket still adds its rows one by one in row order.  `end` and the codes are
            // the same in every lane: the branches are scalar.
            float *mine = sums + c;
            const uint16_t *xc = x + (size_t)c0 * kFdwDim + c;
            for (int i0 = 0; i0 < end; i0 += 16) {
                float xs[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {                        // past the pass's end: its last row again, unused (no branch)
                    const int ij = i0 + j < end ? i0 + j : end - 1;
                    xs[j] = elem_to_float<F16>(xc[(size_t)ij * kFdwDim]);
                }
#pragma unroll
                for (int g = 0; g < 16; g += 4) {
                    const int i = i0 + g;
                    if (i + 4 <= end) {
                        const int b0 = code_buf[i] * kFdwSumStride, b1 = code_buf[i + 1] * kFdwSumStride;
                        const int b2 = code_buf[i + 2] * kFdwSumStride, b3 = code_buf[i + 3] * kFdwSumStride;
                        float s1 = mine[b1], s2 = mine[b2], s3 = mine[b3];
                        const float v0 = mine[b0] + xs[g];
                        if (b1 == b0) s1 = v0;
                        const float v1 = s1 + xs[g + 1];
                        if (b2 == b1) s2 = v1;
                        else if (b2 == b0) s2 = v0;
                        const float v2 = s2 + xs[g + 2];
                        if (b3 == b2) s3 = v2;
                        else if (b3 == b1) s3 = v1;
                        else if (b3 == b0) s3 = v0;
                        const float v3 = s3 + xs[g + 3];
                        mine[b0] = v0;                               // in row order: the last write to a shared bucket is its latest sum
                        mine[b1] = v1;
                        mine[b2] = v2;
                        mine[b3] = v3;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (i + j < end) mine[code_buf[i + j] * kFdwSumStride] += xs[g + j];
                    }
                }
            }
            __syncthreads();
        }

        // 3. the row every empty bucket takes: nearest code, lowest first row on a tie
        if (t < B && is_doc && fill_empty && n > 0 && cnt[t] == 0) {
            int best_d = 99, best_row = 0x7fffffff;
            for (int b2 = 0; b2 < B; ++b2) {
                if (cnt[b2] == 0) continue;
                const int d = __popc((unsigned)(t ^ b2));
                const int fr = first[b2];
                if (d < best_d || (d == best_d && fr < best_row)) {
                    best_d = d;
                    best_row = fr;
                }
            }
            fill[t] = best_row >= 0 && best_row < n ? best_row : -1;
        }
        __syncthreads();
        // ... and the vector of every bucket, in place
        for (int b = 0; b < B; ++b) {
            const int nb = cnt[b];
            float v = 0.0f;
            if (nb > 0) {
                v = sums[b * kFdwSumStride + c];
                if (is_doc) v = v / (float)nb;
            } else {
                const int fr = fill[b];
                if (fr >= 0) v = elem_to_float<F16>(x[(size_t)fr * kFdwDim + c]);
            }
            sums[b * kFdwSumStride + c] = v;
        }

        // 4. projection: output (b, j) = sum_c S[r][j][c] v_b[c] / sqrt(d_proj), JP values of j at a time
        for (int j0 = 0; j0 < dproj; j0 += JP) {
            for (int i = t; i < JP * kFdwDim; i += kFdwThreads) {
                const int jj = i / kFdwDim, cc = i - jj * kFdwDim;   // coalesced read of S[r][j0 + jj][cc]
                St[cc * st_stride + jj] = S[((size_t)r * dproj + j0 + jj) * kFdwDim + cc];
            }
            __syncthreads();                                         // S[r]^T, and at j0 = 0 every bucket's vector
            for (int oi = t; oi < B * JP; oi += kFdwThreads) {
                const int b = oi / JP, jj = oi - b * JP;
                const float *vb = sums + b * kFdwSumStride;
                float acc = 0.0f;
                for (int cc = 0; cc < kFdwDim; ++cc) acc = __builtin_fmaf(St[cc * st_stride + jj], vb[cc], acc);
                o[((size_t)r * B + b) * dproj + j0 + jj] = fde_wide_store_elem<F16>(acc * inv_sqrt);
            }
            __syncthreads();                                         // LDS is rewritten by the next slab / rep
        }
    }
}

}  // namespace msim
