// Hard-negative mining over a score matrix and the page gather behind it, for gfx950 (MI355X) (include/maxsim.h: msim_mine_*,
// msim_gather_pages).  Mining is "mask, then the existing selection": the full scan and msim_topk_f32 are unchanged.
//
//   mine_bounds_kernel   one wave per query: pos[q] = the maximum of scores[q, c] over the query's positives that lie in the shard
//                        and are alive (CSR: pos_ids[pos_off[q] .. pos_off[q + 1])), or +inf where there is none (-inf in `local`
//                        mode: the value a rank that holds no positive sends into the all-reduce).
//   mine_mask_kernel     grid.x = column tiles of 1024, then ONE more column of workgroups (the scatter section); grid.y = row groups.
//                        Streaming section, one lane per 4 consecutive columns: the 4 mask bytes are read once, then per row one
//                        16-byte load, the compare against fp32(max_ratio) * pos[q] (one multiply, the reference's `scores > thresh`),
//                        and stores of -inf only into the columns that change (16 bytes at a time where all four do).
//                        Scatter section: -inf at scores[q, id - id_base] for every in-shard positive of q.
//                        Both sections only ever write -inf, and the streaming section never rewrites a column it leaves alone, so
//                        their order is free; a positive's column is -inf in the end whichever section got there first.
//   gather_pages_kernel  one workgroup per output slot: id -> page (checked against [id_base, id_base + n_d)), its offsets (checked
//                        against [0, d_rows]), then min(len, pad_rows) rows as ONE contiguous run of 16-byte pieces, four in flight per
//                        lane, and zeros up to pad_rows.  Bytes moved: slots x pad_rows x row_bytes written, the copied rows read,
//                        12 bytes of id and length per slot: a copy bound by HBM (MI355X: 8 TB/s nominal, ~6.3 TB/s for a plain copy).
// Every column, positive and row index is checked before it becomes an address; nothing allocates or synchronises.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kMineThreads = 256;
constexpr int kMineTileCols = kMineThreads * 4;    // columns per workgroup of the streaming section
constexpr int kMineRowGroups = 64;                 // grid.y at most: each workgroup walks rows q, q + grid.y, ...

typedef __attribute__((ext_vector_type(4))) unsigned int mine_u32x4;

// the query's slice of the positives list, clipped to [0, nnz] (a broken offset pair yields an empty slice, never an address)
__device__ __forceinline__ void mine_pos_range(const int32_t *__restrict__ pos_off, int q, long long nnz, long long *a, long long *b) {
    long long lo = pos_off[q], hi = pos_off[q + 1];
    if (lo < 0) lo = 0;
    if (hi > nnz) hi = nnz;
    *a = lo;
    *b = hi;                                       // hi <= lo: nothing to do
}

// grid: ceil(n_q / 4) workgroups of 4 waves, one wave per query
__global__ __launch_bounds__(kMineThreads) void mine_bounds_kernel(const float *__restrict__ scores, long long ld, int n_q, long long n,
                                                                   const int64_t *__restrict__ pos_ids,
                                                                   const int32_t *__restrict__ pos_off, long long nnz,
                                                                   long long id_base, const uint8_t *__restrict__ alive, int local,
                                                                   float *__restrict__ bounds) {
    const int lane = threadIdx.x & 63;
    const long long q = (long long)blockIdx.x * (kMineThreads / 64) + (threadIdx.x >> 6);
    if (q >= n_q) return;                                // wave-uniform
    long long a, b;
    mine_pos_range(pos_off, (int)q, nnz, &a, &b);
    float best = -__builtin_inff();
    int found = 0;
    for (long long i = a + lane; i < b; i += 64) {
        const long long id = pos_ids[i];
        const long long c = id - id_base;
        if (id >= 0 && c >= 0 && c < n && (alive == nullptr || alive[c] != 0)) {
            const float v = scores[q * ld + c];
            best = v > best ? v : best;
            found = 1;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const float o = __shfl_xor(best, s);
        best = o > best ? o : best;
        found |= __shfl_xor(found, s);
    }
    if (lane == 0) bounds[q] = found ? best : (local ? -__builtin_inff() : __builtin_inff());
}

// RATIO: compare against max_ratio * bounds[q] (reads the scores); otherwise only the tombstones decide (nothing is read but `alive`)
template <bool RATIO>
__global__ __launch_bounds__(kMineThreads) void mine_mask_kernel(float *__restrict__ scores, long long ld, int n_q, long long n,
                                                                 const float *__restrict__ bounds, float max_ratio,
                                                                 const uint8_t *__restrict__ alive, const int64_t *__restrict__ pos_ids,
                                                                 const int32_t *__restrict__ pos_off, long long nnz, long long id_base,
                                                                 unsigned tiles, int vec_ok) {
    const float ninf = -__builtin_inff();
    if (blockIdx.x >= tiles) {                           // the scatter section: the positives' own columns
        for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
            long long a, b;
            mine_pos_range(pos_off, q, nnz, &a, &b);
            for (long long i = a + threadIdx.x; i < b; i += kMineThreads) {
                const long long id = pos_ids[i];
                const long long c = id - id_base;
                if (id >= 0 && c >= 0 && c < n) scores[(long long)q * ld + c] = ninf;
            }
        }
        return;
    }
    const long long c0 = ((long long)blockIdx.x * kMineThreads + threadIdx.x) * 4;
    if (c0 >= n) return;
    const int cols = n - c0 < 4 ? (int)(n - c0) : 4;     // the row's tail
    bool dead[4];
    int n_dead = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        dead[u] = alive != nullptr && u < cols && alive[c0 + u] == 0;
        n_dead += dead[u];
    }
    if (!RATIO && !n_dead) return;
    for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
        float *p = scores + (long long)q * ld + c0;
        bool drop[4];
        int n_drop = 0;
        if (RATIO) {
            const float thresh = max_ratio * bounds[q];  // ONE fp32 multiply; NaN (0 x inf) compares false: nothing is dropped
            float v[4] = {ninf, ninf, ninf, ninf};
            if (cols == 4 && vec_ok) {
                const f32x4 w = *reinterpret_cast<const f32x4 *>(p);
                v[0] = w[0], v[1] = w[1], v[2] = w[2], v[3] = w[3];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (u < cols) v[u] = p[u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                drop[u] = u < cols && (dead[u] || v[u] > thresh);
                n_drop += drop[u];
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) drop[u] = dead[u];
            n_drop = n_dead;
        }
        if (n_drop == 4 && vec_ok) {
            *reinterpret_cast<f32x4 *>(p) = f32x4{ninf, ninf, ninf, ninf};
        } else if (n_drop) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (drop[u]) p[u] = ninf;
        }
    }
}

// grid: one workgroup per slot; rows [d_rows, lpr * 16 bytes], out [n_slots, pad_rows, lpr * 16 bytes]
__global__ __launch_bounds__(kMineThreads) void gather_pages_kernel(const uint8_t *__restrict__ rows, int lpr, long long d_rows,
                                                                    const int32_t *__restrict__ d_off, int n_d, long long id_base,
                                                                    const int64_t *__restrict__ ids, long long pad_rows,
                                                                    uint8_t *__restrict__ out, int32_t *__restrict__ lengths) {
    const long long slot = blockIdx.x;
    const long long id = ids[slot];
    const long long c = id - id_base;
    long long row0 = 0, len = 0;
    if (id >= 0 && c >= 0 && c < n_d) {
        const long long a = d_off[c], b = d_off[c + 1];
        if (a >= 0 && b >= a && b <= d_rows) {           // broken offsets: no page
            row0 = a;
            len = b - a < pad_rows ? b - a : pad_rows;
        }
    }
    if (threadIdx.x == 0) lengths[slot] = (int32_t)len;
    const long long copy = len * lpr, total = pad_rows * lpr;      // 16-byte pieces: the page's rows are one contiguous run
    const mine_u32x4 *src = reinterpret_cast<const mine_u32x4 *>(rows) + row0 * lpr;
    mine_u32x4 *dst = reinterpret_cast<mine_u32x4 *>(out) + slot * total;
    for (long long i0 = threadIdx.x; i0 < total; i0 += 4 * kMineThreads) {
        mine_u32x4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + u * kMineThreads;
            v[u] = mine_u32x4{0u, 0u, 0u, 0u};
            if (i < copy) v[u] = src[i];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = i0 + u * kMineThreads;
            if (i < total) dst[i] = v[u];
        }
    }
}

}  // namespace msim
