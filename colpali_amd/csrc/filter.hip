// Page filters for gfx950 (MI355X): which pages each query may return (include/maxsim.h: msim_filter_*).  A filter is either
//   BITS    uint32 words [rows, ld_words]: bit c % 32 of word c / 32 is page c; ld_words == 0: ONE row shared by every query;
//   LABELS  page_labels int32 [n], query_labels int32 [n_q]: page c is allowed for q iff page_labels[c] == query_labels[q];
// optionally ANDed with a tombstone mask `alive` uint8 [n] (0 = deleted).  No scorer and no selection kernel changes: a filter either
// masks a score matrix (-inf, then msim_topk_f32) or becomes a candidate list (then msim_fwd_candidates).
//
//   filter_pack_kernel   mask bytes -> words.  A wave owns 256 consecutive columns: each lane loads 4 mask bytes as ONE 32-bit word
//                        (byte loads where the row is not 4-byte aligned, and in the row's tail), a lane shuffle puts column
//                        64 j + lane into lane `lane`, and one ballot per 64 columns yields two words.  Columns >= n vote 0.
//   filter_mask_kernel   the streaming section of mine_mask_kernel: one lane per 4 consecutive columns, the filter (4 bits of one
//                        word, or 4 page labels) and the 4 tombstone bytes are read once per column group -- per row only where the
//                        filter has a row per query -- and -inf is stored only into the columns that change (16 bytes at a time where
//                        all four do and the row is 16-byte aligned).  The scores are never read.
//   filter_list_kernel   the ordered compaction.  One workgroup per query row walks the row in passes of kFilterSpan = 8192 columns:
//                        one word per lane (LABELS and `alive`: built on the fly, 32 ballots of 64 columns per wave, skipped where a
//                        bit word is already empty), a popcount, a wave prefix by lane shuffles, a per-wave carry through LDS and a
//                        running carry across passes give each lane the output position of its first page.  The order is by
//                        construction (ascending ids); nothing is sorted and there is no atomic.
//   filter_ids_kernel    one lane per entry of an id matrix: an in-shard id that is not allowed (or not alive) becomes -1.
// Every column, word and id index is checked against n before it becomes an address; nothing allocates or synchronises.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kFilterThreads = 256;
constexpr int kFilterTileCols = kFilterThreads * 4;    // columns per workgroup of the pack and mask kernels
constexpr int kFilterRowGroups = 64;                   // grid.y at most: each workgroup walks rows q, q + grid.y, ...
constexpr int kFilterSpan = kFilterThreads * 32;       // columns per pass of the list kernel: one 32-bit word per lane

enum { kFilterShared = 0, kFilterPerQuery = 1, kFilterLabels = 2 };

// what every consumer is handed: exactly one of (bits, page_labels + query_labels) is set
struct FilterArgs {
    const uint32_t *bits;
    long long ld_words;                                // 0: one shared row
    const int32_t *page_labels;
    const int32_t *query_labels;
    const uint8_t *alive;                              // or nullptr
};

// grid: (ceil(n / 1024), min(rows, 64)); mask [rows, ld_mask] bytes, words [rows, ld_words]
__global__ __launch_bounds__(kFilterThreads) void filter_pack_kernel(const uint8_t *__restrict__ mask, long long ld_mask, int rows,
                                                                     long long n, uint32_t *__restrict__ words, long long ld_words,
                                                                     int vec_ok) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long base = (long long)blockIdx.x * kFilterTileCols + wave * 256;       // the wave's first column: a multiple of 256
    if (base >= n) return;                                                             // wave-uniform
    const long long n_words = (n + 31) / 32;
    const long long c0 = base + 4 * lane;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        const uint8_t *row = mask + (long long)r * ld_mask;
        uint32_t w = 0;                                                                // the lane's 4 mask bytes, little-endian
        if (vec_ok && c0 + 4 <= n) {
            w = *reinterpret_cast<const uint32_t *>(row + c0);
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (c0 + u < n) w |= (uint32_t)row[c0 + u] << (8 * u);
        }
        unsigned long long b[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                  // column base + 64 j + lane sits in byte lane % 4 of lane 16 j + lane / 4
            const uint32_t got = (uint32_t)__shfl((int)w, 16 * j + (lane >> 2));
            b[j] = __builtin_amdgcn_ballot_w64(((got >> (8 * (lane & 3))) & 0xffu) != 0);
        }
        if (lane < 8) {
            const unsigned long long two = lane < 2 ? b[0] : lane < 4 ? b[1] : lane < 6 ? b[2] : b[3];
            const long long wi = base / 32 + lane;
            if (wi < n_words) words[(long long)r * ld_words + wi] = (uint32_t)(two >> (32 * (lane & 1)));
        }
    }
}

// the 4 bits of columns c0 .. c0 + 3 (c0 a multiple of 4, c0 < n: the word index is below ceil(n / 32))
__device__ __forceinline__ uint32_t filter_nibble(const uint32_t *__restrict__ row_words, long long c0) {
    return (row_words[c0 >> 5] >> (unsigned)(c0 & 31)) & 0xfu;
}

// grid: (ceil(n / 1024), min(n_q, 64))
template <int MODE>
__global__ __launch_bounds__(kFilterThreads) void filter_mask_kernel(float *__restrict__ scores, long long ld, int n_q, long long n,
                                                                     FilterArgs f, int vec_ok, int labels_vec_ok) {
    const float ninf = -__builtin_inff();
    const long long c0 = ((long long)blockIdx.x * kFilterThreads + threadIdx.x) * 4;
    if (c0 >= n) return;
    const int cols = n - c0 < 4 ? (int)(n - c0) : 4;                       // the row's tail
    const uint32_t in_row = (1u << cols) - 1u;
    uint32_t dead = 0;                                                     // bit u: column c0 + u is deleted
    if (f.alive != nullptr) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (u < cols && f.alive[c0 + u] == 0) dead |= 1u << u;
    }
    uint32_t shared_drop = dead;
    int32_t lab[4] = {0, 0, 0, 0};
    if (MODE == kFilterShared) {
        shared_drop |= ~filter_nibble(f.bits, c0) & in_row;
        if (!shared_drop) return;
    } else if (MODE == kFilterLabels) {
        if (cols == 4 && labels_vec_ok) {
            const i32x4 v = *reinterpret_cast<const i32x4 *>(f.page_labels + c0);
            lab[0] = v[0], lab[1] = v[1], lab[2] = v[2], lab[3] = v[3];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < cols) lab[u] = f.page_labels[c0 + u];
        }
    }
    for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
        uint32_t drop = shared_drop;
        if (MODE == kFilterPerQuery) {
            drop |= ~filter_nibble(f.bits + (long long)q * f.ld_words, c0) & in_row;
        } else if (MODE == kFilterLabels) {
            const int32_t want = f.query_labels[q];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (u < cols && lab[u] != want) drop |= 1u << u;
        }
        float *p = scores + (long long)q * ld + c0;
        if (drop == 0xfu && vec_ok) {
            *reinterpret_cast<f32x4 *>(p) = f32x4{ninf, ninf, ninf, ninf};
        } else if (drop) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (drop & (1u << u)) p[u] = ninf;
        }
    }
}

__global__ void filter_status_reset_kernel(int32_t *__restrict__ status) { *status = 0; }

// grid: n_q workgroups, one per query row.  cand [n_q, ld_cand] int64, counts int32 [n_q], *status: set to 1 by a row that overflows
template <int MODE>
__global__ __launch_bounds__(kFilterThreads) void filter_list_kernel(FilterArgs f, long long n, long long id_base,
                                                                     int64_t *__restrict__ cand, long long ld_cand, int m_cap,
                                                                     int32_t *__restrict__ counts, int32_t *__restrict__ status) {
    __shared__ int wave_sums[kFilterThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = blockIdx.x;
    const uint32_t *row_words = MODE == kFilterLabels ? nullptr : f.bits + (MODE == kFilterPerQuery ? q * f.ld_words : 0);
    const int32_t want = MODE == kFilterLabels ? f.query_labels[q] : 0;
    int64_t *out = cand + q * ld_cand;
    long long carry = 0;                                                   // allowed pages of the passes before this one (uniform)
    for (long long pass0 = 0; pass0 < n; pass0 += kFilterSpan) {
        const long long c = pass0 + (long long)threadIdx.x * 32;           // the lane's first column
        uint32_t word = 0;
        if (c < n) {
            word = MODE == kFilterLabels ? 0xffffffffu : row_words[c >> 5];
            if (n - c < 32) word &= (1u << (unsigned)(n - c)) - 1u;        // bits at or above n are never relied upon
        }
        if (MODE == kFilterLabels || f.alive != nullptr) {                 // the words of labels / tombstones, by ballot
            const unsigned long long busy = __builtin_amdgcn_ballot_w64(word != 0);
            const long long wave_c = pass0 + (long long)wave * 2048;       // 64 lanes x 32 columns
            uint32_t made = 0;
            for (int j = 0; j < 32; ++j) {                                 // columns wave_c + 64 j + lane: the words of lanes 2 j, 2 j + 1
                if (!((busy >> (2 * j)) & 3ull)) continue;                 // wave-uniform: both words are empty already
                const long long cc = wave_c + 64 * j + lane;
                bool ok = cc < n;
                if (MODE == kFilterLabels) ok = ok && f.page_labels[cc] == want;
                if (f.alive != nullptr) ok = ok && f.alive[cc] != 0;
                const unsigned long long two = __builtin_amdgcn_ballot_w64(ok);
                if ((lane >> 1) == j) made = (uint32_t)(two >> (32 * (lane & 1)));
            }
            word &= made;
        }
        const int mine = __builtin_popcount(word);
        int inc = mine;                                                    // inclusive prefix inside the wave
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int up = __shfl_up(inc, s);
            if (lane >= s) inc += up;
        }
        __syncthreads();                                                   // the previous pass has read wave_sums
        if (lane == 63) wave_sums[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < kFilterThreads / 64; ++w) {
            const int s = wave_sums[w];
            if (w < wave) before += s;
            total += s;
        }
        long long pos = carry + before + (inc - mine);
        while (word) {
            const int b = __builtin_ctz(word);
            word &= word - 1;
            if (pos < m_cap) out[pos] = id_base + c + b;
            ++pos;
        }
        carry += total;
    }
    for (long long j = carry + threadIdx.x; j < m_cap; j += kFilterThreads) out[j] = -1;
    if (threadIdx.x == 0) {
        counts[q] = (int32_t)carry;                                        // the true count (n <= 2^31 - 1)
        if (carry > m_cap) *status = 1;                                    // every overflowing row stores the same value
    }
}

// grid: (ceil(m / 256), min(n_q, 65535)); ids [n_q, ld] int64, m columns
template <int MODE>
__global__ __launch_bounds__(kFilterThreads) void filter_ids_kernel(int64_t *__restrict__ ids, long long ld, int n_q, long long m,
                                                                    long long n, long long id_base, FilterArgs f) {
    const long long j = (long long)blockIdx.x * kFilterThreads + threadIdx.x;
    if (j >= m) return;
    for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
        int64_t *p = ids + (long long)q * ld + j;
        const long long id = *p;
        const long long c = id - id_base;
        if (id < 0 || c < 0 || c >= n) continue;                           // -1, or another rank's
        bool ok;
        if (MODE == kFilterLabels) {
            ok = f.page_labels[c] == f.query_labels[q];
        } else {
            const uint32_t *row_words = f.bits + (MODE == kFilterPerQuery ? (long long)q * f.ld_words : 0);
            ok = (row_words[c >> 5] >> (unsigned)(c & 31)) & 1u;
        }
        if (f.alive != nullptr) ok = ok && f.alive[c] != 0;
        if (!ok) *p = -1;
    }
}

}  // namespace msim
