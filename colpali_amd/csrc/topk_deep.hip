// Deep row-wise top-k (1024 < k <= 8192; include/maxsim.h: msim_topk_deep_f32) with the order of topk_select.hip,
// (score descending, id ascending), bit for bit.
//
// topk_select.hip keeps k of every 4k per level and stops at k = seg / 4 = 1024.  This file selects by RADIX instead: the 32-bit
// score_key is histogrammed most-significant byte first (256 bins); after four passes the key T of the row's k-th entry and the
// number r of entries still owed by the bucket key == T are known.  Ties at T are resolved by id, smallest first:
//   * one workgroup per row (deep_row_kernel): the same radix select goes on into the id (explicit ids: 64 bits; implicit ids: the
//     column, from its highest byte that can be non-zero), but only while the bucket holds more than is owed -- no tie at the
//     threshold, no extra pass;
//   * split rows (deep_split_*): an ordered count -- every segment's tie count is stored, a tie's rank is the ties of the segments
//     before it plus its rank in column order inside its segment, and rank < r wins.
// Membership of the survivor set is a function of the row's (score, id) set.  WHERE a survivor lands in the gather list is decided
// by an atomically claimed slot; the bitonic sort under ranks_before that follows fixes the order.  (Entries with the same score AND
// the same id are interchangeable: which of them fill the last places is left to a counter.)
// The survivors, at most k, are sorted in dynamic LDS at 12 B per entry (u32 key, u64 id): 96 KiB at k = 8192.
//
// Counts are integers, added with LDS / L2 atomics: the sums do not depend on the order of arrival.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_order.hpp"

namespace msim {

constexpr int kDeepMaxK = 8192;
constexpr int kDeepRowThreads = 1024;       // one workgroup per row: 16 waves share one row's 96 KiB sort
constexpr int kDeepRowLoads = 4;            // scores a thread requests per round of a key pass
constexpr int kDeepSplitThreads = 256;
constexpr int kDeepSplitPer = 8;            // consecutive columns per thread: thread order is column order
constexpr int kDeepSplitSeg = kDeepSplitThreads * kDeepSplitPer;
constexpr int kDeepEntryBytes = 12;
constexpr int kDeepLdsTail = (256 + 8) * 4;  // histogram and the pick's four words (+ two counters) behind the entries
// per row of a split plan, zeroed by the host on the stream in every call: four 256-bin histograms and the gather counter (+ 3 pad)
constexpr int kDeepRowWords = 4 * 256 + 4;

// ---- counting: all lanes of the wave call these (uniform control flow); `on` says whether this lane takes part
__device__ __forceinline__ void deep_count(uint32_t *hist, bool on, uint32_t bin) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(on);
    if (m == 0ull) return;
    const int first = __builtin_ctzll(m);
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first);
    // score rows crowd into one bin of the top byte: the lanes that share the first live lane's bin add once, together
    const unsigned long long same = __builtin_amdgcn_ballot_w64(on && bin == b0);
    if (on) {
        if (bin != b0) atomicAdd(&hist[bin], 1u);
        else if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
    }
}

// the same for N entries per lane at once: one broadcast and one add for all the entries of the wave that share the first live
// entry's bin (a ballot and a scalar popcount each), one branch over the rest -- which is all a pass does per entry when nothing of
// the wave matches the prefix any more
template <int N>
__device__ __forceinline__ void deep_count_n(uint32_t *hist, const bool (&on)[N], const uint32_t (&bin)[N]) {
    bool any = false;
    uint32_t mine = 0u;
#pragma unroll
    for (int u = N - 1; u >= 0; --u) {
        any = any || on[u];
        if (on[u]) mine = bin[u];               // (ends as the lane's first live entry's bin)
    }
    const unsigned long long m = __builtin_amdgcn_ballot_w64(any);
    if (m == 0ull) return;
    const int first = __builtin_ctzll(m);
    const uint32_t b0 = (uint32_t)__shfl((int)mine, first);
    uint32_t same = 0u;
    bool other = false;
#pragma unroll
    for (int u = 0; u < N; ++u) {
        same += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(on[u] && bin[u] == b0));
        other = other || (on[u] && bin[u] != b0);
    }
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], same);
    if (__builtin_amdgcn_ballot_w64(other) != 0ull) {
#pragma unroll
        for (int u = 0; u < N; ++u)
            if (on[u] && bin[u] != b0) atomicAdd(&hist[bin[u]], 1u);
    }
}

// a slot of `counter` for every lane with `take`: one atomic per wave.  The slot's VALUE depends on arrival order.
__device__ __forceinline__ uint32_t deep_claim(uint32_t *counter, bool take) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(take);
    if (m == 0ull) return 0u;
    const int lane = threadIdx.x & 63;
    const int first = __builtin_ctzll(m);
    uint32_t base = 0u;
    if (lane == first) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, first);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// One digit of the select: of the 256 bins in `hist` (LDS), walked from bin 255 down (DESC: key digits) or from bin 0 up (id
// digits), the bin that holds the r-th entry.  sel[0] = bin, sel[1] = entries still owed inside it (1 .. its count), sel[2] = its
// count, sel[3] = the sum of all bins.  r is clamped to the sum (a row with fewer than k entries gives all it has); a sum of 0 leaves
// sel[1] = 0.  Wave 0 works (4 bins per lane), every thread of the workgroup calls; ends with a barrier.
template <bool DESC>
__device__ __forceinline__ void deep_pick(const uint32_t *hist, uint32_t r, uint32_t *sel) {
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        uint32_t h[4];
        uint32_t s = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pos = lane * 4 + j;
            h[j] = hist[DESC ? 255 - pos : pos];
            s += h[j];
        }
        uint32_t inc = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
            if (lane >= d) inc += o;
        }
        const uint32_t total = (uint32_t)__shfl((int)inc, 63);
        if (r > total) r = total;
        if (lane == 0) {
            sel[3] = total;
            if (total == 0u) sel[0] = 0u, sel[1] = 0u, sel[2] = 0u;
        }
        uint32_t before = inc - s;
        if (r > before && r <= inc) {                      // exactly one lane when total > 0 (r >= 1)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (r > before && r <= before + h[j]) {
                    const int pos = lane * 4 + j;
                    sel[0] = (uint32_t)(DESC ? 255 - pos : pos);
                    sel[1] = r - before;
                    sel[2] = h[j];
                }
                before += h[j];
            }
        }
    }
    __syncthreads();
}

// bitonic sort of (skey, sid)[0 .. npow2) best-first under ranks_before; every thread of the workgroup calls
template <int THREADS>
__device__ __forceinline__ void deep_sort(uint32_t *skey, uint64_t *sid, int npow2) {
    const int tid = threadIdx.x;
    for (int size = 2; size <= npow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < npow2 / 2; t += THREADS) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool first_wins = (lo & size) == 0;
                const uint32_t ka = skey[lo], kb = skey[hi];
                const uint64_t ia = sid[lo], ib = sid[hi];
                if (ranks_before(ka, ia, kb, ib) != first_wins) {
                    skey[lo] = kb, skey[hi] = ka;
                    sid[lo] = ib, sid[hi] = ia;
                }
            }
        }
    }
    __syncthreads();
}

// pad [have, npow2) with "no entry", sort, and write the row's k outputs with the (-inf, -1) padding.  sid holds the id
// (explicit) or the column (implicit: the id is id_base + column).
template <int THREADS>
__device__ __forceinline__ void deep_sort_store(uint32_t *skey, uint64_t *sid, int have, int k, bool implicit, long long id_base,
                                                float *__restrict__ os, int64_t *__restrict__ oi) {
    int npow2 = 64;
    while (npow2 < have) npow2 <<= 1;
    for (int i = have + (int)threadIdx.x; i < npow2; i += THREADS) skey[i] = 0u, sid[i] = ~0ull;
    deep_sort<THREADS>(skey, sid, npow2);
    for (int j = threadIdx.x; j < k; j += THREADS) {
        const bool valid = j < have;
        os[j] = valid ? key_score(skey[j]) : -INFINITY;
        oi[j] = valid ? (implicit ? (int64_t)(id_base + (long long)sid[j]) : (int64_t)sid[j]) : -1;
    }
}

// ---------------------------------------------------------------- one workgroup per row
// grid: n_q; dynamic LDS: cap x 12 B + kDeepLdsTail, cap = the power of two >= max(64, min(k, n)).  The row is re-read per digit
// pass (L2 hits for all but the longest rows).  first_id_digit: the first of the eight id bytes (most significant = 0) that can
// differ -- 0 with explicit ids, 8 - bytes(n - 1) for columns.
__global__ __launch_bounds__(kDeepRowThreads) void deep_row_kernel(const float *__restrict__ scores, const int64_t *__restrict__ ids,
                                                                   long long n, long long ld, long long id_base, int k, int cap,
                                                                   int first_id_digit, float *__restrict__ out_scores,
                                                                   int64_t *__restrict__ out_ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char deep_lds[];
    uint64_t *sid = reinterpret_cast<uint64_t *>(deep_lds);
    uint32_t *skey = reinterpret_cast<uint32_t *>(sid + cap);
    uint32_t *hist = skey + cap;
    uint32_t *sel = hist + 256;                 // [0..3] the pick, [4] gather counter, [5] counter of the == bucket
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const float *srow = scores + row * ld;
    const int64_t *irow = ids ? ids + row * ld : nullptr;
    float *os = out_scores + row * (long long)k;
    int64_t *oi = out_ids + row * (long long)k;

    // ---- the key T of the k-th entry: four digits, most significant first
    uint32_t prefix = 0u, owed = (uint32_t)k, bucket = 0u;
    for (int d = 0; d < 4; ++d) {
        const int shift = 24 - 8 * d;
        const uint32_t above = d == 0 ? 0u : 0xffffffffu << (shift + 8);          // the bits the passes before decided ...
        const uint32_t want = d == 0 ? 0u : prefix << (shift + 8);                // ... and what they decided
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (long long b = 0; b < n; b += kDeepRowLoads * kDeepRowThreads) {       // (uniform trip count: ballots inside)
            uint32_t bin[kDeepRowLoads];
            bool on[kDeepRowLoads];
#pragma unroll
            for (int u = 0; u < kDeepRowLoads; ++u) {                              // the loads of one round, all requested first
                const long long i = b + u * kDeepRowThreads + tid;
                on[u] = i < n;
                const uint32_t key = on[u] ? score_key(srow[i]) : 0u;
                if (irow && on[u]) on[u] = irow[i] >= 0;
                on[u] = on[u] && (key & above) == want;
                bin[u] = (key >> shift) & 255u;
            }
            deep_count_n<kDeepRowLoads>(hist, on, bin);
        }
        __syncthreads();
        deep_pick<true>(hist, owed, sel);
        prefix = (prefix << 8) | sel[0];
        owed = sel[1];
        bucket = sel[2];
        __syncthreads();                        // everyone has read sel and hist
        if (owed == 0u) break;                  // (uniform) the row has no entry at all
    }
    if (owed == 0u) {
        for (int j = tid; j < k; j += kDeepRowThreads) os[j] = -INFINITY, oi[j] = -1;
        return;
    }
    const uint32_t T = prefix;

    // ---- ties at T: the smallest ids, by the same select on the id's bytes, while the bucket holds more than it owes
    uint64_t id_prefix = 0ull;
    int id_digits = 0;                          // id bytes decided, counted from the most significant
    for (int d = first_id_digit; d < 8 && owed < bucket; ++d) {
        const int shift = 56 - 8 * d;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (long long b = 0; b < n; b += kDeepRowThreads) {
            const long long i = b + tid;
            bool on = i < n;
            uint64_t id = 0ull;
            if (on) {
                id = irow ? (uint64_t)irow[i] : (uint64_t)i;
                on = score_key(srow[i]) == T && (!irow || (int64_t)id >= 0);
            }
            on = on && (d == 0 || (id >> (shift + 8)) == id_prefix);
            deep_count(hist, on, (uint32_t)(id >> shift) & 255u);
        }
        __syncthreads();
        deep_pick<false>(hist, owed, sel);
        id_prefix = (id_prefix << 8) | sel[0];
        owed = sel[1];
        bucket = sel[2];
        id_digits = d + 1;
        __syncthreads();
    }

    // ---- gather: key > T, ties whose id is below the decided prefix, and `owed` entries of the bucket that is left (all of it,
    // unless the row lists the same (score, id) more than once)
    if (tid == 0) sel[4] = 0u, sel[5] = 0u;
    __syncthreads();
    const int id_shift = 64 - 8 * id_digits;    // (unused when id_digits == 0)
    for (long long b = 0; b < n; b += kDeepRowThreads) {
        const long long i = b + tid;
        bool on = i < n;
        uint32_t key = 0u;
        uint64_t id = 0ull;
        if (on) {
            key = score_key(srow[i]);
            id = irow ? (uint64_t)irow[i] : (uint64_t)i;
            on = key >= T && (!irow || (int64_t)id >= 0);
        }
        bool take = on && key > T;
        bool last = on && key == T;
        if (id_digits > 0) {
            const uint64_t hi = id >> id_shift;
            take = take || (last && hi < id_prefix);
            last = last && hi == id_prefix;
        }
        const uint32_t turn = deep_claim(&sel[5], last);
        take = take || (last && turn < owed);
        const uint32_t slot = deep_claim(&sel[4], take);
        if (take && slot < (uint32_t)cap) skey[slot] = key, sid[slot] = id;
    }
    __syncthreads();
    int have = (int)sel[4];
    have = have > k ? k : have > cap ? cap : have;
    __syncthreads();
    deep_sort_store<kDeepRowThreads>(skey, sid, have, k, irow == nullptr, id_base, os, oi);
}

// ---------------------------------------------------------------- split rows (implicit ids): few long rows
// Workspace of row q: counts[q] = kDeepRowWords u32 (hist[4][256], gather counter), seg_hist[q][segs][256] u32 (every word written
// by pass 3: never zeroed), surv_key / surv_col [q][k] u32.

// the digits chosen so far: walks the finished histograms of passes 0 .. upto-1 (each a copy into LDS and one pick).  Returns the
// prefix; *owed / *bucket as deep_pick leaves them (owed == 0: the row has no entry)
__device__ __forceinline__ uint32_t deep_split_prefix(const uint32_t *__restrict__ counts, int upto, int k, uint32_t *hist, uint32_t *sel,
                                                      uint32_t *owed_out, uint32_t *bucket_out) {
    uint32_t prefix = 0u, owed = (uint32_t)k, bucket = 0u;
    for (int p = 0; p < upto; ++p) {
        hist[threadIdx.x] = counts[p * 256 + threadIdx.x];
        __syncthreads();
        deep_pick<true>(hist, owed, sel);
        prefix = (prefix << 8) | sel[0];
        owed = sel[1];
        bucket = sel[2];
        __syncthreads();
        if (owed == 0u) break;
    }
    *owed_out = owed;
    *bucket_out = bucket;
    return prefix;
}

// grid: (segs, n_q).  Pass d adds this segment's digit-d counts of the keys that match the prefix of passes < d.
__global__ __launch_bounds__(kDeepSplitThreads) void deep_split_hist_kernel(const float *__restrict__ scores, long long n, long long ld, int k,
                                                                            int d, uint32_t *__restrict__ counts_all,
                                                                            uint32_t *__restrict__ seg_hist_all) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t lhist[256];
    __shared__ uint32_t sel[4];
    const int tid = threadIdx.x;
    const long long row = blockIdx.y;
    uint32_t *counts = counts_all + row * kDeepRowWords;
    lhist[tid] = 0u;
    uint32_t owed, bucket;
    const uint32_t prefix = deep_split_prefix(counts, d, k, hist, sel, &owed, &bucket);     // (barriers inside; at d == 0: none)
    __syncthreads();
    const int shift = 24 - 8 * d;
    if (owed != 0u) {
        const long long base = (long long)blockIdx.x * kDeepSplitSeg;
        const float *srow = scores + row * ld;
        const uint32_t above = d == 0 ? 0u : 0xffffffffu << (shift + 8);
        const uint32_t want = d == 0 ? 0u : prefix << (shift + 8);
        uint32_t bin[kDeepSplitPer];
        bool on[kDeepSplitPer];
#pragma unroll
        for (int j = 0; j < kDeepSplitPer; ++j) {
            const long long i = base + j * kDeepSplitThreads + tid;          // (a histogram does not care about column order)
            on[j] = i < n;
            const uint32_t key = on[j] ? score_key(srow[i]) : 0u;
            on[j] = on[j] && (key & above) == want;
            bin[j] = (key >> shift) & 255u;
        }
        deep_count_n<kDeepSplitPer>(lhist, on, bin);
    }
    __syncthreads();
    const uint32_t c = lhist[tid];
    if (c) atomicAdd(&counts[d * 256 + tid], c);
    if (d == 3) seg_hist_all[(row * gridDim.x + blockIdx.x) * 256 + tid] = c;
}

// exclusive prefix of `v` over the workgroup's threads in thread order; *total = the sum.  wsum: LDS [THREADS / 64 + 1]
__device__ __forceinline__ uint32_t deep_block_excl(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += o;
    }
    __syncthreads();                            // wsum is free (a previous call's readers are done)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kDeepSplitThreads / 64; ++w) {
        const uint32_t s = wsum[w];
        if (w < wave) before += s;
        all += s;
    }
    *total = all;
    return before + inc - v;
}

// grid: (segs, n_q).  Thread t owns columns base + 8 t .. + 7, so thread order is column order: a tie's rank is (ties of the
// segments before, from seg_hist) + (ties of the threads before) + (its place among the thread's own).
__global__ __launch_bounds__(kDeepSplitThreads) void deep_split_gather_kernel(const float *__restrict__ scores, long long n, long long ld, int k,
                                                                              uint32_t *__restrict__ counts_all,
                                                                              const uint32_t *__restrict__ seg_hist_all,
                                                                              uint32_t *__restrict__ surv_key_all,
                                                                              uint32_t *__restrict__ surv_col_all) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sel[4];
    __shared__ uint32_t wsum[kDeepSplitThreads / 64 + 1];
    __shared__ uint32_t claimed;
    const int tid = threadIdx.x;
    const long long row = blockIdx.y;
    uint32_t *counts = counts_all + row * kDeepRowWords;
    uint32_t owed, bucket;
    const uint32_t T = deep_split_prefix(counts, 4, k, hist, sel, &owed, &bucket);
    if (owed == 0u) return;                     // (uniform) nothing in this row
    const long long base = (long long)blockIdx.x * kDeepSplitSeg + (long long)tid * kDeepSplitPer;
    const float *srow = scores + row * ld;
    uint32_t key[kDeepSplitPer];
    uint32_t above = 0u, ties = 0u;
#pragma unroll
    for (int j = 0; j < kDeepSplitPer; ++j) {
        key[j] = base + j < n ? score_key(srow[base + j]) : 0u;         // 0: below every entry's key (T >= score_key(-inf) > 0)
        above += key[j] > T;
        ties += key[j] == T;
    }
    // ties in the segments before this one
    uint32_t part = 0u;
    const uint32_t *sh = seg_hist_all + row * gridDim.x * 256 + (T & 255u);
    for (int s = tid; s < (int)blockIdx.x; s += kDeepSplitThreads) part += sh[(long long)s * 256];
    uint32_t ties_before_seg, ties_seg, tie_rank;
    (void)deep_block_excl(part, wsum, &ties_before_seg);
    tie_rank = ties_before_seg + deep_block_excl(ties, wsum, &ties_seg);
    uint32_t mine = above;
#pragma unroll
    for (int j = 0; j < kDeepSplitPer; ++j) {
        if (key[j] == T) {
            if (tie_rank < owed) ++mine;
            else key[j] = 0u;                   // a tie that lost: no longer a candidate
            ++tie_rank;
        }
    }
    uint32_t total;
    uint32_t at = deep_block_excl(mine, wsum, &total);
    if (tid == 0) claimed = total ? atomicAdd(&counts[4 * 256], total) : 0u;      // where the block lands: arrival order, the sort undoes it
    __syncthreads();
    at += claimed;
    uint32_t *sk = surv_key_all + row * (long long)k;
    uint32_t *sc = surv_col_all + row * (long long)k;
#pragma unroll
    for (int j = 0; j < kDeepSplitPer; ++j) {
        if (key[j] >= T && key[j] != 0u) {
            if (at < (uint32_t)k) sk[at] = key[j], sc[at] = (uint32_t)(base + j);
            ++at;
        }
    }
}

// grid: n_q; dynamic LDS as deep_row_kernel (no histogram needed, same layout).  Sorts the row's gathered survivors and stores.
__global__ __launch_bounds__(kDeepRowThreads) void deep_split_sort_kernel(const uint32_t *__restrict__ counts_all,
                                                                          const uint32_t *__restrict__ surv_key_all,
                                                                          const uint32_t *__restrict__ surv_col_all, int k, int cap,
                                                                          long long id_base, float *__restrict__ out_scores,
                                                                          int64_t *__restrict__ out_ids) {
    extern __shared__ __attribute__((aligned(16))) unsigned char deep_lds[];
    uint64_t *sid = reinterpret_cast<uint64_t *>(deep_lds);
    uint32_t *skey = reinterpret_cast<uint32_t *>(sid + cap);
    const long long row = blockIdx.x;
    int have = (int)counts_all[row * kDeepRowWords + 4 * 256];
    have = have > k ? k : have > cap ? cap : have;
    const uint32_t *sk = surv_key_all + row * (long long)k;
    const uint32_t *sc = surv_col_all + row * (long long)k;
    for (int i = threadIdx.x; i < have; i += kDeepRowThreads) skey[i] = sk[i], sid[i] = (uint64_t)sc[i];
    deep_sort_store<kDeepRowThreads>(skey, sid, have, k, true, id_base, out_scores + row * (long long)k, out_ids + row * (long long)k);
}

}  // namespace msim
