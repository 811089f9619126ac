// Document-level search for gfx950 (MI355X): pages grouped into documents (include/maxsim.h: msim_group_*).
//
// A shard's n pages belong to G documents, given as a CSR: offsets int32 [G + 1], pages int32 [n] -- the LOCAL page indices of
// document g are pages[offsets[g] .. offsets[g + 1]), ascending.  No scorer and no top-k kernel changes: the group reduction sits
// between the scan and msim_topk_f32, the grouped selection behind msim_fwd_candidates and behind the all-gather.
//
//   group_reduce_kernel  entry (q, g) of [n_q, G] = the best page of document g for query q under the project's order (score_key
//                        descending, page ascending).  A GATHER over the CSR: every output has exactly one owner, so there is no
//                        atomic and nothing depends on the order in which anything runs.  A workgroup owns 256 consecutive
//                        documents and walks the rows q, q + grid.y, ...; a document is reduced in one of three forms by its length:
//                          <= kGroupThreadMax   by ONE LANE: its page indices sit in up to 16 registers, loaded once for all rows;
//                          <= kGroupWaveMax     by ONE WAVE: lane l holds pages l, l + 64, ... (16 registers again), one packed
//                                               64-bit maximum per lane, six cross-lane steps;
//                          above                by the WORKGROUP: 256 lanes stride over the CSR (re-read per row: L2 hits, the list of
//                                               one document is at most 4 n bytes), wave maxima meet in LDS.
//                        A candidate is one u64 = (score_key << 32) | ~page, so "ranks before" is one unsigned compare and the
//                        maximum is the winner; a page that scores -inf packs to 0 and never wins.  The score written is re-read
//                        from the winner's column: its own bits, -0.0 included.
//   group_select_kernel  the grouped top-k of one candidate row per workgroup, two bitonic sorts in dynamic LDS (20 B per entry,
//                        80 KiB at m = 4096): by (document, score desc, page asc) -- the head of every run is its document's best
//                        entry --, then the heads by (score desc, document asc).
// Every page index is checked against n, every offset clipped to [0, n], before it becomes an address; nothing allocates or
// synchronises.
#pragma once
#include "maxsim_common.hpp"
#include "topk_select.hip"

namespace msim {

constexpr int kGroupThreads = 256;
constexpr int kGroupThreadMax = MSIM_GROUP_THREAD_MAX;   // longest document one lane reduces
constexpr int kGroupWaveMax = MSIM_GROUP_WAVE_MAX;       // longest document one wave reduces
constexpr int kGroupRegs = 16;                           // page indices a lane keeps: kGroupThreadMax, and kGroupWaveMax / 64
static_assert(kGroupThreadMax == kGroupRegs && kGroupWaveMax == 64 * kGroupRegs, "the register file of a lane holds 16 page indices");
constexpr uint32_t kGroupNoneKey = 0x007fffffu;          // score_key(-inf): a key at or below it is "no page"
constexpr int kGroupSelectMaxM = MSIM_GROUP_SELECT_MAX_M;
constexpr int kGroupSelectMaxK = MSIM_GROUP_SELECT_MAX_K;
constexpr int kGroupSelectEntryBytes = 20;               // u64 document, u64 page, u32 key

__device__ __forceinline__ unsigned long long group_pack(float s, int32_t page) {
    const uint32_t k = score_key(s);
    return k <= kGroupNoneKey ? 0ull : ((unsigned long long)k << 32) | (uint32_t)~(uint32_t)page;
}

__device__ __forceinline__ unsigned long long group_wave_max(unsigned long long v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ int group_wave_max_int(int v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const int o = __shfl_xor(v, s);
        v = o > v ? o : v;
    }
    return v;
}

// the winner of (q, g): its own score bits and its GLOBAL page id, or (-inf, -1)
__device__ __forceinline__ void group_store(unsigned long long best, const float *__restrict__ row, long long id_base,
                                            float *__restrict__ out_s, int64_t *__restrict__ out_p, long long at) {
    if (best == 0ull) {
        out_s[at] = -__builtin_inff();
        out_p[at] = -1;
    } else {
        const uint32_t page = ~(uint32_t)best;
        out_s[at] = row[page];
        out_p[at] = id_base + (long long)page;
    }
}

// grid: (ceil(G / 256), row groups).  scores [n_q, ld] fp32, offsets [G + 1], pages [n]; out_s / out_p [n_q, ld_out]
__global__ __launch_bounds__(kGroupThreads) void group_reduce_kernel(const float *__restrict__ scores, long long ld, int n_q, long long n,
                                                                     const int32_t *__restrict__ offsets,
                                                                     const int32_t *__restrict__ pages, int n_groups, long long id_base,
                                                                     float *__restrict__ out_s, int64_t *__restrict__ out_p,
                                                                     long long ld_out) {
    __shared__ unsigned long long long_docs[kGroupThreads / 64];       // per wave: which of its 64 documents the workgroup reduces
    __shared__ unsigned long long wave_best[kGroupThreads / 64];
    const float ninf = -__builtin_inff();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long g0 = (long long)blockIdx.x * kGroupThreads;
    const long long g = g0 + threadIdx.x;
    int beg = 0, len = 0;
    if (g < n_groups) {
        long long b = offsets[g], e = offsets[g + 1];
        b = b < 0 ? 0 : b > n ? n : b;
        e = e < b ? b : e > n ? n : e;
        beg = (int)b;
        len = (int)(e - b);
    }
    const bool mine = g < n_groups && len <= kGroupThreadMax;
    const unsigned long long by_wave = __builtin_amdgcn_ballot_w64(g < n_groups && len > kGroupThreadMax && len <= kGroupWaveMax);
    const unsigned long long by_block = __builtin_amdgcn_ballot_w64(g < n_groups && len > kGroupWaveMax);
    if (lane == 0) long_docs[wave] = by_block;

    // ---- one lane per document
    {
        const int longest = group_wave_max_int(mine ? len : 0);        // wave-uniform trip count
        int32_t pg[kGroupRegs];
#pragma unroll
        for (int j = 0; j < kGroupRegs; ++j) {
            pg[j] = -1;
            if (mine && j < len) {
                const int32_t p = pages[beg + j];
                pg[j] = (uint32_t)p < (unsigned long long)n ? p : -1;
            }
        }
        if (mine) {
            for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
                const float *row = scores + (long long)q * ld;
                unsigned long long best = 0ull;
                float bits = ninf;
#pragma unroll
                for (int j = 0; j < kGroupRegs; ++j) {
                    if (j >= longest) break;
                    const float s = pg[j] >= 0 ? row[pg[j]] : ninf;
                    const unsigned long long v = pg[j] >= 0 ? group_pack(s, pg[j]) : 0ull;
                    if (v > best) best = v, bits = s;
                }
                const long long at = (long long)q * ld_out + g;
                out_s[at] = bits;
                out_p[at] = best ? id_base + (long long)(uint32_t)~(uint32_t)best : -1;
            }
        }
    }

    // ---- one wave per document
    for (unsigned long long todo = by_wave; todo;) {
        const int src = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int gb = __shfl(beg, src), gl = __shfl(len, src);
        const long long gg = g0 + wave * 64 + src;
        int32_t pg[kGroupRegs];
#pragma unroll
        for (int j = 0; j < kGroupRegs; ++j) {
            const int i = lane + 64 * j;
            pg[j] = -1;
            if (i < gl) {
                const int32_t p = pages[gb + i];
                pg[j] = (uint32_t)p < (unsigned long long)n ? p : -1;
            }
        }
        for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
            const float *row = scores + (long long)q * ld;
            unsigned long long best = 0ull;
#pragma unroll
            for (int j = 0; j < kGroupRegs; ++j) {
                if (64 * j >= gl) break;                               // wave-uniform
                const float s = pg[j] >= 0 ? row[pg[j]] : ninf;
                const unsigned long long v = pg[j] >= 0 ? group_pack(s, pg[j]) : 0ull;
                best = v > best ? v : best;
            }
            best = group_wave_max(best);
            if (lane == 0) group_store(best, row, id_base, out_s, out_p, (long long)q * ld_out + gg);
        }
    }

    // ---- the workgroup per document
    __syncthreads();
    for (int w = 0; w < kGroupThreads / 64; ++w) {
        for (unsigned long long todo = long_docs[w]; todo;) {          // uniform over the workgroup
            const int src = __builtin_ctzll(todo);
            todo &= todo - 1;
            const long long gg = g0 + w * 64 + src;
            long long b = offsets[gg], e = offsets[gg + 1];
            b = b < 0 ? 0 : b > n ? n : b;
            e = e < b ? b : e > n ? n : e;
            const int gl = (int)(e - b);
            const int32_t *list = pages + b;
            for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
                const float *row = scores + (long long)q * ld;
                unsigned long long best = 0ull;
#pragma unroll 4
                for (int i = threadIdx.x; i < gl; i += kGroupThreads) {
                    const int32_t p = list[i];
                    if ((uint32_t)p < (unsigned long long)n) {
                        const unsigned long long v = group_pack(row[p], p);
                        best = v > best ? v : best;
                    }
                }
                best = group_wave_max(best);
                if (lane == 0) wave_best[wave] = best;
                __syncthreads();
                if (threadIdx.x == 0) {
#pragma unroll
                    for (int x = 1; x < kGroupThreads / 64; ++x) best = wave_best[x] > best ? wave_best[x] : best;
                    group_store(best, row, id_base, out_s, out_p, (long long)q * ld_out + gg);
                }
                __syncthreads();                                       // wave_best is free again
            }
        }
    }
}

// ---------------------------------------------------------------- the grouped top-k of candidate rows
// BY_DOC: (document ascending, score descending, page ascending) -- the first entry of a run is its document's best;
// otherwise (score descending, document ascending), the order of the result.  An empty entry is (key 0, document ~0): last in both.
template <bool BY_DOC>
__device__ __forceinline__ bool group_before(uint32_t ka, uint64_t ga, uint64_t pa, uint32_t kb, uint64_t gb, uint64_t pb) {
    if (BY_DOC) return ga < gb || (ga == gb && (ka > kb || (ka == kb && pa < pb)));
    return ka > kb || (ka == kb && ga < gb);
}

template <bool BY_DOC>
__device__ __forceinline__ void group_sort(uint32_t *skey, uint64_t *sgid, uint64_t *spage, int npow2, int tid) {
    for (int size = 2; size <= npow2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = tid; t < npow2 / 2; t += kGroupThreads) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool first_wins = (lo & size) == 0;
                const uint32_t ka = skey[lo], kb = skey[hi];
                const uint64_t ga = sgid[lo], gb = sgid[hi];
                const uint64_t pa = spage[lo], pb = spage[hi];
                if (group_before<BY_DOC>(ka, ga, pa, kb, gb, pb) != first_wins) {
                    skey[lo] = kb, skey[hi] = ka;
                    sgid[lo] = gb, sgid[hi] = ga;
                    spage[lo] = pb, spage[hi] = pa;
                }
            }
        }
    }
    __syncthreads();
}

// grid: n_q workgroups, one per row; dynamic LDS: npow2 x 20 bytes (npow2 = the power of two >= max(m, 64)); no static LDS, so
// the dynamic region starts 16-byte aligned.  scores / gids / pages [n_q, ld], m columns; outputs [n_q, k]
__global__ __launch_bounds__(kGroupThreads) void group_select_kernel(const float *__restrict__ scores, const int64_t *__restrict__ gids,
                                                                     const int64_t *__restrict__ pages, int m, long long ld, int k,
                                                                     int npow2, float *__restrict__ out_s, int64_t *__restrict__ out_g,
                                                                     int64_t *__restrict__ out_p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char group_lds[];
    uint64_t *sgid = reinterpret_cast<uint64_t *>(group_lds);
    uint64_t *spage = sgid + npow2;
    uint32_t *skey = reinterpret_cast<uint32_t *>(spage + npow2);
    const int tid = threadIdx.x;
    const long long row = blockIdx.x;
    const float *srow = scores + row * ld;
    const int64_t *grow = gids + row * ld;
    const int64_t *prow = pages + row * ld;
    for (int i = tid; i < npow2; i += kGroupThreads) {
        uint32_t key = 0u;
        uint64_t gid = ~0ull, page = ~0ull;
        if (i < m) {
            const uint32_t ky = score_key(srow[i]);
            const int64_t gi = grow[i];
            if (gi >= 0 && ky > kGroupNoneKey) key = ky, gid = (uint64_t)gi, page = (uint64_t)prow[i];
        }
        skey[i] = key;
        sgid[i] = gid;
        spage[i] = page;
    }
    group_sort<true>(skey, sgid, spage, npow2, tid);
    constexpr int kPer = kGroupSelectMaxM / kGroupThreads;
    bool head[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = tid + j * kGroupThreads;
        head[j] = i < npow2 && skey[i] != 0u && (i == 0 || sgid[i - 1] != sgid[i]);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int i = tid + j * kGroupThreads;
        if (i < npow2 && !head[j]) skey[i] = 0u, sgid[i] = ~0ull;
    }
    group_sort<false>(skey, sgid, spage, npow2, tid);
    for (int j = tid; j < k; j += kGroupThreads) {
        const bool valid = j < npow2 && skey[j] != 0u;
        const long long at = row * k + j;
        out_s[at] = valid ? key_score(skey[j]) : -INFINITY;
        out_g[at] = valid ? (int64_t)sgid[j] : -1;
        out_p[at] = valid ? (int64_t)spage[j] : -1;
    }
}

}  // namespace msim
