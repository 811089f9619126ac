// The full scan of a residual-compressed shard for gfx950 (MI355X): scores[q, c] for every query and every page, straight from the
// compressed rows (include/maxsim.h: msim_res_scores).  K1s's shape (maxsim_stream.hip) with the loader of the residual rerank
// (residual_codec.hip: res_page_max): a wave holds a GROUP of consecutive queries in registers as the MFMA B operand and walks
// pages of its own (gw, gw + GW, ...), so a page is decoded once per group, not once per (query, page) entry.
//
// Kernels:
//   res_scan_groups_kernel  one wave: the group table, greedily from the DEVICE q_off.  A group is a run of consecutive queries of
//                           at most kResScanGroupQueries queries (8 reduction lanes each) whose tokens span at most `cap_units`
//                           16-token units of the flat token matrix from the group's first token on; one query alone may exceed
//                           the cap (never 8 units).  Every offset is checked (0 <= length <= 128, inside the token matrix) and
//                           the group count is compared with the count the host derived from q_off_host by the same rule: any
//                           disagreement sets the status word.  It also initialises the status words (no memset node).
//   res_scan_kernel         persistent grid, two workgroups per CU, one wave = one pipeline.  Per group: the units into registers,
//                           the queries' token ranges into the 64 B behind the wave's per-token max table; per page: offsets
//                           checked, res_page_max (decode in registers -> swizzled LDS slab -> operand fetch -> slab_units, the tail
//                           form for the last slab: rows past the page's end re-read its last row and are masked, never
//                           zero-filled), store_token_max, then 8 lanes per query run reduce_query_tokens over that query's token
//                           range and one lane stores scores[q, c].  The MFMA chain of a token does not depend on the column it
//                           sits in and reduce_query_tokens is a pure function of the token values and the query's length, so
//                           the bits do not depend on the grouping: entry (q, c) has the bits msim_fwd_ragged gives the same
//                           query against the decoded page.
//   res_scan_poison_kernel  a set status word: every score of the call becomes NaN.
// LDS and launch bounds are res_candidates_kernel's (kResLdsPerWave per wave, 256 threads, two waves per SIMD).  Every index read
// from memory is checked before it becomes an address: codes against K and page offsets against the row count (that page scores
// NaN, no other column changes), query offsets in the prologue, the group table again where it is read.
#pragma once
#include "residual_codec.hip"
#include "residual_scan_groups.hpp"

namespace msim {

constexpr int kResScanGroupUnits = kStreamMaxUnits;       // token cap of a group, in 16-token units (above kResPrefetchUnits the slab
                                                          // loads are issued at the top of the slab: DESIGN.md section 3.18)

// the group table and the greedy rule: residual_scan_groups.hpp (shared with the scan at width 320)
__global__ __launch_bounds__(64) void res_scan_groups_kernel(const int32_t *__restrict__ q_off, int n_q, long long q_rows, int cap_units,
                                                             int n_groups_host, ResScanGroup *__restrict__ groups,
                                                             int32_t *__restrict__ status) {
    const int lane = threadIdx.x;
    bool bad = false;
    int g = 0, cur_q0 = 0, cur_nq = 0, cur_tok0 = 0, prev = 0;
    if (q_off[0] != 0) bad = true;
    auto emit = [&]() {
        if (lane == 0 && g < n_q) groups[g] = ResScanGroup{cur_q0, cur_nq, cur_tok0, prev};
        ++g;
    };
    for (int base = 0; base < n_q && !bad; base += 64) {       // 64 offsets per load, handed round by readlane: wave-uniform control flow
        const int idx = base + 1 + lane;
        const int v = idx <= n_q ? q_off[idx] : 0;
        const int cnt = n_q - base < 64 ? n_q - base : 64;
        for (int i = 0; i < cnt; ++i) {
            const int e = __shfl(v, i);
            const long long len = (long long)e - prev;
            if (len < 0 || len > kStreamMaxUnits * kUnitTok || e > q_rows) {
                bad = true;
                break;
            }
            if (res_scan_new_group(cur_nq, cur_tok0, e, cap_units)) {
                emit();
                cur_q0 = base + i;
                cur_nq = 0;
                cur_tok0 = prev;
            }
            ++cur_nq;
            prev = e;
        }
    }
    if (!bad && cur_nq > 0) emit();
    if (g != n_groups_host) bad = true;                         // the host validated another q_off
    if (lane < 4) status[lane] = lane == 0 ? (bad ? kResBadQuery : 0) : lane == 1 ? g : 0;
}

// one group against this wave's pages
template <int NU, bool F16, int BITS>
__device__ __forceinline__ void res_scan_group(const uint16_t *__restrict__ Qt, const ResScanGroup &gr, const uint16_t *__restrict__ codes,
                                               const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K,
                                               const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                               long long d_rows, float *__restrict__ scores, long long ld, char *slab, char *tokmax,
                                               const float *wtab, const int (&rd_off)[2][kKSteps16], int lane, long long gw, long long GW) {
    QueryUnit qu[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) load_query_unit(qu[u], Qt, gr.tok0 + u * kUnitTok, gr.tok1, lane, true);
    const int *rtab = reinterpret_cast<const int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    for (long long c = gw; c < n_d; c += GW) {
        const long long r0 = d_off[c], r1 = d_off[c + 1];
        bool bad = r0 < 0 || r1 < r0 || r1 > d_rows;            // never trust a device offset with an address
        ResPage pg;
        pg.r0 = bad ? 0 : r0;
        pg.len = __builtin_amdgcn_readfirstlane(bad ? 0 : (int)(r1 - r0));
        const bool clamp = clamp0 != nullptr && clamp0[c] != 0;
        float mx[NU];
        res_page_max<NU, F16, BITS>(mx, qu, codes, res, C, K, pg, bad, slab, wtab, rd_off, lane);
#pragma unroll
        for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], lane);
        res_wave_sync();
        const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        int ln = lane;
        asm volatile("" : "+v"(ln));                            // opaque: nothing derived from the lane id stays live across the slab loop
        const int rq = ln >> 3, ri = ln & 7;
        if (rq < gr.nq) {
            const int s = rtab[2 * rq], e = rtab[2 * rq + 1];
            float tot = reduce_query_tokens<F16>(tokmax, s, e, ri, clamp, false);
            if (any_bad && e > s) tot = __builtin_nanf("");     // a query of 0 tokens read no page: it keeps its 0
            if (ri == 0) scores[(size_t)(gr.q0 + rq) * ld + c] = tot;
        }
        res_wave_sync();                                        // the sums have read the table before the next page writes it
    }
}

template <bool F16, int BITS>
__global__ __launch_bounds__(256, 2) void res_scan_kernel(const uint16_t *__restrict__ Qt,       // [q_rows, 128] flat query tokens
                                                          const int32_t *__restrict__ q_off,    // [n_q + 1]
                                                          int n_q, long long q_rows,
                                                          const uint16_t *__restrict__ codes,   // [d_rows]
                                                          const uint8_t *__restrict__ res,      // [d_rows, 16 BITS]
                                                          const uint16_t *__restrict__ C,       // [K, 128]
                                                          int K, const float *__restrict__ weights,
                                                          const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                          const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                          int n_d, long long d_rows, float *__restrict__ scores, long long ld,
                                                          const ResScanGroup *__restrict__ groups, int n_groups,
                                                          int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (*status != 0) return;                                   // a q_off the host did not validate: the poison kernel writes the scores
    char *slab = smem + wave * kResLdsPerWave;
    char *tokmax = slab + kSlabBytes;
    int *rtab = reinterpret_cast<int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    float *wtab = reinterpret_cast<float *>(tokmax + kStreamTokBytes);
    if (lane < (1 << BITS)) wtab[lane] = weights[lane];
    res_wave_sync();
    int rd_off[2][kKSteps16];
    slab_rd_offsets16(lane, rd_off);

    const long long gw = (long long)blockIdx.x * 4 + wave;
    const long long GW = (long long)gridDim.x * 4;
    for (int g = 0; g < n_groups; ++g) {
        ResScanGroup gr = groups[g];
        gr.q0 = __builtin_amdgcn_readfirstlane(gr.q0);
        gr.nq = __builtin_amdgcn_readfirstlane(gr.nq);
        gr.tok0 = __builtin_amdgcn_readfirstlane(gr.tok0);
        gr.tok1 = __builtin_amdgcn_readfirstlane(gr.tok1);
        const int n_tok = gr.tok1 - gr.tok0;
        if (gr.q0 < 0 || gr.nq < 1 || gr.nq > kResScanGroupQueries || gr.nq > n_q - gr.q0 || gr.tok0 < 0 || gr.tok1 < gr.tok0 ||
            gr.tok1 > q_rows || n_tok > kStreamMaxUnits * kUnitTok) {   // the table is the prologue's: checked again before it addresses
            if (lane == 0) atomicOr(status, kResBadQuery);
            continue;
        }
        // the queries' token ranges inside the group, written by the lanes that read them back; clamped to the table
        if ((lane >> 3) < gr.nq) {
            int s = q_off[gr.q0 + (lane >> 3)] - gr.tok0, e = q_off[gr.q0 + (lane >> 3) + 1] - gr.tok0;
            s = s < 0 ? 0 : s > n_tok ? n_tok : s;
            e = e < s ? s : e > n_tok ? n_tok : e;
            rtab[2 * (lane >> 3)] = s;
            rtab[2 * (lane >> 3) + 1] = e;
        }
        res_wave_sync();
        switch ((n_tok + kUnitTok - 1) / kUnitTok) {
#define MSIM_RES_SCAN_CASE(U) \
            case U: res_scan_group<U, F16, BITS>(Qt, gr, codes, res, C, K, d_off, clamp0, n_d, d_rows, scores, ld, slab, tokmax, wtab, rd_off, lane, gw, GW); break;
            MSIM_RES_SCAN_CASE(1)
            MSIM_RES_SCAN_CASE(2)
            MSIM_RES_SCAN_CASE(3)
            MSIM_RES_SCAN_CASE(4)
            MSIM_RES_SCAN_CASE(5)
            MSIM_RES_SCAN_CASE(6)
            MSIM_RES_SCAN_CASE(7)
            MSIM_RES_SCAN_CASE(8)
#undef MSIM_RES_SCAN_CASE
            default:                                            // only queries of 0 tokens: a sum over no tokens, no page is read
                for (long long c = gw; c < n_d; c += GW)
                    if ((lane & 7) == 0 && (lane >> 3) < gr.nq) scores[(size_t)(gr.q0 + (lane >> 3)) * ld + c] = 0.0f;
                break;
        }
    }
}

// a device q_off that disagrees with the host copy: every score of the call becomes NaN
__global__ __launch_bounds__(256) void res_scan_poison_kernel(const int32_t *__restrict__ status, int n_q, int n_d,
                                                              float *__restrict__ scores, long long ld) {
    if (*status == 0) return;
    const long long E = (long long)n_q * n_d;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long q = e / n_d;
        scores[(size_t)q * ld + (e - q * n_d)] = __builtin_nanf("");
    }
}

}  // namespace msim
