// The full scan of a residual-compressed shard at width 320 (ColQwen3) for gfx950 (MI355X): scores[q, c] for every query and every
// page, straight from the compressed rows (include/maxsim.h: msim_res_wide_scores).  residual_scan.hip's shape at the budget of the
// wide rerank (residual_wide.hip: rw_page_max): a wave holds a GROUP of consecutive queries in registers as the MFMA B operand and
// walks pages of its own (gw, gw + GW, ...), so a page is decoded once per group, not once per (query, page) entry.
//
// Kernels:
//   res_wide_scan_groups_kernel  res_scan_groups_kernel's copy in this unit: the group table, greedily from the DEVICE q_off (at most 8
//                           queries and `cap_units` 16-token units per group; one query alone may reach 8 units), every offset
//                           checked, the group count compared with the host's, the status words initialised (no memset node).
//   res_wide_scan_kernel    persistent grid, ONE workgroup of four waves per CU (kRwLdsBytes of LDS, a wave alone on its SIMD with
//                           the unified 512 registers), one wave = one pipeline.  Per group: the table's fields checked again, the
//                           1 .. 8 units into registers once (a token at or past tok1 is a zero row), the queries' clamped token
//                           ranges into the 64 B behind the wave's per-token max table; per page: offsets checked against d_rows,
//                           rw_page_max (decode into three panel-slabs -> operand fetch -> one fp32 chain over p = 0, 1, 2 with ks
//                           ascending -> tail mask -> exact max), store_token_max, then 8 lanes per query run reduce_query_tokens
//                           over that query's token range and one lane stores scores[q, c].  The MFMA chain of a token does not
//                           depend on the column it sits in and reduce_query_tokens is a pure function of the token values and the
//                           query's length, so the bits do not depend on the grouping: entry (q, c) has the bits
//                           res_wide_candidates_kernel gives the same query against page c.
//   res_wide_scan_poison_kernel  a set status word: every score of the call becomes NaN.
// Every index read from memory is checked before it becomes an address: codes against K and page offsets against the row count (that
// page scores NaN for every query that has tokens, no other column changes), query offsets in the prologue, the group table again
// where it is read.  All row addressing is 64-bit.  Nothing allocates or synchronises; no float atomics.
#pragma once
#include "residual_scan_groups.hpp"
#include "residual_wide.hip"

namespace msim {

constexpr int kRwScanGroupUnits = kStreamMaxUnits;        // token cap of a group, in 16-token units: four 32-token queries are one pass

__global__ __launch_bounds__(64) void res_wide_scan_groups_kernel(const int32_t *__restrict__ q_off, int n_q, long long q_rows,
                                                                  int cap_units, int n_groups_host, ResScanGroup *__restrict__ groups,
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
    if (lane < 4) status[lane] = lane == 0 ? (bad ? kRwBadQuery : 0) : lane == 1 ? g : 0;
}

// one group against this wave's pages
template <int NU, bool F16, int BITS>
__device__ __forceinline__ void rw_scan_group(const uint16_t *__restrict__ Qt, const ResScanGroup &gr, const uint16_t *__restrict__ codes,
                                              const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K,
                                              const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                              long long d_rows, float *__restrict__ scores, long long ld, char *slabs, int lane,
                                              long long gw, long long GW) {
    char *tokmax = slabs + kRwPanels * kSlabBytes;
    const int *rtab = reinterpret_cast<const int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    const float *wtab = reinterpret_cast<const float *>(tokmax + kStreamTokBytes);
    // the group's units: K1cP's B operands, [unit][k-step of 32], resident across the page loop
    bf16x8 qf[NU][kRwKSteps];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int row = gr.tok0 + u * kUnitTok + (lane & 15);
        const bool valid = row < gr.tok1;
        const uint16_t *p = Qt + (size_t)(valid ? row : 0) * kRwDim + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < kRwKSteps; ++ks) {
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
            qf[u][ks] = valid ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    for (long long c = gw; c < n_d; c += GW) {
        const long long r0 = d_off[c], r1 = d_off[c + 1];
        bool bad = r0 < 0 || r1 < r0 || r1 > d_rows;            // never trust a device offset with an address
        const long long p0 = bad ? 0 : r0;
        const int len = __builtin_amdgcn_readfirstlane(bad ? 0 : (int)(r1 - r0));
        const bool clamp = clamp0 != nullptr && clamp0[c] != 0;
        int ln = lane;
        asm volatile("" : "+v"(ln));                            // opaque: nothing derived from the lane id stays live across the pages
        int rd_off[2][kKSteps16];                               // per page, as the rerank's are per entry
        slab_rd_offsets16(ln, rd_off);
        float mx[NU];
        rw_page_max<NU, F16, BITS>(mx, qf, codes, res, C, K, p0, len, bad, slabs, wtab, rd_off, ln);
#pragma unroll
        for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], ln);
        rw_wave_sync();
        const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        const int rq = ln >> 3, ri = ln & 7;
        if (rq < gr.nq) {
            const int s = rtab[2 * rq], e = rtab[2 * rq + 1];
            float tot = reduce_query_tokens<F16>(tokmax, s, e, ri, clamp, false);
            if (any_bad && e > s) tot = __builtin_nanf("");     // a query of 0 tokens read no page: it keeps its 0
            if (ri == 0) scores[(size_t)(gr.q0 + rq) * ld + c] = tot;
        }
        rw_wave_sync();                                         // the sums have read the table before the next page writes it
    }
}

// one wave per SIMD (no second launch bound): eight resident units are 320 operand registers of the unified 512
template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_wide_scan_kernel(const uint16_t *__restrict__ Qt,        // [q_rows, 320] flat query tokens
                                                            const int32_t *__restrict__ q_off,     // [n_q + 1]
                                                            int n_q, long long q_rows,
                                                            const uint16_t *__restrict__ codes,    // [d_rows]
                                                            const uint8_t *__restrict__ res,       // [d_rows, 40 BITS]
                                                            const uint16_t *__restrict__ C,        // [K, 320]
                                                            int K, const float *__restrict__ weights,
                                                            const int32_t *__restrict__ d_off,     // [n_d + 1]
                                                            const uint8_t *__restrict__ clamp0,    // [n_d] or null
                                                            int n_d, long long d_rows, float *__restrict__ scores, long long ld,
                                                            const ResScanGroup *__restrict__ groups, int n_groups,
                                                            int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (*status != 0) return;                                   // a q_off the host did not validate: the poison kernel writes the scores
    char *slabs = smem + wave * kRwLdsPerWave;
    char *tokmax = slabs + kRwPanels * kSlabBytes;
    int *rtab = reinterpret_cast<int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    float *wtab = reinterpret_cast<float *>(tokmax + kStreamTokBytes);
    if (lane < (1 << BITS)) wtab[lane] = weights[lane];
    rw_wave_sync();

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
            if (lane == 0) atomicOr(status, kRwBadQuery);
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
        rw_wave_sync();
        switch ((n_tok + kUnitTok - 1) / kUnitTok) {
#define MSIM_RW_SCAN_CASE(U) \
            case U: rw_scan_group<U, F16, BITS>(Qt, gr, codes, res, C, K, d_off, clamp0, n_d, d_rows, scores, ld, slabs, lane, gw, GW); break;
            MSIM_RW_SCAN_CASE(1)
            MSIM_RW_SCAN_CASE(2)
            MSIM_RW_SCAN_CASE(3)
            MSIM_RW_SCAN_CASE(4)
            MSIM_RW_SCAN_CASE(5)
            MSIM_RW_SCAN_CASE(6)
            MSIM_RW_SCAN_CASE(7)
            MSIM_RW_SCAN_CASE(8)
#undef MSIM_RW_SCAN_CASE
            default:                                            // only queries of 0 tokens: a sum over no tokens, no page is read
                for (long long c = gw; c < n_d; c += GW)
                    if ((lane & 7) == 0 && (lane >> 3) < gr.nq) scores[(size_t)(gr.q0 + (lane >> 3)) * ld + c] = 0.0f;
                break;
        }
        rw_wave_sync();                                         // the sums have read the ranges before the next group writes them
    }
}

// a device q_off that disagrees with the host copy: every score of the call becomes NaN
__global__ __launch_bounds__(256) void res_wide_scan_poison_kernel(const int32_t *__restrict__ status, int n_q, int n_d,
                                                                   float *__restrict__ scores, long long ld) {
    if (*status == 0) return;
    const long long E = (long long)n_q * n_d;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long long)gridDim.x * 256) {
        const long long q = e / n_d;
        scores[(size_t)q * ld + (e - q * n_d)] = __builtin_nanf("");
    }
}

}  // namespace msim
