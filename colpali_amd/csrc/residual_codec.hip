// A residual-compressed copy of a packed corpus for gfx950 (MI355X): PLAID's second half.  Every corpus row is stored as the uint16
// id of its centroid (centroid_index.hip) plus `bits` (2 or 4) of residual per dimension, and candidate lists are reranked
// straight from those rows: no full-precision embedding is kept (include/maxsim.h: msim_res_*).
//   encode:  e_k = fl32(float(x_k) - float(C[c]_k));  bucket b_k = #{cutoffs t : t <= e_k};  dimension k is bits [k bits, k bits + bits)
//            of the row's 16 bits bytes, read as a little-endian bit string -- 8 consecutive k are one 16- / 32-bit field
//   decode:  xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k])     (one fp32 add, one rounding, no renormalisation)
//
// Kernels:
//   res_encode_kernel      one lane per (row, 8 dimensions): the row's 16 bytes, the same 16 bytes of its centroid row (from L2: K x 256 B
//                          is 64 .. 512 KiB), 8 subtractions and cutoff counts, one 2- / 4-byte field stored.  16 lanes read one row.
//   res_decode_kernel      the same mapping backwards over a row range; a row whose code is >= K decodes to NaN.
//   res_candidates_kernel  K1c's contract (maxsim_candidates.hip) over the compressed rows.  One WAVE per entry (q, j), grid-stride over
//                          the n_q x m entries, no inversion and no workspace beyond a status word: the query's 1 .. 8 units sit in
//                          registers (K1s's B operands), the page streams in 32-row slabs.  A slab never exists in HBM: lane
//                          (l4, l16) decodes the 16-byte chunk l16 of rows 4 i + l4 (i = 0 .. 7) in registers and stores it into the
//                          wave-private LDS slab at K1s's swizzled position (maxsim_common.hpp: slab_swizzled_off), so the operand
//                          fetch, the four-k-step fp32 MFMA chains, the exact max over rows (slab_units) and the token sum
//                          (reduce_query_tokens) are K1s's own: entry (q, j) has the bits msim_fwd_candidates gives the same query
//                          against the decoded page.  Up to kResPrefetchUnits query units, the centroid chunks and fields of slab
//                          s + 1 are in flight (40 registers) while the MFMAs of slab s run, and the codes of slab s + 2 behind them
//                          (1 register: lane r holds row r's code, handed round by ds_bpermute); with more units the 40 registers
//                          do not fit next to the query and the loads are issued at the top of the slab.  Rows past the page's end
//                          in the last slab re-read the page's last row and are masked to -inf behind the MFMAs (slab_units' tail
//                          form), never zero-filled.  The page loop (res_page_max) is shared with the full scan
//                          (residual_scan.hip), which keeps a group of queries resident and walks the shard's pages.
//   LDS per wave: 8 KiB slab + the per-token max table (kStreamTokBytes) + 64 B of weights = 10 368 B; 41 472 B per workgroup of four
//   waves.  Registers: up to 8 units x 16 query VGPRs + 32 operand + 32 accumulator (+ 40 in flight): launch bounds of two waves per
//   SIMD, 256 VGPRs; 4 VGPRs of per-lane constants sit in scratch, stored once at kernel start and reloaded outside the slab loops.
// Every index read from memory is checked before it becomes an address: a code against K (the page then scores NaN, others are
// untouched), page offsets against the row count, query offsets against the token count (status word + NaN over the call).
#pragma once
#include <type_traits>

#include "maxsim_common.hpp"
#include "maxsim_stream.hip"

namespace msim {

constexpr int kResChunks = kDim / 8;                       // 16-byte chunks (8 dimensions) per row
constexpr int kResLdsPerWave = kSlabBytes + kStreamTokBytes + 64;
constexpr int kResLdsBytes = 4 * kResLdsPerWave;
constexpr int kResPrefetchUnits = 5;                       // up to this many query units the next slab's loads fly under the MFMAs
constexpr int kResBadQuery = 1;                            // bit of the status word

template <bool F16>
__device__ __forceinline__ uint16_t res_to_elem(float v) {
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)v);
    else return __builtin_bit_cast(uint16_t, (__bf16)v);
}

// 8 dimensions of one row: centroid chunk + weights[bucket], rounded once
template <bool F16, int BITS, class W>
__device__ __forceinline__ bf16x8 res_decode_chunk(const bf16x8 &cc, uint32_t field, W &&weight) {
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = (field >> (j * BITS)) & ((1u << BITS) - 1);
        out[j] = (short)res_to_elem<F16>(elem_to_float<F16>((uint16_t)cc[j]) + weight(b));
    }
    return out;
}

template <int BITS>
__device__ __forceinline__ uint32_t res_load_field(const uint8_t *__restrict__ res, long long row, int chunk) {
    if constexpr (BITS == 2) return *reinterpret_cast<const uint16_t *>(res + row * 32 + chunk * 2);
    else return *reinterpret_cast<const uint32_t *>(res + row * 64 + chunk * 4);
}

// ---------------------------------------------------------------------------------------------------------------- encode
template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_encode_kernel(const uint16_t *__restrict__ X,        // [n_rows, 128]
                                                         const uint16_t *__restrict__ codes,    // [n_rows]
                                                         long long n_rows,
                                                         const uint16_t *__restrict__ C,        // [K, 128]
                                                         int K, const float *__restrict__ cutoffs,
                                                         uint8_t *__restrict__ res) {           // [n_rows, 16 BITS]
    constexpr int NC = (1 << BITS) - 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t >> 4;
    const int c = (int)(t & 15);
    if (row >= n_rows) return;
    float cut[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) cut[i] = cutoffs[i];
    const int code = codes[row];
    uint32_t field = 0;                                                 // a code >= K never becomes an address: all-zero buckets
    if (code < K) {
        const bf16x8 x = *reinterpret_cast<const bf16x8 *>(X + (size_t)row * kDim + c * 8);
        const bf16x8 cc = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kDim + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = elem_to_float<F16>((uint16_t)x[j]) - elem_to_float<F16>((uint16_t)cc[j]);
            uint32_t b = 0;
#pragma unroll
            for (int i = 0; i < NC; ++i) b += cut[i] <= e ? 1u : 0u;
            field |= b << (j * BITS);
        }
    }
    if constexpr (BITS == 2) *reinterpret_cast<uint16_t *>(res + row * 32 + c * 2) = (uint16_t)field;
    else *reinterpret_cast<uint32_t *>(res + row * 64 + c * 4) = field;
}

// ---------------------------------------------------------------------------------------------------------------- decode
template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_decode_kernel(const uint16_t *__restrict__ codes, const uint8_t *__restrict__ res,
                                                         long long row0, long long row1, const uint16_t *__restrict__ C, int K,
                                                         const float *__restrict__ weights,
                                                         uint16_t *__restrict__ out) {          // [row1 - row0, 128]
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = row0 + (t >> 4);
    const int c = (int)(t & 15);
    if (row >= row1) return;
    const int code = codes[row];
    bf16x8 v;
    if (code < K) {
        const bf16x8 cc = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kDim + c * 8);
        v = res_decode_chunk<F16, BITS>(cc, res_load_field<BITS>(res, row, c), [&](int b) { return weights[b]; });
    } else {
        const short nan = (short)(F16 ? 0x7e00 : 0x7fc0);
        v = bf16x8{nan, nan, nan, nan, nan, nan, nan, nan};
    }
    *reinterpret_cast<bf16x8 *>(out + (size_t)(row - row0) * kDim + c * 8) = v;
}

// ---------------------------------------------------------------------------------------------------------------- rerank
__device__ __forceinline__ void res_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct ResPage {                                    // one checked page: rows r0 .. r0 + len - 1 of the codes / residuals
    long long r0;
    int len;
};

// one page against NU resident query units, decoded slab by slab: mx[u] = the running maxima of unit u over this lane's rows
// (-inf for a page without rows).  Shared by the rerank (res_entry) and the scan (residual_scan.hip: res_scan_group).
template <int NU, bool F16, int BITS>
__device__ __forceinline__ void res_page_max(float (&mx)[NU], const QueryUnit (&qu)[NU], const uint16_t *__restrict__ codes,
                                             const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K, const ResPage &pg,
                                             bool &bad, char *slab, const float *wtab, const int (&rd_off)[2][kKSteps16], int lane) {
    const int l16 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int u = 0; u < NU; ++u) mx[u] = -INFINITY;

    const int len = pg.len;
    const int n_slabs = (len + kSlabRows - 1) / kSlabRows;
    // lane r (and r + 32) holds the code of slab row r; a row past the page's end names the page's last row
    auto load_codes = [&](int s) -> int {
        if (s >= n_slabs) return 0;
        const int r = s * kSlabRows + (lane & 31);
        return (int)codes[pg.r0 + (r < len ? r : len - 1)];
    };
    bf16x8 cc[8];
    uint32_t fld[8];
    auto issue_raw = [&](int s, int codev) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = 4 * i + l4;
            int code = __shfl(codev, row);
            if (code >= K) {                            // a broken code never becomes an address: the page scores NaN
                bad = true;
                code = 0;
            }
            const int pr = s * kSlabRows + row;
            const long long grow = pg.r0 + (pr < len ? pr : len - 1);
            cc[i] = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kDim + l16 * 8);
            fld[i] = res_load_field<BITS>(res, grow, l16);
        }
    };
    auto decode_store = [&]() {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = 4 * i + l4;
            const bf16x8 v = res_decode_chunk<F16, BITS>(cc[i], fld[i], [&](int b) { return wtab[b]; });
            *reinterpret_cast<bf16x8 *>(slab + slab_swizzled_off(row, l16)) = v;
        }
    };
    int code_next = 0;
    if (NU <= kResPrefetchUnits && n_slabs > 0) {
        const int code0 = load_codes(0);
        code_next = load_codes(1);
        issue_raw(0, code0);
    }
    auto body = [&](auto tail_c, int s, int rows_left) {
        constexpr bool kTail = decltype(tail_c)::value;
        if constexpr (NU > kResPrefetchUnits) issue_raw(s, load_codes(s));   // 7 and 8 units leave no 40 registers next to the MFMAs
        decode_store();
        if constexpr (NU <= kResPrefetchUnits) {                 // in flight behind this slab's MFMAs
            if (s + 1 < n_slabs) issue_raw(s + 1, code_next);
            code_next = load_codes(s + 2);
        }
        res_wave_sync();
        bf16x8 af[2][kKSteps16];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int ks = 0; ks < kKSteps16; ++ks) af[g][ks] = *reinterpret_cast<const bf16x8 *>(slab + rd_off[g][ks]);
        slab_units<F16, NU, kTail, true>(mx, af, qu, rows_left, lane, [](int) {});
        res_wave_sync();                                        // the operands are in registers before the next slab is stored
    };
    const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
    for (int s = 0; s < n_full; ++s) body(std::false_type{}, s, kSlabRows);
    if (rem > 0) body(std::true_type{}, n_full, rem);
}

// the score of one entry: the query's NU units against the page.  Returns in lanes 0 .. 7; lane 0 stores.
template <int NU, bool F16, int BITS>
__device__ __forceinline__ float res_entry(const uint16_t *__restrict__ Qt, int qs, int qe, const uint16_t *__restrict__ codes,
                                           const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K, const ResPage &pg,
                                           bool clamp, bool &bad, char *slab, char *tokmax, const float *wtab,
                                           const int (&rd_off)[2][kKSteps16], int lane) {
    QueryUnit qu[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) load_query_unit(qu[u], Qt, qs + u * kUnitTok, qe, lane, true);
    float mx[NU];
    res_page_max<NU, F16, BITS>(mx, qu, codes, res, C, K, pg, bad, slab, wtab, rd_off, lane);

#pragma unroll
    for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], lane);
    res_wave_sync();
    float tot = 0.0f;
    if (lane < 8) tot = reduce_query_tokens<F16>(tokmax, 0, qe - qs, lane, clamp, false);
    res_wave_sync();                                            // the sums have read the table before the next entry writes it
    return tot;
}

template <bool F16, int BITS>
__global__ __launch_bounds__(256, 2) void res_candidates_kernel(const uint16_t *__restrict__ Qt,       // [q_rows, 128] flat query tokens
                                                                const int32_t *__restrict__ q_off,    // [n_q + 1]
                                                                int n_q, long long q_rows,
                                                                const uint16_t *__restrict__ codes,   // [d_rows]
                                                                const uint8_t *__restrict__ res,      // [d_rows, 16 BITS]
                                                                const uint16_t *__restrict__ C,       // [K, 128]
                                                                int K, const float *__restrict__ weights,
                                                                const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                                const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                                int n_d, long long d_rows,
                                                                const int64_t *__restrict__ cand, long long ld_cand, int m,
                                                                long long id_base, float *__restrict__ scores, long long ld,
                                                                int64_t *__restrict__ out_ids, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slab = smem + wave * kResLdsPerWave;
    char *tokmax = slab + kSlabBytes;
    float *wtab = reinterpret_cast<float *>(tokmax + kStreamTokBytes);
    if (lane < (1 << BITS)) wtab[lane] = weights[lane];
    res_wave_sync();
    int rd_off[2][kKSteps16];
    slab_rd_offsets16(lane, rd_off);

    const long long E = (long long)n_q * m;
    const long long GW = (long long)gridDim.x * 4;
    for (long long e = (long long)blockIdx.x * 4 + wave; e < E; e += GW) {
        const int q = (int)(e / m), j = (int)(e - (long long)q * m);
        const int64_t id = cand[(size_t)q * ld_cand + j];
        const long long dl = (long long)id - id_base;
        const bool valid = id >= 0 && dl >= 0 && dl < n_d;
        if (out_ids && lane == 0) out_ids[(size_t)q * ld + j] = valid ? id : -1;
        float *dst = scores + (size_t)q * ld + j;
        if (!valid) {
            if (lane == 0) *dst = -INFINITY;
            continue;
        }
        const int d = __builtin_amdgcn_readfirstlane((int)dl);
        const long long qs = q_off[q], qe = q_off[q + 1];
        if (qs < 0 || qe < qs || qe > q_rows || qe - qs > kStreamMaxUnits * kUnitTok) {     // the host validated another q_off
            if (lane == 0) {
                atomicOr(status, kResBadQuery);
                *dst = __builtin_nanf("");
            }
            continue;
        }
        const int len_q = __builtin_amdgcn_readfirstlane((int)(qe - qs));
        if (len_q == 0) {                                       // a sum over no tokens: what every scorer returns for it
            if (lane == 0) *dst = 0.0f;
            continue;
        }
        const long long r0 = d_off[d], r1 = d_off[d + 1];
        if (r0 < 0 || r1 < r0 || r1 > d_rows) {                 // never trust a device offset with an address
            if (lane == 0) *dst = __builtin_nanf("");
            continue;
        }
        ResPage pg;
        pg.r0 = r0;
        pg.len = __builtin_amdgcn_readfirstlane((int)(r1 - r0));
        const bool clamp = clamp0 != nullptr && clamp0[d] != 0;
        bool bad = false;
        float tot = 0.0f;
        switch ((len_q + kUnitTok - 1) / kUnitTok) {
#define MSIM_RES_CASE(U) \
            case U: tot = res_entry<U, F16, BITS>(Qt, (int)qs, (int)qe, codes, res, C, K, pg, clamp, bad, slab, tokmax, wtab, rd_off, lane); break;
            MSIM_RES_CASE(1)
            MSIM_RES_CASE(2)
            MSIM_RES_CASE(3)
            MSIM_RES_CASE(4)
            MSIM_RES_CASE(5)
            MSIM_RES_CASE(6)
            MSIM_RES_CASE(7)
            MSIM_RES_CASE(8)
#undef MSIM_RES_CASE
            default: break;
        }
        const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        if (lane == 0) *dst = any_bad ? __builtin_nanf("") : tot;
    }
}

// the status word starts at zero: a kernel, not a memset node (maxsim_candidates.hip: cand_zero_kernel)
__global__ void res_zero_status_kernel(int32_t *__restrict__ status) {
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// a device q_off that disagrees with the host copy: every score of the call becomes NaN
__global__ __launch_bounds__(256) void res_poison_kernel(const int32_t *__restrict__ status, int n_q, int m, float *__restrict__ scores,
                                                         long long ld) {
    if (*status == 0) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_q * m) return;
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    scores[(size_t)q * ld + j] = __builtin_nanf("");
}

}  // namespace msim
