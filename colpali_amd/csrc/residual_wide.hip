// The residual-compressed shard at width 320 (ColQwen3) for gfx950 (MI355X): the centroid-code first stage and PLAID's second half
// over rows of 640 bytes (include/maxsim.h: msim_cent_wide_*, msim_res_wide_*).  The contracts are those of centroid_index.hip and
// residual_codec.hip with 320 for 128:
//   encode:  code[r]  = argmax_k <row_r, C_k>      one fp32 chain of ten v_mfma_f32_16x16x32 from zero, k-steps ascending; the lowest k
//                                                  wins equal values
//   table:   S[i, k]  = fp16(fl32 <q_i, C_k>)      the same chain, rounded once; the table[n_q * nb][K][32] layout of msim_cent_table,
//                                                  so the scan (cent_scores_kernel) serves both widths and no scan kernel is added
//   codec:   e_k = fl32(float(x_k) - float(C[c]_k));  bucket b_k = #{cutoffs t : t <= e_k};  dimension k is bits [k bits, k bits + bits) of
//            the row's 40 bits bytes, a little-endian bit string (80 B at 2 bits, 160 B at 4): 8 consecutive k are one 16- / 32-bit field
//            xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k])      (one fp32 add, one rounding, no renormalisation)
//
// Kernels:
//   cent_wide_encode_kernel   cent_encode_kernel with ten k-steps.  Its four row tiles per wave would be 160 operand VGPRs beside the 80
//                             of the two centroid tiles in flight, so a wave keeps TWO tiles of 16 page rows (80 VGPRs) and a workgroup
//                             covers 128 rows: 160 operand VGPRs, two waves per SIMD.
//   cent_wide_table_kernel    cent_table_kernel with ten k-steps: the block's two 16-token tiles (80 VGPRs) against one centroid tile (40).
//   res_wide_encode_kernel /  one lane per (row, 8 dimensions): 40 lanes per row.
//   res_wide_decode_kernel
//   res_wide_candidates_kernel  res_candidates_kernel's shape -- one WAVE per entry (q, j), grid-stride over n_q x m, the query's 1 .. 8
//                             units in registers, no inversion, no workspace beyond a status word -- with K1cP's arithmetic
//                             (maxsim_candidates_panels.hip).  A 32-row slab of a page is decoded in registers into three wave-private
//                             panel-slabs (dimensions 0 .. 127, 128 .. 255, 256 .. 319), each the LDS image of a width-128 slab
//                             (slab_swizzled_off; the third holds chunks 0 .. 7 of every row), so the operand fetch is K1cP's.  Per
//                             (slab, unit) ONE fp32 accumulator from zero runs across the panels p = 0, 1, 2 with ks ascending in each
//                             (4 + 4 + 2 k-steps of 32), then the tail mask (rows past the page's end re-read the page's last row and
//                             are set to -inf behind the MFMAs, never zero-filled), the exact max over rows and reduce_query_tokens:
//                             entry (q, j) has the bits msim_fwd_candidates_wide gives the query against the decoded page.  The
//                             page loop is rw_page_max, shared with the full scan (residual_wide_scan.hip).
//   LDS per wave: 3 x 8 KiB panel-slabs + the per-token max table (kStreamTokBytes) + 64 B of weights = 26 752 B; 107 008 B per
//   workgroup of four waves, one workgroup per CU.  Registers: up to 8 units x 40 query VGPRs = 320, so a wave runs alone on its SIMD
//   with the unified 512-register file (__launch_bounds__(256) and no second bound), as K1cP.  hipcc reports 256 + 256 registers and
//   360 B of scratch per lane: the eight-unit form parks 12 query fragments while an entry is set up (back in registers before its
//   slab loop), and a few lane-derived constants live in scratch across the unit switch; the slab loops of 4 and 5 units reload 1 - 3
//   of them per slab, the other loops touch no scratch.
// Every index read from memory is checked before it becomes an address: a code against K (the page then scores NaN, others are
// untouched), page offsets against the row count, query offsets against the token count (status word + NaN over the call).  All row
// addressing is 64-bit (row * 80, row * 160, row * 320 elements).  Nothing allocates or synchronises; no float atomics.
#pragma once
#include <type_traits>

#include "maxsim_common.hpp"
#include "maxsim_stream.hip"

namespace msim {

constexpr int kRwDim = 320;                                // the row width of this file
constexpr int kRwKSteps = kRwDim / 32;                     // 10 k-steps of 32
constexpr int kRwChunks = kRwDim / 8;                      // 40 16-byte chunks (8 dimensions) per row
constexpr int kRwPanels = 3;                               // panels of 128 dimensions; the last holds 64
constexpr int kRwLastKSteps = kRwKSteps - 2 * kKSteps16;   // 2 k-steps of 32 in the last panel
constexpr int kRwMinK = 256, kRwMaxK = 2048;
constexpr int kRwMaxTokens = 128;
constexpr int kRwBlockTok = 32;                            // query tokens per table block (centroid_index.hip: kCentBlockTok)
constexpr int kRwEncTiles = 2;                             // 16-row tiles per encode wave
constexpr int kRwEncRows = 4 * kRwEncTiles * 16;           // page rows per encode workgroup: 128
constexpr int kRwLdsPerWave = kRwPanels * kSlabBytes + kStreamTokBytes + 64;
constexpr int kRwLdsBytes = 4 * kRwLdsPerWave;
constexpr int kRwBadQuery = 1;                             // bit of the status word

typedef _Float16 rw_h4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- centroid encode
template <bool F16>
__global__ __launch_bounds__(256, 2) void cent_wide_encode_kernel(const uint16_t *__restrict__ X,       // [n_rows, 320]
                                                                  const int32_t *__restrict__ off,     // [n_d + 1]
                                                                  int n_d, long long n_rows, int max_doc_rows,
                                                                  const uint16_t *__restrict__ C,       // [K, 320]
                                                                  int K, uint16_t *__restrict__ codes,  // [n_rows]
                                                                  int32_t *__restrict__ status) {       // [n_d] or null
    constexpr int KS = kRwKSteps;
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
    const int row_base = blockIdx.y * kRwEncRows + wave * (kRwEncTiles * 16);
    if (row_base >= len) return;

    // the wave's rows: B operands of up to 2 tiles (a row past the page's end reads the page's last row and is never stored)
    bf16x8 xf[kRwEncTiles][KS];
    bool live[kRwEncTiles];
#pragma unroll
    for (int t = 0; t < kRwEncTiles; ++t) {
        live[t] = row_base + t * 16 < len;                             // wave-uniform
        int row = row_base + t * 16 + l16;
        row = row < len ? row : len - 1;
        const uint16_t *src = X + (size_t)(r0 + row) * kRwDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[t][ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
    }
    float bs[kRwEncTiles];
    int bk[kRwEncTiles];
#pragma unroll
    for (int t = 0; t < kRwEncTiles; ++t) {
        bs[t] = -INFINITY;
        bk[t] = -1;
    }

    auto load_tile = [&](bf16x8 (&cf)[KS], int c) {                     // centroids 16 c .. 16 c + 15 (K is a multiple of 16)
        const uint16_t *src = C + (size_t)(c * 16 + l16) * kRwDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cf[ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
    };
    auto tile = [&](const bf16x8 (&cf)[KS], int c) {
        const int k0 = c * 16 + 4 * l4;                                 // D: lane holds row l16 against centroids k0 .. k0 + 3
#pragma unroll
        for (int t = 0; t < kRwEncTiles; ++t) {
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

#pragma unroll
    for (int t = 0; t < kRwEncTiles; ++t) {
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
        if (l4 == 0 && row < len) codes[r0 + row] = (uint16_t)(bk[t] < 0 ? 0 : bk[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- centroid table
// table [n_q * nb][K][32] fp16: block b of query q holds its tokens 32 b .. 32 b + 31 (0 for a token the query does not have)
template <bool F16>
__global__ __launch_bounds__(256) void cent_wide_table_kernel(const uint16_t *__restrict__ Qt,      // [q_rows, 320] flat query tokens
                                                              const int32_t *__restrict__ q_off,   // [n_q + 1]
                                                              int n_q, long long q_rows, int nb,
                                                              const uint16_t *__restrict__ C,      // [K, 320]
                                                              int K, _Float16 *__restrict__ table) {
    constexpr int KS = kRwKSteps;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l16 = lane & 15, l4 = lane >> 4;
    const int blk = blockIdx.x, q = blk / nb, b = blk - q * nb;
    if (q >= n_q) return;
    const long long qs = q_off[q], qe = q_off[q + 1];
    const bool ok = qs >= 0 && qe >= qs && qe <= q_rows && qe - qs <= (long long)nb * kRwBlockTok;
    const int len = ok ? (int)(qe - qs) : 0;

    bf16x8 qf[2][KS];                                                   // A: the block's two 16-token tiles
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int tok = b * kRwBlockTok + h * 16 + l16;
        const bool valid = tok < len;
        const uint16_t *src = Qt + (size_t)(valid ? qs + tok : 0) * kRwDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[h][ks] = valid ? *reinterpret_cast<const bf16x8 *>(src + ks * 32) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    _Float16 *out = table + (size_t)blk * K * kRwBlockTok;
    const int k_base = blockIdx.y * 256 + wave * 64;                    // 64 centroids per wave: 4 tiles (K is a multiple of 256)
#pragma unroll 1
    for (int c = 0; c < 4; ++c) {
        const int k = k_base + c * 16 + l16;
        const uint16_t *src = C + (size_t)k * kRwDim + l4 * 8;
        bf16x8 cf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cf[ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma16<F16>(qf[h][ks], cf[ks], acc);      // one chain, k ascending
            // D: lane holds centroid k against tokens 16 h + 4 l4 + {0 .. 3}
            const rw_h4 v = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
            *reinterpret_cast<rw_h4 *>(out + (size_t)k * kRwBlockTok + h * 16 + 4 * l4) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the codec
template <bool F16>
__device__ __forceinline__ uint16_t rw_to_elem(float v) {
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)v);
    else return __builtin_bit_cast(uint16_t, (__bf16)v);
}

// 8 dimensions of one row: centroid chunk + weights[bucket], rounded once
template <bool F16, int BITS, class W>
__device__ __forceinline__ bf16x8 rw_decode_chunk(const bf16x8 &cc, uint32_t field, W &&weight) {
    bf16x8 out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int b = (field >> (j * BITS)) & ((1u << BITS) - 1);
        out[j] = (short)rw_to_elem<F16>(elem_to_float<F16>((uint16_t)cc[j]) + weight(b));
    }
    return out;
}

// the field of chunk `chunk` (0 .. 39) of row `row`: 64-bit addressing, row * 80 or row * 160 bytes
template <int BITS>
__device__ __forceinline__ uint32_t rw_load_field(const uint8_t *__restrict__ res, long long row, int chunk) {
    if constexpr (BITS == 2) return *reinterpret_cast<const uint16_t *>(res + row * (kRwChunks * 2) + chunk * 2);
    else return *reinterpret_cast<const uint32_t *>(res + row * (kRwChunks * 4) + chunk * 4);
}

template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_wide_encode_kernel(const uint16_t *__restrict__ X,       // [n_rows, 320]
                                                              const uint16_t *__restrict__ codes,   // [n_rows]
                                                              long long n_rows,
                                                              const uint16_t *__restrict__ C,       // [K, 320]
                                                              int K, const float *__restrict__ cutoffs,
                                                              uint8_t *__restrict__ res) {          // [n_rows, 40 BITS]
    constexpr int NC = (1 << BITS) - 1;
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long row = t / kRwChunks;
    const int c = (int)(t - row * kRwChunks);
    if (row >= n_rows) return;
    float cut[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) cut[i] = cutoffs[i];
    const int code = codes[row];
    uint32_t field = 0;                                                 // a code >= K never becomes an address: all-zero buckets
    if (code < K) {
        const bf16x8 x = *reinterpret_cast<const bf16x8 *>(X + (size_t)row * kRwDim + c * 8);
        const bf16x8 cc = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kRwDim + c * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float e = elem_to_float<F16>((uint16_t)x[j]) - elem_to_float<F16>((uint16_t)cc[j]);
            uint32_t b = 0;
#pragma unroll
            for (int i = 0; i < NC; ++i) b += cut[i] <= e ? 1u : 0u;
            field |= b << (j * BITS);
        }
    }
    if constexpr (BITS == 2) *reinterpret_cast<uint16_t *>(res + row * (kRwChunks * 2) + c * 2) = (uint16_t)field;
    else *reinterpret_cast<uint32_t *>(res + row * (kRwChunks * 4) + c * 4) = field;
}

template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_wide_decode_kernel(const uint16_t *__restrict__ codes, const uint8_t *__restrict__ res,
                                                              long long row0, long long row1, const uint16_t *__restrict__ C, int K,
                                                              const float *__restrict__ weights,
                                                              uint16_t *__restrict__ out) {         // [row1 - row0, 320]
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long rel = t / kRwChunks;
    const long long row = row0 + rel;
    const int c = (int)(t - rel * kRwChunks);
    if (row >= row1) return;
    const int code = codes[row];
    bf16x8 v;
    if (code < K) {
        const bf16x8 cc = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kRwDim + c * 8);
        v = rw_decode_chunk<F16, BITS>(cc, rw_load_field<BITS>(res, row, c), [&](int b) { return weights[b]; });
    } else {
        const short nan = (short)(F16 ? 0x7e00 : 0x7fc0);
        v = bf16x8{nan, nan, nan, nan, nan, nan, nan, nan};
    }
    *reinterpret_cast<bf16x8 *>(out + (size_t)rel * kRwDim + c * 8) = v;
}

// ---------------------------------------------------------------------------------------------------------------- rerank
__device__ __forceinline__ void rw_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one page (rows r0 .. r0 + len - 1) against NU resident query units, decoded slab by slab into the wave's three panel-slabs: mx[u] =
// the running maxima of unit u over this lane's rows (-inf for a page without rows).  Shared by the rerank (rw_entry) and the scan
// (residual_wide_scan.hip: rw_scan_group).
template <int NU, bool F16, int BITS>
__device__ __forceinline__ void rw_page_max(float (&mx)[NU], const bf16x8 (&qf)[NU][kRwKSteps], const uint16_t *__restrict__ codes,
                                            const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K, long long r0, int len,
                                            bool &bad, char *slabs, const float *wtab, const int (&rd_off)[2][kKSteps16], int lane) {
    const int l16 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int u = 0; u < NU; ++u) mx[u] = -INFINITY;

    // one chunk of one slab row: decoded in registers, stored at the panel-slab's swizzled position
    auto decode_one = [&](int s, int codev, int row, int chunk) {
        int code = __shfl(codev, row);
        if (code >= K) {                                // a broken code never becomes an address: the page scores NaN
            bad = true;
            code = 0;
        }
        const int pr = s * kSlabRows + row;
        const long long grow = r0 + (pr < len ? pr : len - 1);          // a row past the page's end names the page's last row
        const bf16x8 cc = *reinterpret_cast<const bf16x8 *>(C + (size_t)code * kRwDim + chunk * 8);
        const uint32_t fld = rw_load_field<BITS>(res, grow, chunk);
        const bf16x8 v = rw_decode_chunk<F16, BITS>(cc, fld, [&](int b) { return wtab[b]; });
        *reinterpret_cast<bf16x8 *>(slabs + (chunk >> 4) * kSlabBytes + slab_swizzled_off(row, chunk & 15)) = v;
    };

    auto slab = [&](auto tail_c, int s, int rows_left) {
        constexpr bool kTail = decltype(tail_c)::value;
        // lane r (and r + 32) holds the code of slab row r
        const int cr = s * kSlabRows + (lane & 31);
        const int codev = (int)codes[r0 + (cr < len ? cr : len - 1)];
        // panels 0 and 1: lane (l4, l16) decodes chunk 16 p + l16 of rows 4 i + l4; panel 2: lane decodes chunk 32 + (lane & 7) of rows
        // 8 i + (lane >> 3)
        // Five batches of four chunks, fenced: at most four centroid chunks and fields are in flight next to the query's registers
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
#pragma unroll
                for (int i = 4 * h; i < 4 * h + 4; ++i) decode_one(s, codev, 4 * i + l4, 16 * p + l16);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
        for (int i = 0; i < 4; ++i) decode_one(s, codev, 8 * i + (lane >> 3), 32 + (lane & 7));
        rw_wave_sync();

        UnitAcc acc[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int g = 0; g < 2; ++g) acc[u].a[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < kRwPanels; ++p) {
            const int nks = p == kRwPanels - 1 ? kRwLastKSteps : kKSteps16;
            const char *src = slabs + p * kSlabBytes;
            // one panel's 32 operand registers at a time: with eight units (320 query + 64 accumulator registers) the next panel's
            // fragments do not fit beside this one's
            if constexpr (NU > 6) __builtin_amdgcn_sched_barrier(0);
            bf16x8 af[2][kKSteps16];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int ks = 0; ks < kKSteps16; ++ks)
                    if (ks < nks) af[g][ks] = *reinterpret_cast<const bf16x8 *>(src + rd_off[g][ks]);
#pragma unroll
            for (int ks = 0; ks < kKSteps16; ++ks)
                if (ks < nks) {
#pragma unroll
                    for (int u = 0; u < NU; ++u)
#pragma unroll
                        for (int g = 0; g < 2; ++g) acc[u].a[g] = mfma16<F16>(af[g][ks], qf[u][p * kKSteps16 + ks], acc[u].a[g]);
                }
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if constexpr (kTail) unit_mask_tail(acc[u], rows_left, lane);
            unit_fold(mx[u], acc[u]);
        }
        rw_wave_sync();                                         // the operands are in registers before the next slab is stored
    };
    const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
    for (int s = 0; s < n_full; ++s) slab(std::false_type{}, s, kSlabRows);
    if (rem > 0) slab(std::true_type{}, n_full, rem);
}

// the score of one entry: the query's NU units against the page rows r0 .. r0 + len - 1.  Returns in lanes 0 .. 7; lane 0 stores.
template <int NU, bool F16, int BITS>
__device__ __forceinline__ float rw_entry(const uint16_t *__restrict__ Qt, int qs, int qe, const uint16_t *__restrict__ codes,
                                          const uint8_t *__restrict__ res, const uint16_t *__restrict__ C, int K, long long r0, int len,
                                          bool clamp, bool &bad, char *slabs, int lane) {
    const int l16 = lane & 15, l4 = lane >> 4;
    char *tokmax = slabs + kRwPanels * kSlabBytes;
    const float *wtab = reinterpret_cast<const float *>(tokmax + kStreamTokBytes);
    int rd_off[2][kKSteps16];                                   // per entry, not per kernel: nothing of it lives across the unit switch
    slab_rd_offsets16(lane, rd_off);
    // the query's units: K1cP's B operands, [unit][k-step of 32]
    bf16x8 qf[NU][kRwKSteps];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int row = qs + u * kUnitTok + l16;
        const bool valid = row < qe;
        const uint16_t *p = Qt + (size_t)(valid ? row : 0) * kRwDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < kRwKSteps; ++ks) {
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
            qf[u][ks] = valid ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    float mx[NU];
    rw_page_max<NU, F16, BITS>(mx, qf, codes, res, C, K, r0, len, bad, slabs, wtab, rd_off, lane);

#pragma unroll
    for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], lane);
    rw_wave_sync();
    float tot = 0.0f;
    if (lane < 8) tot = reduce_query_tokens<F16>(tokmax, 0, qe - qs, lane, clamp, false);
    rw_wave_sync();                                             // the sums have read the table before the next entry writes it
    return tot;
}

// one wave per SIMD (no second launch bound): eight resident units are 320 operand registers of the unified 512
template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_wide_candidates_kernel(const uint16_t *__restrict__ Qt,      // [q_rows, 320] flat query tokens
                                                                  const int32_t *__restrict__ q_off,   // [n_q + 1]
                                                                  int n_q, long long q_rows,
                                                                  const uint16_t *__restrict__ codes,  // [d_rows]
                                                                  const uint8_t *__restrict__ res,     // [d_rows, 40 BITS]
                                                                  const uint16_t *__restrict__ C,      // [K, 320]
                                                                  int K, const float *__restrict__ weights,
                                                                  const int32_t *__restrict__ d_off,   // [n_d + 1]
                                                                  const uint8_t *__restrict__ clamp0,  // [n_d] or null
                                                                  int n_d, long long d_rows,
                                                                  const int64_t *__restrict__ cand, long long ld_cand, int m,
                                                                  long long id_base, float *__restrict__ scores, long long ld,
                                                                  int64_t *__restrict__ out_ids, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *slabs = smem + wave * kRwLdsPerWave;
    char *tokmax = slabs + kRwPanels * kSlabBytes;
    float *wtab = reinterpret_cast<float *>(tokmax + kStreamTokBytes);
    if (lane < (1 << BITS)) wtab[lane] = weights[lane];
    rw_wave_sync();

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
                atomicOr(status, kRwBadQuery);
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
        const int len = __builtin_amdgcn_readfirstlane((int)(r1 - r0));
        const bool clamp = clamp0 != nullptr && clamp0[d] != 0;
        bool bad = false;
        float tot = 0.0f;
        switch ((len_q + kUnitTok - 1) / kUnitTok) {
#define MSIM_RW_CASE(U) \
            case U: tot = rw_entry<U, F16, BITS>(Qt, (int)qs, (int)qe, codes, res, C, K, r0, len, clamp, bad, slabs, lane); break;
            MSIM_RW_CASE(1)
            MSIM_RW_CASE(2)
            MSIM_RW_CASE(3)
            MSIM_RW_CASE(4)
            MSIM_RW_CASE(5)
            MSIM_RW_CASE(6)
            MSIM_RW_CASE(7)
            MSIM_RW_CASE(8)
#undef MSIM_RW_CASE
            default: break;
        }
        const bool any_bad = __builtin_amdgcn_ballot_w64(bad) != 0;
        if (lane == 0) *dst = any_bad ? __builtin_nanf("") : tot;
    }
}

// the status word starts at zero: a kernel, not a memset node (maxsim_candidates.hip: cand_zero_kernel)
__global__ void res_wide_zero_status_kernel(int32_t *__restrict__ status) {
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// a device q_off that disagrees with the host copy: every score of the call becomes NaN
__global__ __launch_bounds__(256) void res_wide_poison_kernel(const int32_t *__restrict__ status, int n_q, int m,
                                                              float *__restrict__ scores, long long ld) {
    if (*status == 0) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_q * m) return;
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    scores[(size_t)q * ld + j] = __builtin_nanf("");
}

}  // namespace msim
