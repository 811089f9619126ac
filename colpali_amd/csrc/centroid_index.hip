// A centroid-code copy of a packed corpus for gfx950 (MI355X): a PLAID-style first stage for two-stage search.  Every corpus row is
// stored as the uint16 id of its nearest centroid (2 B per row instead of 256 B); a page is scored by centroid interaction:
//   encode:  code[r]  = argmax_k <row_r, C_k>            (fp32-accumulated MFMA chain; the lowest k wins a tie)
//   table:   S[i, k]  = fp16(fl32 <q_i, C_k>)             (one MFMA chain per entry, k ascending)
//   score:   M_i      = max_j S[i, code_j]                (an exact max of fp16 values; max(M_i, 0) where clamp0[c] is set)
//            score    = the SEQUENTIAL fp32 sum, in token order, of float(M_i).    0-row page: -inf.  A code >= K: NaN.
// (include/maxsim.h: msim_cent_*).  The scan reads no corpus row and runs no MFMA: it is a table lookup bound by LDS reads.
//
// Kernels:
//   cent_encode_kernel   maxsim_align.hip with the roles swapped.  Workgroup (page, block of 256 rows): every wave keeps 4 tiles of 16
//                        page rows in registers (the B operand) and streams the K centroids from L2 in tiles of 16 (the A operand,
//                        one tile loaded ahead).  One chain of 4 v_mfma_f32_16x16x32 from zero per (centroid tile, row tile); each
//                        lane keeps a running (max, first k) over its centroids, the four lane groups are folded at the end.
//   cent_table_kernel    workgroup (32-token block of a query, 256 centroids): the block's tokens are the A operand, so a lane
//                        holds 4 consecutive tokens of one centroid and stores them as one 8-byte piece of table[block][k][32].
//   cent_scores_kernel   workgroup (query, range of pages), 8 waves.  The table of one 32-token block sits in LDS (K x 64 B); wave
//                        w scans pages of its own, one lane per page row: a coalesced 2-byte code load per row (4 rows in flight
//                        per lane), 4 ds_read_b128 for the row's 64 B of table, 16 v_pk_max_f16 into the running maxima.  At a
//                        page's end the 16 packed registers are folded across the wave by a halving butterfly (8 + 4 + 2 + 1 + 1 + 1
//                        exchanges), the 32 maxima are parked in a per-wave LDS slot, and once 16 pages are parked 16 lanes add
//                        one page each in token order.  A query longer than 32 tokens reloads the table per block and carries
//                        the sum on through scores[] (the same lane writes and reads a page's entry).
//   LDS image of the table: row k at byte 64 k, its 16-byte piece p at position p ^ ((k >> 2) & 3).  Under ds_read_b128 banking
//   ((a / 4) mod 64, lane groups of 16) a plain image puts every row's piece p on one of FOUR 4-bank sets; with the swizzle the
//   set is 16 (k & 3) + 4 (p ^ ((k >> 2) & 3)): sixteen sets chosen by k & 15, at no cost in LDS (K = 2048 leaves no room to pad).
// Nothing allocates or synchronises; no float atomics.  Every address comes from a checked number: page offsets against the row
// count, query offsets against the token count, a code against K before it becomes an LDS address.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kCentBlockTok = 32;           // query tokens per table block
constexpr int kCentTableRow = 64;           // bytes of table per centroid and block: 32 fp16
constexpr int kCentMinK = 256, kCentMaxK = 2048;
constexpr int kCentMaxTokens = 128;
constexpr int kCentWaves = 8;               // waves of a scan workgroup
constexpr int kCentBatch = 16;              // pages a wave parks before their token sums
constexpr int kCentMaxPpw = 64;             // pages per wave
constexpr int kCentEncRows = 256;           // page rows per encode workgroup: 4 waves x 4 tiles x 16
constexpr int kCentEncTiles = 4;

typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------- encode
template <bool F16>
__global__ __launch_bounds__(256) void cent_encode_kernel(const uint16_t *__restrict__ X,        // [n_rows, 128]
                                                          const int32_t *__restrict__ off,      // [n_d + 1]
                                                          int n_d, long long n_rows, int max_doc_rows,
                                                          const uint16_t *__restrict__ C,        // [K, 128]
                                                          int K, uint16_t *__restrict__ codes,   // [n_rows]
                                                          int32_t *__restrict__ status) {        // [n_d] or null
    constexpr int KS = kKSteps16;
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
        if (l4 == 0 && row < len) codes[r0 + row] = (uint16_t)(bk[t] < 0 ? 0 : bk[t]);
    }
}

// ---------------------------------------------------------------------------------------------------------------- table
// table [n_q * nb][K][32] fp16: block b of query q holds its tokens 32 b .. 32 b + 31 (0 for a token the query does not have)
template <bool F16>
__global__ __launch_bounds__(256) void cent_table_kernel(const uint16_t *__restrict__ Qt,       // [q_rows, 128] flat query tokens
                                                         const int32_t *__restrict__ q_off,    // [n_q + 1]
                                                         int n_q, long long q_rows, int nb,
                                                         const uint16_t *__restrict__ C,       // [K, 128]
                                                         int K, _Float16 *__restrict__ table) {
    constexpr int KS = kKSteps16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l16 = lane & 15, l4 = lane >> 4;
    const int blk = blockIdx.x, q = blk / nb, b = blk - q * nb;
    if (q >= n_q) return;
    const long long qs = q_off[q], qe = q_off[q + 1];
    const bool ok = qs >= 0 && qe >= qs && qe <= q_rows && qe - qs <= (long long)nb * kCentBlockTok;
    const int len = ok ? (int)(qe - qs) : 0;

    bf16x8 qf[2][KS];                                                   // A: the block's two 16-token tiles
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int tok = b * kCentBlockTok + h * 16 + l16;
        const bool valid = tok < len;
        const uint16_t *src = Qt + (size_t)(valid ? qs + tok : 0) * kDim + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            qf[h][ks] = valid ? *reinterpret_cast<const bf16x8 *>(src + ks * 32) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
    _Float16 *out = table + (size_t)blk * K * kCentBlockTok;
    const int k_base = blockIdx.y * 256 + wave * 64;                    // 64 centroids per wave: 4 tiles (K is a multiple of 256)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int k = k_base + c * 16 + l16;
        const uint16_t *src = C + (size_t)k * kDim + l4 * 8;
        bf16x8 cf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) cf[ks] = *reinterpret_cast<const bf16x8 *>(src + ks * 32);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma16<F16>(qf[h][ks], cf[ks], acc);      // one chain, k ascending
            // D: lane holds centroid k against tokens 16 h + 4 l4 + {0 .. 3}
            const h4 v = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
            *reinterpret_cast<h4 *>(out + (size_t)k * kCentBlockTok + h * 16 + 4 * l4) = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scan
__device__ __forceinline__ h2 cent_pkmax(h2 a, h2 b) { return __builtin_elementwise_max(a, b); }   // v_pk_max_f16
__device__ __forceinline__ h2 cent_h2(int v) { return __builtin_bit_cast(h2, v); }
__device__ __forceinline__ int cent_i(h2 v) { return __builtin_bit_cast(int, v); }

__device__ __forceinline__ void cent_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// one halving step of the page-end fold: lanes whose bit `BIT` is set keep the upper N registers, the others the lower N; each
// sends the half it drops to its partner and folds the half it receives
template <int N, int BIT>
__device__ __forceinline__ void cent_fold_half(h2 (&m)[16], bool hi) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int send = cent_i(hi ? m[i] : m[i + N]);
        const h2 keep = hi ? m[i + N] : m[i];
        m[i] = cent_pkmax(keep, cent_h2(__shfl_xor(send, BIT)));
    }
}

// LDS: [K * 64 B table][kCentWaves x kCentBatch x 64 B parked maxima]
__global__ __launch_bounds__(kCentWaves * 64) void cent_scores_kernel(const _Float16 *__restrict__ table,      // [n_q * nb][K][32]
                                                                      const int32_t *__restrict__ q_off, int n_q, long long q_rows,
                                                                      int nb, int K, const uint16_t *__restrict__ codes,
                                                                      const int32_t *__restrict__ d_off,
                                                                      const uint8_t *__restrict__ clamp0, int n_d, long long d_rows,
                                                                      int ppw, int n_pr, float *__restrict__ scores, long long ld) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *park = smem + (size_t)K * kCentTableRow + wave * (kCentBatch * kCentTableRow);

    // XCD-aware bijective remap: the workgroups of one page range (one per query) run back to back on one XCD and share its L2
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, q8n = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8n + 1) : r8 * (q8n + 1) + (xcd - r8) * q8n) + (orig >> 3);
    const int q = wgid % n_q, pr = wgid / n_q;
    if (pr >= n_pr) return;                                             // (whole workgroups: the barriers below stay complete)

    const long long qs = q_off[q], qe = q_off[q + 1];
    const bool q_ok = qs >= 0 && qe >= qs && qe <= q_rows && qe - qs <= (long long)nb * kCentBlockTok;
    const int len_q = q_ok ? (int)(qe - qs) : 0;
    const int nbq = (len_q + kCentBlockTok - 1) / kCentBlockTok;
    const int n_pass = nbq > 0 ? nbq : 1;                               // a query of 0 tokens still writes its 0 / -inf

    const long long p_first = ((long long)pr * kCentWaves + wave) * ppw;
    const int np = p_first >= n_d ? 0 : (int)(n_d - p_first < ppw ? n_d - p_first : ppw);
    const int p0 = np ? (int)p_first : 0;
    float *srow = scores + (long long)q * ld;

    for (int b = 0; b < n_pass; ++b) {
        if (b) __syncthreads();                                         // every wave is done with the previous block's table
        {
            const i32x4 *src = reinterpret_cast<const i32x4 *>(table + ((size_t)q * nb + b) * K * kCentBlockTok);
            for (int i = threadIdx.x; i < K * 4; i += kCentWaves * 64) {
                const int k = i >> 2, pc = i & 3;
                *reinterpret_cast<i32x4 *>(smem + k * kCentTableRow + ((pc ^ ((k >> 2) & 3)) << 4)) = src[i];
            }
        }
        __syncthreads();
        const int ntok = len_q - b * kCentBlockTok < kCentBlockTok ? len_q - b * kCentBlockTok : kCentBlockTok;   // <= 0: no token
        const bool last = b + 1 == n_pass;

        for (int pb = 0; pb < np; pb += kCentBatch) {
            const int nbat = np - pb < kCentBatch ? np - pb : kCentBatch;
            // the batch's page offsets, one per lane (lane i: off[p0 + pb + i], i <= nbat)
            const int offl = lane <= nbat ? d_off[p0 + pb + lane] : 0;
            const int offn = __shfl_down(offl, 1);
            const bool bad_off = lane < nbat && (offl < 0 || offn < offl || (long long)offn > d_rows);
            bool my_bad = bad_off;                                      // lane j: page pb + j is broken (offsets or a code)
            const bool my_empty = offn == offl;

            for (int j = 0; j < nbat; ++j) {
                const int r0 = __builtin_amdgcn_readlane(offl, j), r1 = __builtin_amdgcn_readlane(offn, j);
                const bool skip = __builtin_amdgcn_readlane((int)bad_off, j) != 0;
                h2 m[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) m[i] = h2{-(_Float16)INFINITY, -(_Float16)INFINITY};
                bool bad_code = false;
                if (!skip) {
                    for (int r = r0 + lane; r < r1; r += 4 * 64) {       // 4 rows in flight per lane
                        int code[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) code[u] = r + 64 * u < r1 ? (int)codes[r + 64 * u] : -1;
#pragma unroll
                        for (int u = 0; u < 4; ++u) {
                            if (code[u] < 0) continue;                   // no such row: the lane's maxima stay as they are
                            int k = code[u];
                            if (k >= K) {                                // a broken index never becomes an LDS address
                                bad_code = true;
                                k = 0;
                            }
                            const char *row = smem + k * kCentTableRow;
                            const int s = (k >> 2) & 3;
#pragma unroll
                            for (int pc = 0; pc < 4; ++pc) {
                                const i32x4 v = *reinterpret_cast<const i32x4 *>(row + ((pc ^ s) << 4));
#pragma unroll
                                for (int e = 0; e < 4; ++e) m[4 * pc + e] = cent_pkmax(m[4 * pc + e], cent_h2(v[e]));
                            }
                        }
                    }
                }
                if (__builtin_amdgcn_ballot_w64(bad_code) != 0 && lane == j) my_bad = true;
                // fold across the wave: register i of lane l ends as token pair l >> 2 in every lane
                cent_fold_half<8, 32>(m, (lane & 32) != 0);
                cent_fold_half<4, 16>(m, (lane & 16) != 0);
                cent_fold_half<2, 8>(m, (lane & 8) != 0);
                cent_fold_half<1, 4>(m, (lane & 4) != 0);
                m[0] = cent_pkmax(m[0], cent_h2(__shfl_xor(cent_i(m[0]), 2)));
                m[0] = cent_pkmax(m[0], cent_h2(__shfl_xor(cent_i(m[0]), 1)));
                if ((lane & 3) == 0) *reinterpret_cast<int *>(park + j * kCentTableRow + (lane >> 2) * 4) = cent_i(m[0]);
            }
            cent_wave_sync();
            if (lane < nbat) {                                          // lane j adds page pb + j in token order
                const int p = p0 + pb + lane;
                const bool c0 = clamp0 && clamp0[p];
                float T = b ? srow[p] : 0.0f;
                const _Float16 *mx = reinterpret_cast<const _Float16 *>(park + lane * kCentTableRow);
                for (int i = 0; i < ntok; ++i) {
                    float v = (float)mx[i];
                    if (c0) v = __builtin_fmaxf(v, 0.0f);
                    T += v;
                }
                if (last) T = (my_bad || !q_ok) ? __builtin_nanf("") : my_empty ? -__builtin_inff() : T;
                srow[p] = T;
            }
            cent_wave_sync();                                           // the sums have read the slots before the next batch parks
        }
    }
}

}  // namespace msim
