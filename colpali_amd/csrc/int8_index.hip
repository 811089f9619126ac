// An int8 copy of a packed corpus for gfx950 (MI355X): a token-level first stage for two-stage search.  It keeps MaxSim's token
// structure, streams 128 B per row instead of 256 B and scores on v_mfma_i32_16x16x64_i8 (2x the bf16 rate).  Every per-token
// maximum is an exact integer, so a score's bits are fixed by the documented order below (include/maxsim.h: msim_i8_*).
//
// Quantization (fp32 on the bf16 / f16 values; `/` is the correctly rounded fp32 division, rintf rounds half to even):
//   page c: a = max |x| over its rows; inv = 127 / a; code = x == 0 ? 0 : clamp(rint(x * inv), -127, 127); scale = a / 127.
//   A page with a = 0 gets codes 0 and scale 0.  A query token row is quantized the same way with its own row max.
// Score:  I_ij = sum_k q8_ik d8_jk (int32, exact);  M_ic = max_j I_ij (max(M_ic, 0) when clamp0[c]);
//         S_qc = sd_c * T,  T = the sequential fp32 sum, in token order, of float(M_ic) * sq_i.   0-row page: -inf.
//
// Kernels:
//   i8_encode_docs_kernel     one 256-thread workgroup per page: 16 lanes per row, 8 elements (16 B) each.  Pass 1 reduces the page
//                             max (exact whatever the order), pass 2 re-reads the page (from L2) and writes 8 code bytes per lane.
//   i8_encode_rows_kernel     the query tokens: 16 rows per workgroup, the row max folded across its 16 lanes by xor-shuffles.
//   i8_scores_kernel<NT,GW,D> one wave scores a GROUP of whole queries (NT 16-token tiles in registers, the B operand) against a
//                             range of consecutive pages.  The pages' rows are ONE contiguous stream of 16-row chunks (the A
//                             operand), read by bounds-checked buffer loads D chunks ahead.  Two 16x16x64 MFMAs per (chunk, tile);
//                             the running max is a v_max_i32 on the accumulators.  Only a chunk that holds a page boundary is
//                             masked; at a page's end the per-token maxima are folded across lanes, scaled, summed in token order
//                             by one lane per query (through LDS) and stored once per (query, page).
//                             GW waves of a workgroup take GW query groups of ONE page range (the rows are read once per workgroup
//                             from L2, the others hit in L1), and consecutive workgroups of a page range run on one XCD.
//                             Its body is token_scores<NT,GW,D,Rows> over I8Rows; binary_index.hip runs the same body over its
//                             sign-bit rows.
// Nothing allocates or synchronises.  Every address comes from a checked index: page offsets against the row count, query offsets
// against the token count and the caller's bound on a query's length.  A page range or a query whose offsets break them is
// written as NaN.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kI8Row = kDim;               // bytes per int8 row
constexpr int kI8MaxRange = 63;            // pages per wave range (their offsets sit in one lane each)

typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

__device__ __forceinline__ float i8_absmax8(const bf16x8 &e, bool f16, float m) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float v = f16 ? elem_to_float<true>((uint16_t)e[u]) : elem_to_float<false>((uint16_t)e[u]);
        m = __builtin_fmaxf(m, __builtin_fabsf(v));
    }
    return m;
}

// the 8 codes of one 16-byte piece, packed little-endian
template <bool F16>
__device__ __forceinline__ u32x2 i8_codes8(const bf16x8 &e, float inv) {
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const float x = elem_to_float<F16>((uint16_t)e[u]);
        const float p = x * inv;                                     // one rounding; inv = +inf for a page in the subnormal range
        const float r = __builtin_fminf(__builtin_fmaxf(__builtin_rintf(p), -127.0f), 127.0f);
        const int c = x == 0.0f ? 0 : (int)r;
        w[u >> 2] |= ((uint32_t)c & 0xffu) << (8 * (u & 3));
    }
    return u32x2{w[0], w[1]};
}

// one workgroup per page: rows off[p] .. off[p + 1] - 1 of X [n_rows, 128]; codes at the same rows of C [n_rows, 128]
template <bool F16>
__global__ __launch_bounds__(256) void i8_encode_docs_kernel(const uint16_t *__restrict__ X, const int32_t *__restrict__ off, int n_d,
                                                             long long n_rows, int8_t *__restrict__ C, float *__restrict__ scales) {
    __shared__ float wmax[4];
    const int t = threadIdx.x, p = blockIdx.x;
    if (p >= n_d) return;
    const long long r0 = off[p], r1 = off[p + 1];
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {                          // never trust a device offset with an address
        if (t == 0) scales[p] = __builtin_nanf("");
        return;
    }
    const int sub = t & 15, rsub = t >> 4;                            // 16 lanes per row, 16 rows per pass
    float m = 0.0f;
    for (long long r = r0 + rsub; r < r1; r += 16)
        m = i8_absmax8(*reinterpret_cast<const bf16x8 *>(X + r * kDim + sub * 8), F16, m);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, s));
    if ((t & 63) == 0) wmax[t >> 6] = m;
    __syncthreads();
    const float a = __builtin_fmaxf(__builtin_fmaxf(wmax[0], wmax[1]), __builtin_fmaxf(wmax[2], wmax[3]));
    const float inv = 127.0f / a;
    for (long long r = r0 + rsub; r < r1; r += 16) {
        const bf16x8 e = *reinterpret_cast<const bf16x8 *>(X + r * kDim + sub * 8);
        *reinterpret_cast<u32x2 *>(C + r * kI8Row + sub * 8) = i8_codes8<F16>(e, inv);
    }
    if (t == 0) scales[p] = a / 127.0f;
}

// one row per 16 lanes: codes C [n_rows, 128] and scales [n_rows] of X [n_rows, 128]
template <bool F16>
__global__ __launch_bounds__(256) void i8_encode_rows_kernel(const uint16_t *__restrict__ X, long long n_rows, int8_t *__restrict__ C,
                                                             float *__restrict__ scales) {
    const int t = threadIdx.x, sub = t & 15;
    const long long r = (long long)blockIdx.x * 16 + (t >> 4);
    const bool live = r < n_rows;
    bf16x8 e = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) e = *reinterpret_cast<const bf16x8 *>(X + r * kDim + sub * 8);
    float m = i8_absmax8(e, F16, 0.0f);
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) m = __builtin_fmaxf(m, __shfl_xor(m, s));
    const float inv = 127.0f / m;
    if (live) {
        *reinterpret_cast<u32x2 *>(C + r * kI8Row + sub * 8) = i8_codes8<F16>(e, inv);
        if (sub == 0) scales[r] = m / 127.0f;
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scorer
constexpr int kI8Tile = 16;                 // tokens per tile (MFMA N) and rows per chunk (MFMA M)

__device__ __forceinline__ i32x4 i8_mfma(const i32x4 &a, const i32x4 &b, const i32x4 &c) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }   // v_max_i32

__device__ __forceinline__ int lane_of(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// The page rows of the int8 index, as the scorer below reads them: 128 code bytes per row, the lane's two 16-byte pieces ARE its A
// operands, and a page's token sum is scaled by the page's fp32 scale.  (binary_index.hip has the sign-bit rows.)
struct I8Rows {
    const int8_t *__restrict__ d8;
    const float *__restrict__ sd;
    static constexpr int kRowBytes = kI8Row;
    struct Chunk {
        i32x4 v[2];
    };
    __device__ __forceinline__ const void *row(long long r) const { return d8 + r * kI8Row; }
    __device__ __forceinline__ static void load(const __amdgpu_buffer_rsrc_t &rs, int row, int l4, Chunk &c) {
        const int voff = row * kI8Row + l4 * 16;                     // past the stream's end: the descriptor returns zeros
        c.v[0] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, 0, 0));
        c.v[1] = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff + 64, 0, 0));
    }
    __device__ __forceinline__ static void operands(const Chunk &c, i32x4 &a0, i32x4 &a1) {
        a0 = c.v[0];
        a1 = c.v[1];
    }
    __device__ __forceinline__ float page_score(int p, float T) const { return sd[p] * T; }
};

// NT: 16-token tiles per wave; GW: waves of a workgroup that share one page range (1, 2 or 4); D: chunks loaded ahead; Rows: the
// page rows (I8Rows, BinRows): their bytes per row, the chunk load, its expansion to the two A operands, and the page's scale
// queries: group g = queries g * QG .. g * QG + QG - 1, query slot s owns tiles s * TPQ .. s * TPQ + TPQ - 1 (QG * TPQ <= NT);
// with passes > 1 (QG = 1, TPQ = NT) the page range is streamed once per NT tiles and the sum carries on in token order.
template <int NT, int GW, int D, class Rows>
__device__ __forceinline__ void token_scores(const int8_t *__restrict__ q8, const float *__restrict__ sq,
                                             const int32_t *__restrict__ q_off, int n_q, long long q_rows, int QG, int TPQ, int passes,
                                             const Rows rows, const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0,
                                             int n_d, long long d_rows, int ppw, int n_groups, int n_gb, float *__restrict__ scores,
                                             long long ld) {
    static_assert(GW == 1 || GW == 2 || GW == 4, "waves per page range");
    constexpr int RW = 4 / GW;                                         // page ranges per workgroup
    __shared__ float vals_all[4][NT * kI8Tile];
    __shared__ float part_all[4][kI8MaxRange];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *vals = vals_all[wave];
    float *part = part_all[wave];

    // XCD-aware bijective remap: the query-group blocks of one page range run back to back on one XCD and share its L2
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, q8n = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8n + 1) : r8 * (q8n + 1) + (xcd - r8) * q8n) + (orig >> 3);
    const int gb = wgid % n_gb, pb = wgid / n_gb;
    const int g = gb * GW + wave % GW;
    const long long p0l = ((long long)pb * RW + wave / GW) * ppw;
    if (g >= n_groups || p0l >= n_d) return;                           // whole waves only: no workgroup barrier below
    const int p0 = (int)p0l, np = n_d - p0 < ppw ? n_d - p0 : ppw;

    // the range's page offsets, one per lane (lane i: off[p0 + i], i <= np), checked before any is used
    const int offl = lane <= np ? d_off[p0 + lane] : 0;
    const int offn = __shfl_down(offl, 1);
    const bool bad_page = lane < np && (offl < 0 || offn < offl || (long long)offn > d_rows);
    const int R0 = lane_of(offl, 0), R1 = lane_of(offl, np);
    const bool range_ok = !__builtin_amdgcn_ballot_w64(bad_page) && R1 - R0 <= (1 << 23);   // 32-bit buffer offsets below

    // the group's queries: lane s < QG holds query g * QG + s
    const long long qi_l = (long long)g * QG + lane;
    int qa = 0, ql = 0, qok = 0;
    if (lane < QG && qi_l < n_q) {
        const long long a = q_off[qi_l], b = q_off[qi_l + 1];
        qok = a >= 0 && b >= a && b <= q_rows && b - a <= (long long)passes * TPQ * kI8Tile;
        if (qok) {
            qa = (int)a;
            ql = (int)(b - a);
        }
    }
    const int nqs = (int)(n_q - (long long)g * QG < QG ? n_q - (long long)g * QG : QG);   // live query slots

    if (!range_ok) {
        for (int pl = 0; pl < np; ++pl)
            if (lane < nqs) scores[((long long)g * QG + lane) * ld + p0 + pl] = __builtin_nanf("");
        return;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(rows.row(R0)), 0,
                                                                        (R1 - R0) * Rows::kRowBytes, 0x00020000);
    const int nrows = R1 - R0, nch = (nrows + kI8Tile - 1) / kI8Tile;
    const int lrow = lane & 15, l4 = lane >> 4, kq = l4 * 16;         // operand lane map: row lrow, bytes kq .. kq + 15 of each half

    for (int pass = 0; pass < passes; ++pass) {
        // the query fragments (B) and token scales of this pass, in registers for the whole page range
        i32x4 qb[NT][2];
        float sqv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int s = t / TPQ, tok = (pass * NT + t % TPQ) * kI8Tile + lrow;
            const int a = __shfl(qa, s), l = __shfl(ql, s);
            qb[t][0] = qb[t][1] = i32x4{0, 0, 0, 0};
            sqv[t] = 0.0f;
            if (s < nqs && tok < l) {
                const i32x4 *src = reinterpret_cast<const i32x4 *>(q8 + (long long)(a + tok) * kI8Row + kq);
                qb[t][0] = src[0];
                qb[t][1] = src[4];
                sqv[t] = sq[a + tok];
            }
        }

        auto load = [&](int ch, typename Rows::Chunk &dst) { Rows::load(rs, ch * kI8Tile + lrow, l4, dst); };

        i32x4 runmax[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) runmax[t] = i32x4{INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
        int pl = 0;
        int pstart = 0, pend = lane_of(offl, 1) - R0;

        // page pl ends: fold the tiles' maxima, scale, sum in token order, store
        auto finish = [&]() {
            const int p = p0 + pl;
            const bool empty = pend == pstart;
            const bool c0 = clamp0 && clamp0[p];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                int m = imax(imax(runmax[t][0], runmax[t][1]), imax(runmax[t][2], runmax[t][3]));
                m = imax(m, __shfl_xor(m, 16));
                m = imax(m, __shfl_xor(m, 32));
                if (c0) m = imax(m, 0);
                if (lane < 16) vals[t * kI8Tile + lane] = (float)m * sqv[t];
                runmax[t] = i32x4{INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < nqs) {
                float T = pass ? part[pl] : 0.0f;
                const int lo = pass * NT * kI8Tile, hi = ql < lo + TPQ * kI8Tile ? ql : lo + TPQ * kI8Tile;
                const float *v = vals + lane * TPQ * kI8Tile - lo;
                for (int k = lo; k < hi; ++k) T += v[k];
                if (pass + 1 < passes) {
                    part[pl] = T;
                } else {
                    const float s = empty ? -__builtin_inff() : qok ? rows.page_score(p, T) : __builtin_nanf("");
                    scores[((long long)g * QG + lane) * ld + p] = s;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                           // the sums have read vals before the next page writes them
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            ++pl;
            pstart = pend;
            pend = pl < np ? lane_of(offl, pl + 1) - R0 : 0x7fffffff;
        };

        typename Rows::Chunk buf[D];
#pragma unroll
        for (int d = 0; d < D; ++d) load(d, buf[d]);
        for (int ch0 = 0; ch0 < nch; ch0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int ch = ch0 + d;
                if (ch >= nch) break;
                i32x4 a0, a1;
                Rows::operands(buf[d], a0, a1);
                load(ch + D, buf[d]);
                i32x4 acc[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = i8_mfma(a0, qb[t][0], i32x4{0, 0, 0, 0});
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = i8_mfma(a1, qb[t][1], acc[t]);
                // D: lane holds token (lane & 15) of each tile against chunk rows 4 (lane >> 4) + {0..3}
                const int cs = ch * kI8Tile, ce = cs + kI8Tile;
                if (pstart <= cs && pend >= ce) {                         // the chunk lies inside one page: every row is real, no mask
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) runmax[t][r] = imax(runmax[t][r], acc[t][r]);
                    if (pend == ce && pl < np) finish();
                } else {
                    // a page boundary inside the chunk.  A range's last partial chunk always comes here (its last boundary is the
                    // range's end), so the rows the descriptor made up past it stay outside [lo, hi) of every page that is stored
                    while (true) {
                        const int lo = (pstart > cs ? pstart : cs) - cs, hi = (pend < ce ? pend : ce) - cs;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = (lane >> 4) * 4 + r;
                            if (row >= lo && row < hi)
#pragma unroll
                                for (int t = 0; t < NT; ++t) runmax[t][r] = imax(runmax[t][r], acc[t][r]);
                        }
                        if (pl < np && pend <= ce) {
                            finish();
                            continue;
                        }
                        break;
                    }
                }
            }
        }
        while (pl < np) finish();                                         // empty pages at the range's end (and a range of 0 rows)
    }
}

template <int NT, int GW, int D>
__global__ __launch_bounds__(256) void i8_scores_kernel(const int8_t *__restrict__ q8, const float *__restrict__ sq,
                                                        const int32_t *__restrict__ q_off, int n_q, long long q_rows, int QG, int TPQ,
                                                        int passes, const int8_t *__restrict__ d8, const float *__restrict__ sd,
                                                        const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                                        long long d_rows, int ppw, int n_groups, int n_gb, float *__restrict__ scores,
                                                        long long ld) {
    token_scores<NT, GW, D>(q8, sq, q_off, n_q, q_rows, QG, TPQ, passes, I8Rows{d8, sd}, d_off, clamp0, n_d, d_rows, ppw, n_groups, n_gb,
                            scores, ld);
}

}  // namespace msim
