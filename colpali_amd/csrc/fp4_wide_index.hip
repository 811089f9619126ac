// The FP4 (OCP e2m1) index at width 320 (ColQwen3) for gfx950 (MI355X): the sibling of fp4_index.hip, as maxsim_candidates' wide
// form is to its 128-wide one.  A row -- a page row or a query token -- is 160 bytes of e2m1 nibbles and ONE E8M0 scale byte, 161 B
// instead of 640, and is scored on v_mfma_scale_f32_16x16x128_f8f6f4: a 320-wide row is 2 1/2 of its K blocks, so one (16 rows x 16
// tokens) product is THREE scaled MFMAs chained through the C operand.  With one scale per row every partial sum is a multiple of
// 2^(eq + ed - 2) below 2^24 of them, so the sum is exact in any order and a score's bits are fixed by the documented order below
// (include/maxsim.h: msim_f4w_*).  Nothing here is shared with fp4_index.hip but the header both include: a shared body changes the
// parent kernels' machine code, so this file has a body of its own and is compiled alone in abi_fp4_wide.hip.
//
// Row code (fp32 / integer logic on the stored bf16 / f16 values; NaN elements are unspecified): msim_f4_encode_rows' rule over 320
//   dimensions.  a = max over all 320 |x_k|.  a == 0: every nibble 0, scale byte 127.  Otherwise e = the smallest integer with
//   a <= 6 * 2^e, clamped to [-32, 32], read from a's exponent and mantissa fields: a = m * 2^E (1 <= m < 2) gives
//   e = E - 2 + (m > 1.5).  y_k = min(|x_k| * 2^-e, 6); code = the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6}, ties to the even code;
//   nibble = sign << 3 | code (0 when the code is 0); dimension k is nibble (k & 1) of byte (k >> 1) of a 160-byte row.  Scale
//   byte = e + 127.
// Score:  I_ij = sum_{k<320} v(q_ik) v(d_jk) (a multiple of 1/4, |I| <= 320 * 36 = 11 520: 46 080 quarters, below 2^24);
//         Z_ij = I_ij * 2^(eq_i + ed_j);  M_ic = max_j Z_ij (max(M_ic, 0) when clamp0[c]);  S_qc = the sequential fp32 sum of M_ic
//         in token order.  0-row page: -inf.
//
// Kernels:
//   f4w_encode_rows_kernel     pages and query tokens alike: 8 lanes per row, 40 elements (80 B, five 16-byte loads) each; the row
//                              maximum (on the bit patterns) folded across the 8 lanes by xor-shuffles; every lane stores its 20
//                              code bytes as five dwords, one lane the scale byte.
//   f4w_scores_kernel<NT,GW,D> f4_scores_kernel's structure: one wave holds a GROUP of whole queries (NT 16-token tiles: 10 VGPRs
//                              and the scale byte per tile) and streams a range of consecutive pages as ONE run of 16-row chunks
//                              behind two bounds-checked buffer descriptors (codes, scale bytes), D chunks ahead.  K block b is
//                              dimensions 128 b .. 128 b + 127, bytes 64 b .. of the row; block 2 holds 64 real dimensions.  Lane
//                              (row = lane & 15, l4 = lane >> 4) holds bytes 16 l4 .. + 15 of blocks 0 and 1 (one b128 load each)
//                              and bytes 8 l4 .. + 7 of block 2 (one b64 load), the upper two registers of that operand zero on
//                              BOTH sides: the same function on A and B, so the order of k inside the instruction does not matter.
//                              Per chunk the MFMAs run block-major over the tiles -- NT independent ones between two that depend
//                              on each other through C.  The running maxima take one v_med3_f32 per accumulator; only a chunk that
//                              holds a page boundary is masked; at a page's end the maxima are folded across lanes, summed in token
//                              order by one lane per query (through LDS) and stored once per (query, page).
// ROWS PAST THE STREAM'S END come back from the descriptors as zero nibbles with scale byte 0: a zero row, which scores 0 and would
// beat every real row of an all-negative page.  Such rows sit only in the stream's last, partial chunk; that chunk holds the last
// page boundary (the stream's end), so it takes the masked path and rows past the boundary never reach a maximum that is stored.
// Nothing allocates or synchronises.  Every address comes from a checked index: page offsets against the row count, query offsets
// against the token count and the caller's bound on a query's length.  A page range or a query whose offsets break them is
// written as NaN.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kF4wDim = 320;
constexpr int kF4wRow = kF4wDim / 2;         // code bytes per row
constexpr int kF4wTile = 16;                 // tokens per tile (MFMA N) and rows per chunk (MFMA M)
constexpr int kF4wMaxRange = 63;             // pages per wave range (their offsets sit in one lane each)
constexpr int kF4wMinExp = -32, kF4wMaxExp = 32;
// rows of one wave range: the largest byte offset a chunk load forms, (rows + 16 (D + 1)) * 160, stays below 2^31
constexpr int kF4wMaxRangeRows = 1 << 23;

typedef __attribute__((ext_vector_type(8))) int f4w_i32x8;
typedef __attribute__((ext_vector_type(2))) int f4w_i32x2;

// |x| of one stored element as fp32 bits (monotone in |x| for everything but NaN)
template <bool F16>
__device__ __forceinline__ uint32_t f4w_abs_bits(uint16_t v) {
    return __float_as_uint(elem_to_float<F16>(v)) & 0x7fffffffu;
}

// the e2m1 nibble of one element: y = min(|x| * 2^-e, 6) rounded to the grid, ties to the even code
__device__ __forceinline__ uint32_t f4w_nibble(float x, float inv) {
    const float y = __builtin_fminf(__builtin_fabsf(x) * inv, 6.0f);
    const uint32_t code = (uint32_t)(y > 0.25f) + (uint32_t)(y >= 0.75f) + (uint32_t)(y > 1.25f) + (uint32_t)(y >= 1.75f) +
                          (uint32_t)(y > 2.5f) + (uint32_t)(y >= 3.5f) + (uint32_t)(y > 5.0f);
    return code ? code | ((__float_as_uint(x) >> 31) << 3) : 0u;
}

// one row per 8 lanes: codes C [n_rows, 160] and scale bytes S [n_rows] of X [n_rows, 320]
template <bool F16>
__global__ __launch_bounds__(256) void f4w_encode_rows_kernel(const uint16_t *__restrict__ X, long long n_rows, uint8_t *__restrict__ C,
                                                              uint8_t *__restrict__ S) {
    const int t = threadIdx.x, sub = t & 7;
    const long long r = (long long)blockIdx.x * 32 + (t >> 3);
    const bool live = r < n_rows;
    bf16x8 e[5];
#pragma unroll
    for (int v = 0; v < 5; ++v) {
        e[v] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live) e[v] = *reinterpret_cast<const bf16x8 *>(X + r * kF4wDim + sub * 40 + v * 8);
    }
    uint32_t a = 0;
#pragma unroll
    for (int v = 0; v < 5; ++v)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint32_t b = f4w_abs_bits<F16>((uint16_t)e[v][u]);
            a = a > b ? a : b;
        }
#pragma unroll
    for (int s = 1; s < 8; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)a, s);
        a = a > o ? a : o;
    }
    // a = m * 2^E: a <= 6 * 2^e = 1.5 * 2^(e + 2) first holds at e = E - 2 when m <= 1.5 and at e = E - 1 above
    int ex = (int)(a >> 23) - 127 - 2 + ((a & 0x7fffffu) > 0x400000u ? 1 : 0);
    ex = ex < kF4wMinExp ? kF4wMinExp : ex > kF4wMaxExp ? kF4wMaxExp : ex;
    if (a == 0) ex = 0;
    const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);       // 2^-e, exact
    if (live) {
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            uint32_t w = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) w |= f4w_nibble(elem_to_float<F16>((uint16_t)e[v][u]), inv) << (4 * u);
            *reinterpret_cast<uint32_t *>(C + r * kF4wRow + sub * 20 + v * 4) = w;
        }
        if (sub == 0) S[r] = (uint8_t)(ex + 127);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scorer
// One K block of 16 rows x 16 tokens added to c: FP4 is format code 4 on both sides; the scale of a lane's block is byte 0 of its
// scale register (op_sel 0), 2^(byte - 127).  The instruction scales the product and adds c as it stands, so c carries the blocks
// before this one in the same units (hardware fact (g)).
__device__ __forceinline__ f32x4 f4w_mfma(const f4w_i32x8 &a, int sa, const f4w_i32x8 &b, int sb, const f32x4 &c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 4, 0, sa, 0, sb);
}

__device__ __forceinline__ float f4w_max(float a, float b) { return __builtin_fmaxf(a, b); }   // no NaN reaches it

// The running maximum in the chunk loop as ONE VALU instruction, max(a, b) = med3(a, b, +inf): see f4_max_acc (fp4_index.hip).
// `inf` must not be a constant the compiler sees.
__device__ __forceinline__ float f4w_max_acc(float a, float b, float inf) { return __builtin_amdgcn_fmed3f(a, b, inf); }

// a row's operand registers in one lane: K blocks 0 and 1 (16 bytes each) and the lane's 8 bytes of block 2
struct F4wRow {
    i32x4 b0, b1;
    f4w_i32x2 b2;
    int s;
};

__device__ __forceinline__ f4w_i32x8 f4w_op(const i32x4 &v) { return f4w_i32x8{v[0], v[1], v[2], v[3], 0, 0, 0, 0}; }
__device__ __forceinline__ f4w_i32x8 f4w_op(const f4w_i32x2 &v) { return f4w_i32x8{v[0], v[1], 0, 0, 0, 0, 0, 0}; }

// NT: 16-token tiles per wave; GW: waves of a workgroup that share one page range (1, 2 or 4); D: chunks loaded ahead.
// queries: group g = queries g * QG .. g * QG + QG - 1, query slot s owns tiles s * TPQ .. s * TPQ + TPQ - 1 (QG * TPQ <= NT);
// with passes > 1 (QG = 1, TPQ = NT) the page range is streamed once per NT tiles and the sum carries on in token order.
template <int NT, int GW, int D>
__global__ __launch_bounds__(256) void f4w_scores_kernel(const uint8_t *__restrict__ q4, const uint8_t *__restrict__ qs,
                                                         const int32_t *__restrict__ q_off, int n_q, long long q_rows, int QG, int TPQ,
                                                         int passes, const uint8_t *__restrict__ d4, const uint8_t *__restrict__ ds,
                                                         const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                                         long long d_rows, int ppw, int n_groups, int n_gb, float *__restrict__ scores,
                                                         long long ld) {
    static_assert(GW == 1 || GW == 2 || GW == 4, "waves per page range");
    constexpr int RW = 4 / GW;                                         // page ranges per workgroup
    constexpr float kNegInf = -__builtin_inff();
    const float kInf = __uint_as_float(0x7f800000u | ((uint32_t)n_d >> 31));   // +inf (n_d >= 0), opaque to the compiler: f4w_max_acc
    __shared__ float vals_all[4][NT * kF4wTile];
    __shared__ float part_all[4][kF4wMaxRange];
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
    const int R0 = __builtin_amdgcn_readlane(offl, 0), R1 = __builtin_amdgcn_readlane(offl, np);
    const bool range_ok = !__builtin_amdgcn_ballot_w64(bad_page) && R1 - R0 <= kF4wMaxRangeRows;   // 32-bit buffer offsets below

    // the group's queries: lane s < QG holds query g * QG + s
    const long long qi_l = (long long)g * QG + lane;
    int qa = 0, ql = 0, qok = 0;
    if (lane < QG && qi_l < n_q) {
        const long long a = q_off[qi_l], b = q_off[qi_l + 1];
        qok = a >= 0 && b >= a && b <= q_rows && b - a <= (long long)passes * TPQ * kF4wTile;
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
    // two descriptors over the range's rows: the code bytes and the scale bytes; past their ends both return zeros
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(d4 + (long long)R0 * kF4wRow), 0,
                                                                        (R1 - R0) * kF4wRow, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(ds + R0), 0, R1 - R0, 0x00020000);
    const int nrows = R1 - R0, nch = (nrows + kF4wTile - 1) / kF4wTile;
    const int lrow = lane & 15, l4 = lane >> 4;                        // operand lane map: row lrow, lane group l4
    const int k01 = l4 * 16, k2 = 128 + l4 * 8;                        // bytes k01 .. + 15 of blocks 0 (and, + 64, 1); k2 .. + 7 of block 2

    for (int pass = 0; pass < passes; ++pass) {
        // the query fragments (B) and their scale bytes of this pass, in registers for the whole page range; a slot without a
        // token is a zero row (zero nibbles, scale byte 0): it scores 0 and is never summed
        F4wRow qb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int s = t / TPQ, tok = (pass * NT + t % TPQ) * kF4wTile + lrow;
            const int a = __shfl(qa, s), l = __shfl(ql, s);
            qb[t].b0 = qb[t].b1 = i32x4{0, 0, 0, 0};
            qb[t].b2 = f4w_i32x2{0, 0};
            qb[t].s = 0;
            if (s < nqs && tok < l) {
                const uint8_t *row = q4 + (long long)(a + tok) * kF4wRow;
                qb[t].b0 = *reinterpret_cast<const i32x4 *>(row + k01);
                qb[t].b1 = *reinterpret_cast<const i32x4 *>(row + 64 + k01);
                qb[t].b2 = *reinterpret_cast<const f4w_i32x2 *>(row + k2);
                qb[t].s = qs[a + tok];
            }
        }

        auto load = [&](int ch, F4wRow &dst) {
            const int row = ch * kF4wTile + lrow;
            dst.b0 = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4wRow + k01, 0, 0));
            dst.b1 = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4wRow + 64 + k01, 0, 0));
            dst.b2 = __builtin_bit_cast(f4w_i32x2, __builtin_amdgcn_raw_buffer_load_b64(rc, row * kF4wRow + k2, 0, 0));
            dst.s = (int)__builtin_amdgcn_raw_buffer_load_b8(rsc, row, 0, 0);
        };

        f32x4 runmax[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) runmax[t] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};
        int pl = 0;
        int pstart = 0, pend = __builtin_amdgcn_readlane(offl, 1) - R0;

        // page pl ends: fold the tiles' maxima, sum in token order, store
        auto finish = [&]() {
            const int p = p0 + pl;
            const bool empty = pend == pstart;
            const bool c0 = clamp0 && clamp0[p];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                float m = f4w_max(f4w_max(runmax[t][0], runmax[t][1]), f4w_max(runmax[t][2], runmax[t][3]));
                m = f4w_max(m, __shfl_xor(m, 16));
                m = f4w_max(m, __shfl_xor(m, 32));
                if (c0) m = f4w_max(m, 0.0f);
                if (lane < 16) vals[t * kF4wTile + lane] = m;
                runmax[t] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < nqs) {
                float T = pass ? part[pl] : 0.0f;
                const int lo = pass * NT * kF4wTile, hi = ql < lo + TPQ * kF4wTile ? ql : lo + TPQ * kF4wTile;
                const float *v = vals + lane * TPQ * kF4wTile - lo;
                for (int k = lo; k < hi; ++k) T += v[k];
                if (pass + 1 < passes) {
                    part[pl] = T;
                } else {
                    const float s = empty ? kNegInf : qok ? T : __builtin_nanf("");
                    scores[((long long)g * QG + lane) * ld + p] = s;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                           // the sums have read vals before the next page writes them
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            ++pl;
            pstart = pend;
            pend = pl < np ? __builtin_amdgcn_readlane(offl, pl + 1) - R0 : 0x7fffffff;
        };

        F4wRow buf[D];
#pragma unroll
        for (int d = 0; d < D; ++d) load(d, buf[d]);
        for (int ch0 = 0; ch0 < nch; ch0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int ch = ch0 + d;
                if (ch >= nch) break;
                const f4w_i32x8 a0 = f4w_op(buf[d].b0), a1 = f4w_op(buf[d].b1), a2 = f4w_op(buf[d].b2);
                const int sa = buf[d].s;
                load(ch + D, buf[d]);
                // block-major over the tiles: NT independent MFMAs between two chained through C
                f32x4 acc[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f4w_mfma(a0, sa, f4w_op(qb[t].b0), qb[t].s, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f4w_mfma(a1, sa, f4w_op(qb[t].b1), qb[t].s, acc[t]);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f4w_mfma(a2, sa, f4w_op(qb[t].b2), qb[t].s, acc[t]);
                // D: lane holds token (lane & 15) of each tile against chunk rows 4 (lane >> 4) + {0..3}
                const int cs = ch * kF4wTile, ce = cs + kF4wTile;
                if (pstart <= cs && pend >= ce) {                         // the chunk lies inside one page: every row is real, no mask
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) runmax[t][r] = f4w_max_acc(runmax[t][r], acc[t][r], kInf);
                    if (pend == ce && pl < np) finish();
                } else {
                    // a page boundary inside the chunk.  A range's last partial chunk always comes here (its last boundary is the
                    // range's end), so the zero rows the descriptors made up past it stay outside [lo, hi) of every page that is stored
                    while (true) {
                        const int lo = (pstart > cs ? pstart : cs) - cs, hi = (pend < ce ? pend : ce) - cs;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int row = (lane >> 4) * 4 + r;
                            if (row >= lo && row < hi)
#pragma unroll
                                for (int t = 0; t < NT; ++t) runmax[t][r] = f4w_max_acc(runmax[t][r], acc[t][r], kInf);
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

}  // namespace msim
