// E2M3 (FP6) query tokens against the FP4 pages of fp4_wide_index.hip, width 320 (include/maxsim.h: msim_f6w_encode_rows,
// msim_f4w_scores_q6): fp6_query.hip's step for the wide index.  The stored index does not change:
// v_mfma_scale_f32_16x16x128_f8f6f4 takes a format per operand, so the 161-byte page rows stay the A operand (FP4, format code 4)
// and the query tokens become a B operand of format code 2.  A batch of queries is a few kilobytes and sits in registers for a
// whole page range.
//
// Query row code: msim_f6_encode_rows' rule over 320 dimensions.  a = max over all 320 |x_k|; a == 0: every field 0, scale byte
//   127.  Otherwise e = the smallest integer with a <= 7.5 * 2^e, clamped to [-32, 32]: a = m * 2^E (1 <= m < 2) gives
//   e = E - 2 + (m > 1.875).  y_k = min(|x_k| * 2^-e, 7.5); code = the nearest of the 32 e2m3 magnitudes (i/8 for codes 0 .. 7,
//   (1 + i/8) * 2^j for code 8 (j + 1) + i), ties to the even code; field = sign << 5 | code (0 when the code is 0).  A token is
//   240 code bytes -- dimension k is the 6-bit field at bit 6 k of the little-endian row -- and one scale byte e + 127.
// Operand map, lane group l4 = lane >> 4 (the partners of the FP4 bytes f4w_scores_kernel loads there):
//   K blocks 0 and 1 (b = 0, 1): the lane's 24 bytes at byte 96 b + 24 l4 are dimensions 128 b + 32 l4 .. + 31: six registers.
//   K block 2: the lane's 12 bytes at byte 192 + 12 l4 are dimensions 256 + 16 l4 .. + 15, fields 0 .. 15 of the operand: three
//              registers, registers 3 .. 5 zero -- beside the page side's 8 bytes (nibbles 0 .. 15, registers 2 and 3 zero).
// Score: as fp4_wide_index.hip with v(q) a multiple of 1/8: I a multiple of 1/16, |I| <= 320 * 7.5 * 6 = 14 400 (230 400
//   sixteenths < 2^24), and so is every partial sum through the chained C operand: exact in fp32 in any order.
//
// Kernels:
//   f6w_encode_rows_kernel        f4w_encode_rows_kernel with the e2m3 grid: 8 lanes per token, 40 elements each; a lane stores its
//                                 40 fields (30 bytes at byte 30 sub of the token) as fifteen 16-bit words.
//   f4w_scores_q6_kernel<NT,GW,D> f4w_scores_kernel with the query fragment as 6 + 6 + 3 VGPRs per tile and B format code 2.  The
//                                 page side is that kernel's, statement for statement: descriptors, chunk loop, masked boundary
//                                 path, v_med3_f32 running maximum, page-end fold, passes, XCD remap, GW waves per range.  It is a
//                                 body of its own because f4w_scores_kernel has to keep its bytes (tools/kernel_diff.py); this
//                                 file uses fp4_wide_index.hip's constants and __forceinline__ helpers and instantiates none of
//                                 its templates.
// With two formats the wide kernel's symmetry argument ("the same function on A and B, so the order of k inside the instruction
// does not matter") no longer holds.  What holds instead is the fact fp6_query.hip records -- nibble j of an FP4 lane meets 6-bit
// field j of the FP6 lane, both ascending from the low bit of the lane's first register -- and, new here, that it holds in a
// HALF-FILLED block: fields 0 .. 15 of a lane meet nibbles 0 .. 15, and the zero registers above them contribute nothing
// (tests/test_gpu_fp6_wide.py settles both on hand-made data, every dimension of block 2 on its own).
#pragma once
#include "fp4_wide_index.hip"

namespace msim {

constexpr int kF6wRow = kF4wDim * 6 / 8;     // code bytes of an e2m3 query token: 240

typedef __attribute__((ext_vector_type(6))) int f6w_i32x6;
typedef __attribute__((ext_vector_type(3))) int f6w_i32x3;

// The 6-bit field of one element: y = min(|x| * 2^-e, 7.5) rounded to the e2m3 grid -- steps of 1/8 below 2 (codes 0 .. 16: the
// subnormals i/8 and the binade of 1), of 1/4 in [2, 4) and of 1/2 in [4, 7.5] -- ties to the even code.  In each piece the code
// is an affine function of y with an even offset, exact in fp32 (y has at most 11 significant bits), so rintf's ties-to-even is
// the code's.
__device__ __forceinline__ uint32_t f6w_field(float x, float inv) {
    const float y = __builtin_fminf(__builtin_fabsf(x) * inv, 7.5f);
    const float c = y < 2.0f ? 8.0f * y : y < 4.0f ? 4.0f * y + 8.0f : 2.0f * y + 16.0f;
    const uint32_t code = (uint32_t)__builtin_rintf(c);
    return code ? code | ((__float_as_uint(x) >> 31) << 5) : 0u;
}

// one token per 8 lanes, as f4w_encode_rows_kernel: codes C [n_rows, 240] and scale bytes S [n_rows] of X [n_rows, 320].  Lane
// `sub` holds dimensions 40 sub .. 40 sub + 39: 240 bits at bit 240 sub of the row, which is byte 30 sub of the token.
template <bool F16>
__global__ __launch_bounds__(256) void f6w_encode_rows_kernel(const uint16_t *__restrict__ X, long long n_rows, uint8_t *__restrict__ C,
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
    // a = m * 2^E: a <= 7.5 * 2^e = 1.875 * 2^(e + 2) first holds at e = E - 2 when m <= 1.875 and at e = E - 1 above
    int ex = (int)(a >> 23) - 127 - 2 + ((a & 0x7fffffu) > 0x700000u ? 1 : 0);
    ex = ex < kF4wMinExp ? kF4wMinExp : ex > kF4wMaxExp ? kF4wMaxExp : ex;
    if (a == 0) ex = 0;
    const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);       // 2^-e, exact
    if (live) {
#pragma unroll
        for (int v = 0; v < 5; ++v) {
            uint64_t w = 0;
#pragma unroll
            for (int u = 0; u < 8; ++u) w |= (uint64_t)f6w_field(elem_to_float<F16>((uint16_t)e[v][u]), inv) << (6 * u);
            uint16_t *dst = reinterpret_cast<uint16_t *>(C + r * kF6wRow + sub * 30 + v * 6);
            dst[0] = (uint16_t)w;
            dst[1] = (uint16_t)(w >> 16);
            dst[2] = (uint16_t)(w >> 32);
        }
        if (sub == 0) S[r] = (uint8_t)(ex + 127);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scorer
// One K block of 16 rows x 16 tokens added to c: A is FP4 (format code 4), B is e2m3 (format code 2); the scales and the C operand
// as in f4w_mfma
__device__ __forceinline__ f32x4 f6w_mfma(const f4w_i32x8 &a, int sa, const f4w_i32x8 &b, int sb, const f32x4 &c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 4, 2, 0, sa, 0, sb);
}

// a query token's operand registers in one lane: K blocks 0 and 1 (24 bytes each) and the lane's 12 bytes of block 2
struct F6wRow {
    f6w_i32x6 b0, b1;
    f6w_i32x3 b2;
    int s;
};

__device__ __forceinline__ f4w_i32x8 f6w_op(const f6w_i32x6 &v) { return f4w_i32x8{v[0], v[1], v[2], v[3], v[4], v[5], 0, 0}; }
__device__ __forceinline__ f4w_i32x8 f6w_op(const f6w_i32x3 &v) { return f4w_i32x8{v[0], v[1], v[2], 0, 0, 0, 0, 0}; }

// the lane's fragment of the token whose 240 code bytes start at `row` (16-byte aligned: 240 = 15 * 16) and whose scale byte is
// `sc`: blocks 0 and 1 at an 8-byte boundary (three b64 loads each), block 2 at a 4-byte boundary (three b32 loads)
__device__ __forceinline__ void f6w_load_token(const uint8_t *row, int sc, int l4, F6wRow &dst) {
    const f4w_i32x2 *s0 = reinterpret_cast<const f4w_i32x2 *>(row + l4 * 24);
    const f4w_i32x2 *s1 = reinterpret_cast<const f4w_i32x2 *>(row + 96 + l4 * 24);
    const int *s2 = reinterpret_cast<const int *>(row + 192 + l4 * 12);
    const f4w_i32x2 u0 = s0[0], u1 = s0[1], u2 = s0[2], w0 = s1[0], w1 = s1[1], w2 = s1[2];
    dst.b0 = f6w_i32x6{u0[0], u0[1], u1[0], u1[1], u2[0], u2[1]};
    dst.b1 = f6w_i32x6{w0[0], w0[1], w1[0], w1[1], w2[0], w2[1]};
    dst.b2 = f6w_i32x3{s2[0], s2[1], s2[2]};
    dst.s = sc;
}

__device__ __forceinline__ void f6w_zero_token(F6wRow &dst) {
    dst.b0 = dst.b1 = f6w_i32x6{0, 0, 0, 0, 0, 0};
    dst.b2 = f6w_i32x3{0, 0, 0};
    dst.s = 0;
}

// the launch parameters are f4w_scores_kernel's; q6: [q_rows, 240]
template <int NT, int GW, int D>
__global__ __launch_bounds__(256) void f4w_scores_q6_kernel(const uint8_t *__restrict__ q6, const uint8_t *__restrict__ qs,
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
    const int k01 = l4 * 16, k2 = 128 + l4 * 8;                        // page bytes k01 .. + 15 of blocks 0 (and, + 64, 1); k2 .. + 7 of block 2

    for (int pass = 0; pass < passes; ++pass) {
        // the query fragments (B) and their scale bytes of this pass, in registers for the whole page range; a slot without a
        // token is a zero row (zero fields, scale byte 0): it scores 0 and is never summed
        F6wRow qb[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int s = t / TPQ, tok = (pass * NT + t % TPQ) * kF4wTile + lrow;
            const int a = __shfl(qa, s), l = __shfl(ql, s);
            f6w_zero_token(qb[t]);
            if (s < nqs && tok < l) f6w_load_token(q6 + (long long)(a + tok) * kF6wRow, qs[a + tok], l4, qb[t]);
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
                for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a0, sa, f6w_op(qb[t].b0), qb[t].s, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a1, sa, f6w_op(qb[t].b1), qb[t].s, acc[t]);
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a2, sa, f6w_op(qb[t].b2), qb[t].s, acc[t]);
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
