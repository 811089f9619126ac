// E2M3 (FP6) query tokens against the FP4 pages of fp4_index.hip (include/maxsim.h: msim_f6_encode_rows, msim_f4_scores_q6).  The
// stored index does not change: v_mfma_scale_f32_16x16x128_f8f6f4 takes a format per operand, so the page rows stay the A operand
// (FP4, format code 4) and the query tokens become a B operand of format code 2, 6 VGPRs per lane, at the FP4 rate.  A batch of
// queries is a few kilobytes and sits in registers for a whole page range; its quantisation error was half of the first stage's.
//
// Query row code: a = max_k |x_k|; a == 0: every field 0, scale byte 127.  Otherwise e = the smallest integer with a <= 7.5 * 2^e,
//   clamped to [-32, 32]: a = m * 2^E (1 <= m < 2) gives e = E - 2 + (m > 1.875).  y_k = min(|x_k| * 2^-e, 7.5); code = the nearest
//   of the 32 e2m3 magnitudes (i/8 for codes 0 .. 7, (1 + i/8) * 2^j for code 8 (j + 1) + i), ties to the even code; field =
//   sign << 5 | code (0 when the code is 0).  A token is 96 code bytes: dimension k is the field at bit 6 (k mod 32) of the
//   little-endian 24-byte group k / 32 -- the B operand of lane group l4 = k / 32 -- and one scale byte e + 127.
// Score: as fp4_index.hip with v(q) a multiple of 1/8: I a multiple of 1/16, |I| <= 128 * 7.5 * 6 = 5760 (92 160 sixteenths < 2^24),
//   exact in fp32 in any order.
//
// Kernels:
//   f6_encode_rows_kernel        f4_encode_rows_kernel with the e2m3 grid: 16 lanes per token, each stores its 8 fields (6 bytes).
//   f4_scores_q6_kernel<NT,GW,D> f4_scores_kernel with the query fragment as 6 VGPRs per tile (three b64 loads at token * 96 +
//                                l4 * 24) and B format code 2.  The page side is that kernel's, statement for statement:
//                                descriptors, chunk loop, masked boundary path, v_med3_f32 running maximum, page-end fold, passes,
//                                XCD remap, GW waves per range.  It is a body of its own because f4_scores_kernel has to keep its
//                                bytes: behind a shared templated body the compiler emitted other code for it (tools/kernel_diff.py).
// With two formats the operand map is no longer symmetric.  The hardware meets nibble j of an FP4 lane with 6-bit field j of the
// FP6 lane, both ascending from the low bit of the lane's first register; the B scale is byte 0 of its register at op_sel 0; the
// mixed-format sum is exact (tests/test_gpu_fp6.py settles the three on hand-made data).
#pragma once
#include "fp4_index.hip"

namespace msim {

constexpr int kF6Row = kDim * 6 / 8;        // code bytes of an e2m3 query token

typedef __attribute__((ext_vector_type(6))) int i32x6;
typedef __attribute__((ext_vector_type(2))) int i32x2;

// The 6-bit field of one element: y = min(|x| * 2^-e, 7.5) rounded to the e2m3 grid -- steps of 1/8 below 2 (codes 0 .. 16: the
// subnormals i/8 and the binade of 1), of 1/4 in [2, 4) and of 1/2 in [4, 7.5] -- ties to the even code.  In each piece the code
// is an affine function of y with an even offset, exact in fp32 (y has at most 11 significant bits), so rintf's ties-to-even is
// the code's.
__device__ __forceinline__ uint32_t f6_field(float x, float inv) {
    const float y = __builtin_fminf(__builtin_fabsf(x) * inv, 7.5f);
    const float c = y < 2.0f ? 8.0f * y : y < 4.0f ? 4.0f * y + 8.0f : 2.0f * y + 16.0f;
    const uint32_t code = (uint32_t)__builtin_rintf(c);
    return code ? code | ((__float_as_uint(x) >> 31) << 5) : 0u;
}

// one token per 16 lanes, as f4_encode_rows_kernel: codes C [n_rows, 96] and scale bytes S [n_rows] of X [n_rows, 128].  Lane `sub`
// holds dimensions 8 sub .. 8 sub + 7: 48 bits at bit 48 (sub & 3) of the 24-byte group sub >> 2, which is byte 6 sub of the token.
template <bool F16>
__global__ __launch_bounds__(256) void f6_encode_rows_kernel(const uint16_t *__restrict__ X, long long n_rows, uint8_t *__restrict__ C,
                                                             uint8_t *__restrict__ S) {
    const int t = threadIdx.x, sub = t & 15;
    const long long r = (long long)blockIdx.x * 16 + (t >> 4);
    const bool live = r < n_rows;
    bf16x8 e = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) e = *reinterpret_cast<const bf16x8 *>(X + r * kDim + sub * 8);
    uint32_t a = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint32_t b = f4_abs_bits<F16>((uint16_t)e[u]);
        a = a > b ? a : b;
    }
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)a, s);
        a = a > o ? a : o;
    }
    // a = m * 2^E: a <= 7.5 * 2^e = 1.875 * 2^(e + 2) first holds at e = E - 2 when m <= 1.875 and at e = E - 1 above
    int ex = (int)(a >> 23) - 127 - 2 + ((a & 0x7fffffu) > 0x700000u ? 1 : 0);
    ex = ex < kF4MinExp ? kF4MinExp : ex > kF4MaxExp ? kF4MaxExp : ex;
    if (a == 0) ex = 0;
    const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);       // 2^-e, exact
    uint64_t w = 0;
#pragma unroll
    for (int u = 0; u < 8; ++u) w |= (uint64_t)f6_field(elem_to_float<F16>((uint16_t)e[u]), inv) << (6 * u);
    if (live) {
        uint16_t *dst = reinterpret_cast<uint16_t *>(C + r * kF6Row + sub * 6);
        dst[0] = (uint16_t)w;
        dst[1] = (uint16_t)(w >> 16);
        dst[2] = (uint16_t)(w >> 32);
        if (sub == 0) S[r] = (uint8_t)(ex + 127);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scorer
// 16 rows x 16 tokens over all 128 dimensions: A is FP4 (format code 4), B is e2m3 (format code 2), 24 bytes per lane; the scales
// as in f4_mfma
__device__ __forceinline__ f32x4 f6_mfma(const i32x4 &a, int sa, const i32x6 &b, int sb) {
    const i32x8 a8 = {a[0], a[1], a[2], a[3], 0, 0, 0, 0}, b8 = {b[0], b[1], b[2], b[3], b[4], b[5], 0, 0};
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 4, 2, 0, sa, 0, sb);
}

// the launch parameters are f4_scores_kernel's; q6: [q_rows, 96]
template <int NT, int GW, int D>
__global__ __launch_bounds__(256) void f4_scores_q6_kernel(const uint8_t *__restrict__ q6, const uint8_t *__restrict__ qs,
                                                           const int32_t *__restrict__ q_off, int n_q, long long q_rows, int QG, int TPQ,
                                                           int passes, const uint8_t *__restrict__ d4, const uint8_t *__restrict__ ds,
                                                           const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                                           long long d_rows, int ppw, int n_groups, int n_gb, float *__restrict__ scores,
                                                           long long ld) {
    static_assert(GW == 1 || GW == 2 || GW == 4, "waves per page range");
    constexpr int RW = 4 / GW;                                         // page ranges per workgroup
    constexpr float kNegInf = -__builtin_inff();
    const float kInf = __uint_as_float(0x7f800000u | ((uint32_t)n_d >> 31));   // +inf (n_d >= 0), opaque to the compiler: f4_max_acc
    __shared__ float vals_all[4][NT * kF4Tile];
    __shared__ float part_all[4][kF4MaxRange];
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
    const bool range_ok = !__builtin_amdgcn_ballot_w64(bad_page) && R1 - R0 <= (1 << 23);   // 32-bit buffer offsets below

    // the group's queries: lane s < QG holds query g * QG + s
    const long long qi_l = (long long)g * QG + lane;
    int qa = 0, ql = 0, qok = 0;
    if (lane < QG && qi_l < n_q) {
        const long long a = q_off[qi_l], b = q_off[qi_l + 1];
        qok = a >= 0 && b >= a && b <= q_rows && b - a <= (long long)passes * TPQ * kF4Tile;
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
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(d4 + (long long)R0 * kF4Row), 0,
                                                                        (R1 - R0) * kF4Row, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(ds + R0), 0, R1 - R0, 0x00020000);
    const int nrows = R1 - R0, nch = (nrows + kF4Tile - 1) / kF4Tile;
    const int lrow = lane & 15, l4 = lane >> 4, kq = l4 * 16;         // operand lane map: row lrow, bytes kq .. kq + 15

    struct Chunk {
        i32x4 v;
        int s;
    };

    for (int pass = 0; pass < passes; ++pass) {
        // the query fragments (B) and their scale bytes of this pass, in registers for the whole page range; a slot without a
        // token is a zero row (zero fields, scale byte 0): it scores 0 and is never summed
        i32x6 qb[NT];
        int qsc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int s = t / TPQ, tok = (pass * NT + t % TPQ) * kF4Tile + lrow;
            const int a = __shfl(qa, s), l = __shfl(ql, s);
            qb[t] = i32x6{0, 0, 0, 0, 0, 0};
            qsc[t] = 0;
            if (s < nqs && tok < l) {
                // the lane's 24-byte group of 6-bit fields, 8-byte aligned: three b64 loads
                const i32x2 *src = reinterpret_cast<const i32x2 *>(q6 + (long long)(a + tok) * kF6Row + l4 * 24);
                const i32x2 w0 = src[0], w1 = src[1], w2 = src[2];
                qb[t] = i32x6{w0[0], w0[1], w1[0], w1[1], w2[0], w2[1]};
                qsc[t] = qs[a + tok];
            }
        }

        auto load = [&](int ch, Chunk &dst) {
            const int row = ch * kF4Tile + lrow;
            dst.v = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4Row + kq, 0, 0));
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
                float m = f4_max(f4_max(runmax[t][0], runmax[t][1]), f4_max(runmax[t][2], runmax[t][3]));
                m = f4_max(m, __shfl_xor(m, 16));
                m = f4_max(m, __shfl_xor(m, 32));
                if (c0) m = f4_max(m, 0.0f);
                if (lane < 16) vals[t * kF4Tile + lane] = m;
                runmax[t] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (lane < nqs) {
                float T = pass ? part[pl] : 0.0f;
                const int lo = pass * NT * kF4Tile, hi = ql < lo + TPQ * kF4Tile ? ql : lo + TPQ * kF4Tile;
                const float *v = vals + lane * TPQ * kF4Tile - lo;
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

        Chunk buf[D];
#pragma unroll
        for (int d = 0; d < D; ++d) load(d, buf[d]);
        for (int ch0 = 0; ch0 < nch; ch0 += D) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int ch = ch0 + d;
                if (ch >= nch) break;
                const i32x4 a = buf[d].v;
                const int sa = buf[d].s;
                load(ch + D, buf[d]);
                f32x4 acc[NT];
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = f6_mfma(a, sa, qb[t], qsc[t]);
                // D: lane holds token (lane & 15) of each tile against chunk rows 4 (lane >> 4) + {0..3}
                const int cs = ch * kF4Tile, ce = cs + kF4Tile;
                if (pstart <= cs && pend >= ce) {                         // the chunk lies inside one page: every row is real, no mask
#pragma unroll
                    for (int t = 0; t < NT; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) runmax[t][r] = f4_max_acc(runmax[t][r], acc[t][r], kInf);
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
                                for (int t = 0; t < NT; ++t) runmax[t][r] = f4_max_acc(runmax[t][r], acc[t][r], kInf);
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
