// The LIST form of fp6_wide_query.hip's scorer (include/maxsim.h: msim_f4w_candidates_q6): e2m3 (FP6) query tokens against the
// FP4 pages a candidate list names, and no other, at width 320.  The index is fp4_wide_index.hip's and the query code is
// fp6_wide_query.hip's; a score has the bits f4w_scores_q6_kernel writes for the same query and page.
//
//   f4w_candidates_q6_kernel<NT>  f4w_candidates_kernel (fp4_wide_candidates.hip) with the query fragment as 6 + 6 + 3 VGPRs per
//                                 tile (f4w_scores_q6_kernel's operand map) and B format code 2.  Everything else is that kernel's,
//                                 statement for statement: one WAVE per entry (q, j) of cand [n_q, m], four waves per workgroup,
//                                 the id, page-offset and query-offset checks, two bounds-checked buffer descriptors over the
//                                 page's own rows, f6w_cand_depth(NT) chunks ahead, three scaled MFMAs per (chunk, tile) chained
//                                 through C and issued block-major, one v_med3_f32 per accumulator, the always-masked last partial
//                                 chunk, the fold, the token-order sum from 0.0f by one lane, one store.
// It is a body of its own: it uses the constants and __forceinline__ helpers of fp4_wide_index.hip, fp4_wide_candidates.hip and
// fp6_wide_query.hip and instantiates none of their templates, so their units compile to the kernels they had
// (tools/kernel_diff.py).
// Nothing allocates or synchronises; the host never reads the list.  Every index is checked before it becomes an address, as in
// f4w_candidates_kernel; an entry that breaks a check is written as NaN, and only that entry.  Base addresses are formed in 64 bits.
#pragma once
#include "fp4_wide_candidates.hip"
#include "fp6_wide_query.hip"

namespace msim {

// chunks loaded ahead: 11 VGPRs each, and f4w_candidates_kernel's depths.  1, 2 and 4 tiles fit with four.  Beside 8 tiles the
// query fragment alone is 120 VGPRs (128 with the scale bytes), the accumulators and maxima 64 more: NO depth fits 256 VGPRs
// (depth 1: 256 + 20 AGPR copies, depth 2: 256 + 37; one wave per SIMD and no scratch either way), and holding the kernel to two
// waves with __launch_bounds__(256, 2) spills 76 (depth 1) or 148 (depth 2) bytes per lane to scratch, inside the chunk loop.  The
// resource report therefore does not decide between the two depths at NT = 8 (depth 1 has 17 fewer AGPR copies, depth 2 one more
// chunk in flight), and neither has been timed against the other: what decided is PLAN COMPATIBILITY -- with the e2m1 kernel's
// depths msim_f4w_candidates_plan describes both query codes and no second plan entry exists (the resource table of DESIGN 3.31)
constexpr int f6w_cand_depth(int NT) { return f4w_cand_depth(NT); }

// q6: [q_rows, 240] e2m3 fields; out_ids: [n_q, ld] or null
template <int NT>
__global__ __launch_bounds__(256) void f4w_candidates_q6_kernel(const uint8_t *__restrict__ q6, const uint8_t *__restrict__ qs,
                                                                const int32_t *__restrict__ q_off, int n_q, long long q_rows,
                                                                const uint8_t *__restrict__ d4, const uint8_t *__restrict__ ds,
                                                                const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0,
                                                                int n_d, long long d_rows, const int64_t *__restrict__ cand, int m,
                                                                long long ld_cand, long long id_base, float *__restrict__ scores,
                                                                long long ld, int64_t *__restrict__ out_ids) {
    static_assert(NT == 1 || NT == 2 || NT == 4 || NT == 8, "16-token tiles per query");
    constexpr int D = f6w_cand_depth(NT);
    constexpr float kNegInf = -__builtin_inff();
    const float kInf = __uint_as_float(0x7f800000u | ((uint32_t)n_d >> 31));   // +inf (n_d >= 0), opaque to the compiler: f4w_max_acc
    __shared__ float vals_all[kF4wCandWaves][NT * kF4wTile];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *vals = vals_all[wave];

    const long long e = (long long)blockIdx.x * kF4wCandWaves + wave;
    if (e >= (long long)n_q * m) return;                               // whole waves only: no workgroup barrier below
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    const int64_t id = cand[(size_t)q * ld_cand + j];
    const bool valid = id >= 0 && id >= id_base && id - id_base < (long long)n_d;
    if (out_ids && lane == 0) out_ids[(size_t)q * ld + j] = valid ? id : -1;
    float *dst = scores + (size_t)q * ld + j;
    if (!valid) {                                                      // no page: nothing is read
        if (lane == 0) *dst = kNegInf;
        return;
    }
    const int d = __builtin_amdgcn_readfirstlane((int)(id - id_base));
    const long long r0 = d_off[d], r1 = d_off[d + 1];
    if (r0 < 0 || r1 < r0 || r1 > d_rows || r1 - r0 > kF4wMaxRangeRows) {   // never trust a device offset with an address
        if (lane == 0) *dst = __builtin_nanf("");
        return;
    }
    const int nrows = __builtin_amdgcn_readfirstlane((int)(r1 - r0));
    if (nrows == 0) {
        if (lane == 0) *dst = kNegInf;
        return;
    }
    const long long qa = q_off[q], qe = q_off[q + 1];
    if (qa < 0 || qe < qa || qe > q_rows || qe - qa > NT * kF4wTile) {
        if (lane == 0) *dst = __builtin_nanf("");
        return;
    }
    const int ql = __builtin_amdgcn_readfirstlane((int)(qe - qa));
    if (ql == 0) {                                                     // a sum over no tokens
        if (lane == 0) *dst = 0.0f;
        return;
    }
    const bool c0 = clamp0 && clamp0[d];
    const int lrow = lane & 15, l4 = lane >> 4;                        // operand lane map: row lrow, lane group l4
    const int k01 = l4 * 16, k2 = 128 + l4 * 8;                        // page bytes k01 .. + 15 of blocks 0 (and, + 64, 1); k2 .. + 7 of block 2

    // the query fragments (B) and their scale bytes, in registers for the whole page; a slot without a token is a zero row (zero
    // fields, scale byte 0): it scores 0 and is never summed
    F6wRow qb[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tok = t * kF4wTile + lrow;
        f6w_zero_token(qb[t]);
        if (tok < ql) f6w_load_token(q6 + (qa + tok) * kF6wRow, qs[qa + tok], l4, qb[t]);
    }

    // two descriptors over the page's own rows: the code bytes and the scale bytes; past their ends both return zeros.  Their
    // inputs are made provably wave-uniform first, or every load below is wrapped in a waterfall loop
    const long long r0u = ((long long)__builtin_amdgcn_readfirstlane((int)(r0 >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)r0);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(d4 + r0u * kF4wRow), 0, nrows * kF4wRow,
                                                                        0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(ds + r0u), 0, nrows, 0x00020000);
    const int nch = (nrows + kF4wTile - 1) / kF4wTile;

    auto load = [&](int ch, F4wRow &dst_c) {
        const int row = ch * kF4wTile + lrow;
        dst_c.b0 = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4wRow + k01, 0, 0));
        dst_c.b1 = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4wRow + 64 + k01, 0, 0));
        dst_c.b2 = __builtin_bit_cast(f4w_i32x2, __builtin_amdgcn_raw_buffer_load_b64(rc, row * kF4wRow + k2, 0, 0));
        dst_c.s = (int)__builtin_amdgcn_raw_buffer_load_b8(rsc, row, 0, 0);
    };

    f32x4 runmax[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) runmax[t] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};

    F4wRow buf[D];
#pragma unroll
    for (int c = 0; c < D; ++c) load(c, buf[c]);
    for (int ch0 = 0; ch0 < nch; ch0 += D) {
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int ch = ch0 + c;
            if (ch >= nch) break;
            const f4w_i32x8 a0 = f4w_op(buf[c].b0), a1 = f4w_op(buf[c].b1), a2 = f4w_op(buf[c].b2);
            const int sa = buf[c].s;
            load(ch + D, buf[c]);
            // block-major over the tiles: NT independent MFMAs between two chained through C
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a0, sa, f6w_op(qb[t].b0), qb[t].s, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a1, sa, f6w_op(qb[t].b1), qb[t].s, acc[t]);
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = f6w_mfma(a2, sa, f6w_op(qb[t].b2), qb[t].s, acc[t]);
            // D: lane holds token (lane & 15) of each tile against chunk rows 4 (lane >> 4) + {0..3}
            const int left = nrows - ch * kF4wTile;                    // the page's rows from this chunk on
            if (left >= kF4wTile) {                                    // every row is the page's: no mask
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) runmax[t][r] = f4w_max_acc(runmax[t][r], acc[t][r], kInf);
            } else {
                // the page's last, partial chunk: the zero rows the descriptors made up past the end never reach a maximum
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (l4 * 4 + r < left)
#pragma unroll
                        for (int t = 0; t < NT; ++t) runmax[t][r] = f4w_max_acc(runmax[t][r], acc[t][r], kInf);
                }
            }
        }
    }

    // the page's end: fold the tiles' maxima, sum in token order, store
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        float mx = f4w_max(f4w_max(runmax[t][0], runmax[t][1]), f4w_max(runmax[t][2], runmax[t][3]));
        mx = f4w_max(mx, __shfl_xor(mx, 16));
        mx = f4w_max(mx, __shfl_xor(mx, 32));
        if (c0) mx = f4w_max(mx, 0.0f);
        if (lane < 16) vals[t * kF4wTile + lane] = mx;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0) {
        float T = 0.0f;
        for (int k = 0; k < ql; ++k) T += vals[k];
        *dst = T;
    }
}

}  // namespace msim
