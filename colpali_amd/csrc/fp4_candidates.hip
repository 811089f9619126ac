// The LIST form of the FP4 index's scorers (include/maxsim.h: msim_f4_candidates, msim_f4_candidates_q6): the FP4 score of the pages a
// candidate list names, and of no other -- the middle stage of a three-stage search (a cheap stage 1 makes a long list, the 65-byte
// FP4 rows cut it, the exact rerank orders the survivors).  The index and both query codes are those of fp4_index.hip (e2m1 tokens)
// and fp6_query.hip (e2m3 tokens); a score has the bits the scans write for the same query and page.
//
//   f4_candidates_kernel<NT,Q6>  one WAVE per entry (q, j) of cand [n_q, m], four waves per workgroup, one workgroup per four
//                                consecutive entries (res_candidates_kernel's work item; no inversion of the list, no workspace).
//                                The wave resolves its id, checks the page's and the query's offsets, holds the query's NT 16-token
//                                tiles in registers (Q6 = false: 4 VGPRs + the scale byte per tile, f4_scores_kernel's operand map;
//                                Q6 = true: 6 VGPRs per tile, f4_scores_q6_kernel's map, B format code 2) and streams the page's own
//                                rows as 16-row chunks behind two bounds-checked buffer descriptors (codes, scale bytes), kF4CandD
//                                chunks ahead: lane (row = lane & 15, l4 = lane >> 4) loads bytes 16 l4 .. 16 l4 + 15 of its row with
//                                one b128 load and the row's scale with a byte load.  ONE scaled MFMA per (chunk, tile); the
//                                running maxima start at -inf and take one v_med3_f32 per accumulator (f4_max_acc).  At the page's
//                                end the maxima are folded across lanes, clamped at 0 under clamp0, written to wave-private LDS and
//                                summed in token order by one lane from 0.0f -- f4_scores_kernel's `finish` -- and stored once.
// ROWS PAST THE PAGE'S END come back from the descriptors as zero rows (zero nibbles, scale byte 0), which score 0 and would beat
// every real row of an all-negative page.  They sit only in the page's last, partial chunk, and that chunk is always masked.
// It is a body of its own, as fp4_wide_index.hip and fp6_query.hip are: it instantiates no template of fp4_index.hip or
// fp6_query.hip, so the units of abi_fp4.hip and abi_fp6.hip compile to the kernels they had (tools/kernel_diff.py).
// Nothing allocates or synchronises; the host never reads the list.  Every index is checked before it becomes an address: the id
// against [id_base, id_base + n_d), the page's offsets against the row count and the range limit of the scan (2^23 rows: 32-bit
// buffer offsets), the query's offsets against the token count and the NT tiles the launch holds.  An entry that breaks one is
// written as NaN, and only that entry.  Base addresses are formed in 64 bits: a shard's code array may exceed 2 GiB.
#pragma once
#include "fp6_query.hip"

namespace msim {

constexpr int kF4CandD = 4;                 // chunks loaded ahead
constexpr int kF4CandWaves = 4;             // waves (entries) per workgroup
constexpr int kF4CandMaxTokens = 8 * kF4Tile;   // the longest query (NT = 8)
constexpr int kF4CandMaxPageRows = 1 << 23; // f4_scores_kernel's range limit

template <bool Q6>
struct F4CandQuery {
    typedef i32x4 frag;
};
template <>
struct F4CandQuery<true> {
    typedef i32x6 frag;
};

// q: [q_rows, 64] e2m1 codes (Q6 = false) or [q_rows, 96] e2m3 codes (Q6 = true); out_ids: [n_q, ld] or null
template <int NT, bool Q6>
__global__ __launch_bounds__(256) void f4_candidates_kernel(const uint8_t *__restrict__ qc, const uint8_t *__restrict__ qs,
                                                            const int32_t *__restrict__ q_off, int n_q, long long q_rows,
                                                            const uint8_t *__restrict__ d4, const uint8_t *__restrict__ ds,
                                                            const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0, int n_d,
                                                            long long d_rows, const int64_t *__restrict__ cand, int m, long long ld_cand,
                                                            long long id_base, float *__restrict__ scores, long long ld,
                                                            int64_t *__restrict__ out_ids) {
    static_assert(NT == 1 || NT == 2 || NT == 4 || NT == 8, "16-token tiles per query");
    typedef typename F4CandQuery<Q6>::frag qfrag;
    constexpr float kNegInf = -__builtin_inff();
    const float kInf = __uint_as_float(0x7f800000u | ((uint32_t)n_d >> 31));   // +inf (n_d >= 0), opaque to the compiler: f4_max_acc
    __shared__ float vals_all[kF4CandWaves][NT * kF4Tile];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *vals = vals_all[wave];

    const long long e = (long long)blockIdx.x * kF4CandWaves + wave;
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
    if (r0 < 0 || r1 < r0 || r1 > d_rows || r1 - r0 > kF4CandMaxPageRows) {   // never trust a device offset with an address
        if (lane == 0) *dst = __builtin_nanf("");
        return;
    }
    const int nrows = __builtin_amdgcn_readfirstlane((int)(r1 - r0));
    if (nrows == 0) {
        if (lane == 0) *dst = kNegInf;
        return;
    }
    const long long qa = q_off[q], qe = q_off[q + 1];
    if (qa < 0 || qe < qa || qe > q_rows || qe - qa > NT * kF4Tile) {
        if (lane == 0) *dst = __builtin_nanf("");
        return;
    }
    const int ql = __builtin_amdgcn_readfirstlane((int)(qe - qa));
    if (ql == 0) {                                                     // a sum over no tokens
        if (lane == 0) *dst = 0.0f;
        return;
    }
    const bool c0 = clamp0 && clamp0[d];
    const int lrow = lane & 15, l4 = lane >> 4, kq = l4 * 16;         // operand lane map: row lrow, bytes kq .. kq + 15

    // the query fragments (B) and their scale bytes, in registers for the whole page; a slot without a token is a zero row (zero
    // codes, scale byte 0): it scores 0 and is never summed
    qfrag qb[NT];
    int qsc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int tok = t * kF4Tile + lrow;
        qsc[t] = 0;
        if constexpr (Q6) {
            qb[t] = i32x6{0, 0, 0, 0, 0, 0};
            if (tok < ql) {
                // the lane's 24-byte group of 6-bit fields, 8-byte aligned: three b64 loads
                const i32x2 *src = reinterpret_cast<const i32x2 *>(qc + (qa + tok) * kF6Row + l4 * 24);
                const i32x2 w0 = src[0], w1 = src[1], w2 = src[2];
                qb[t] = i32x6{w0[0], w0[1], w1[0], w1[1], w2[0], w2[1]};
                qsc[t] = qs[qa + tok];
            }
        } else {
            qb[t] = i32x4{0, 0, 0, 0};
            if (tok < ql) {
                qb[t] = *reinterpret_cast<const i32x4 *>(qc + (qa + tok) * kF4Row + kq);
                qsc[t] = qs[qa + tok];
            }
        }
    }

    // two descriptors over the page's own rows: the code bytes and the scale bytes; past their ends both return zeros.  Their
    // inputs are made provably wave-uniform first, or every load below is wrapped in a waterfall loop
    const long long r0u = ((long long)__builtin_amdgcn_readfirstlane((int)(r0 >> 32)) << 32) |
                          (uint32_t)__builtin_amdgcn_readfirstlane((int)r0);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(d4 + r0u * kF4Row), 0, nrows * kF4Row,
                                                                        0x00020000);
    const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(ds + r0u), 0, nrows, 0x00020000);
    const int nch = (nrows + kF4Tile - 1) / kF4Tile;

    struct Chunk {
        i32x4 v;
        int s;
    };
    auto load = [&](int ch, Chunk &dst_c) {
        const int row = ch * kF4Tile + lrow;
        dst_c.v = __builtin_bit_cast(i32x4, __builtin_amdgcn_raw_buffer_load_b128(rc, row * kF4Row + kq, 0, 0));
        dst_c.s = (int)__builtin_amdgcn_raw_buffer_load_b8(rsc, row, 0, 0);
    };
    auto mfma = [&](const i32x4 &a, int sa, int t) {
        if constexpr (Q6) return f6_mfma(a, sa, qb[t], qsc[t]);
        else return f4_mfma(a, sa, qb[t], qsc[t]);
    };

    f32x4 runmax[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) runmax[t] = f32x4{kNegInf, kNegInf, kNegInf, kNegInf};

    Chunk buf[kF4CandD];
#pragma unroll
    for (int c = 0; c < kF4CandD; ++c) load(c, buf[c]);
    for (int ch0 = 0; ch0 < nch; ch0 += kF4CandD) {
#pragma unroll
        for (int c = 0; c < kF4CandD; ++c) {
            const int ch = ch0 + c;
            if (ch >= nch) break;
            const i32x4 a = buf[c].v;
            const int sa = buf[c].s;
            load(ch + kF4CandD, buf[c]);
            f32x4 acc[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma(a, sa, t);
            // D: lane holds token (lane & 15) of each tile against chunk rows 4 (lane >> 4) + {0..3}
            const int left = nrows - ch * kF4Tile;                     // the page's rows from this chunk on
            if (left >= kF4Tile) {                                     // every row is the page's: no mask
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) runmax[t][r] = f4_max_acc(runmax[t][r], acc[t][r], kInf);
            } else {
                // the page's last, partial chunk: the zero rows the descriptors made up past the end never reach a maximum
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (l4 * 4 + r < left)
#pragma unroll
                        for (int t = 0; t < NT; ++t) runmax[t][r] = f4_max_acc(runmax[t][r], acc[t][r], kInf);
                }
            }
        }
    }

    // the page's end: fold the tiles' maxima, sum in token order, store
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        float mx = f4_max(f4_max(runmax[t][0], runmax[t][1]), f4_max(runmax[t][2], runmax[t][3]));
        mx = f4_max(mx, __shfl_xor(mx, 16));
        mx = f4_max(mx, __shfl_xor(mx, 32));
        if (c0) mx = f4_max(mx, 0.0f);
        if (lane < 16) vals[t * kF4Tile + lane] = mx;
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
