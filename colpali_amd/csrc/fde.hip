// Fixed dimensional encodings (FDE; Dhulipala et al., "MUVERA: Multi-Vector Retrieval via Fixed Dimensional Encodings", NeurIPS
// 2024) for gfx950 (MI355X): a cheap first stage for two-stage search.  Every multi-vector page and query becomes ONE vector of F
// values, and the inner product of a query's and a page's encodings approximates their MaxSim (Chamfer similarity).
//
// The encoding (include/maxsim.h: msim_fde_encode_docs) with R reps, k_sim sign bits and d_proj projected values per bucket,
// B = 2^k_sim, F = R * B * d_proj, host-drawn G [R, k_sim, 128] (normal) and S [R, d_proj, 128] (+-1), both fp32:
//   bucket      phi_r(x) = sum_i 2^i [<G[r, i], x> > 0]
//   projection  psi_r(x) = S[r] x / sqrt(d_proj)
//   entry (r * B + b) * d_proj + j of the FDE = psi_r(v)[j], where v is
//     query:    the SUM of the query's tokens with phi_r = b (zeros if none)
//     document: the MEAN of the page's rows with phi_r = b; an empty bucket with fill_empty takes the row p whose phi_r(p) is
//               nearest to b in Hamming distance (lowest row index on a tie); zeros otherwise, and for a 0-row page.
//
// Kernels:
//   fde_encode_kernel  one 256-thread workgroup per page (or query), rep by rep, all in fp32, rounded once on store:
//                      1. codes: 4 lanes per row, each a 32-column slice of the k_sim dots against G[r] (fp32 from LDS), folded by
//                         two xor-shuffles (the same order in every lane).  Bucket counts and each bucket's first row are LDS
//                         integer atomics (add / min): their results do not depend on the order the atomics ran in.
//                      2. bucket sums: lane (column c, half h) owns sums[h][b][c] for every b and adds its rows in row order; the
//                         two halves are added at the end.  The order depends on the row count only, so reruns are bit-identical.
//                      3. mean (or sum), fill-empty by an integer search over the B codes' first rows, then the projection: one
//                         output per lane, a 128-term dot with S[r] in a fixed order.
//                      The sign dots need fp32 G (a bf16 G would move codes near the hyperplanes), so they run on the vector ALUs;
//                      the projection is applied after averaging (F x 128 FMAs per page, not rows x R x d_proj x 128).
//   fde_scores_kernel  scores[q, c] = <Fq[q], Fd[c]>: a streamed MFMA GEMM (v_mfma_f32_16x16x32 bf16 / f16).  A workgroup owns QB
//                      queries x DB pages; 64-wide k-tiles of both operands stream through an NBUF-deep LDS ring by LDS-DMA
//                      (buffer_load ... lds, 16 B per lane), the 16-byte chunk of each 128-byte row XOR-swizzled on the SOURCE
//                      address so that the fragment reads are bank-conflict free.  Every score is the same sequence of MFMAs over
//                      k-tiles 0 .. F/64 - 1, whatever tile shape or batch the query shares: its bits depend on F only.
// Nothing allocates or synchronises; every address comes from a checked index (row ranges against the row count, tiles through
// buffer descriptors whose bounds return zeros).  A page whose offsets disagree with the row count gets NaN everywhere.
#pragma once
#include "maxsim_common.hpp"
#include "maxsim_stream.hip"

namespace msim {

constexpr int kFdeMaxKsim = 6;
constexpr int kFdeChunk = 64;              // rows per code pass (4 lanes per row)
constexpr int kFdeSumStride = kDim + 1;    // LDS row stride of the bucket sums: the projection's lanes read 4 buckets conflict-free

// LDS bytes of fde_encode_kernel for one configuration
__host__ __device__ constexpr int fde_encode_lds_bytes(int ksim, int dproj) {
    return (2 * (1 << ksim) * kFdeSumStride + ksim * kDim + kDim * dproj) * 4 + (2 * 64 + kFdeChunk) * 4;
}

template <bool F16>
__device__ __forceinline__ uint16_t fde_store_elem(float x) {
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)x);
    else return __builtin_bit_cast(uint16_t, (__bf16)x);
}

// one workgroup per item (page or query): rows off[item] .. off[item + 1] - 1 of X [n_rows, 128]
template <bool F16>
__global__ __launch_bounds__(256) void fde_encode_kernel(const uint16_t *__restrict__ X, const int32_t *__restrict__ off, int n_items,
                                                         long long n_rows, const float *__restrict__ G, const float *__restrict__ S,
                                                         int R, int ksim, int dproj, int is_doc, int fill_empty,
                                                         uint16_t *__restrict__ out, uint8_t *__restrict__ codes) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int B = 1 << ksim;
    float *sums = reinterpret_cast<float *>(smem);                  // [2][B][kFdeSumStride]
    float *Gs = sums + 2 * B * kFdeSumStride;                        // [ksim][128]
    float *St = Gs + ksim * kDim;                                    // [128][dproj]: St[c][j] = S[r][j][c]
    int *cnt = reinterpret_cast<int *>(St + kDim * dproj);           // [64]
    int *first = cnt + 64;                                           // [64]
    int *code_buf = first + 64;                                      // [kFdeChunk]
    const int t = threadIdx.x;
    const int item = blockIdx.x;
    if (item >= n_items) return;
    const long long F = (long long)R * B * dproj;
    uint16_t *o = out + (size_t)item * F;
    const long long r0 = off[item], r1 = off[item + 1];
    if (r0 < 0 || r1 < r0 || r1 > n_rows) {                          // never trust a device offset with an address
        const uint16_t nan = F16 ? 0x7e00 : 0x7fc0;
        for (long long f = t; f < F; f += 256) o[f] = nan;
        return;
    }
    const int n = (int)(r1 - r0);
    const uint16_t *x = X + (size_t)r0 * kDim;
    const float inv_sqrt = 1.0f / __builtin_sqrtf((float)dproj);
    const int c = t & (kDim - 1), h = t >> 7;                        // the bucket-sum lane: column, half
    const int crow = t >> 2, part = t & 3;                           // the code lane: row of the chunk, 32-column slice

    for (int r = 0; r < R; ++r) {
        for (int i = t; i < ksim * kDim; i += 256) Gs[i] = G[(size_t)r * ksim * kDim + i];
        for (int i = t; i < dproj * kDim; i += 256) {
            const int j = i / kDim, cc = i - j * kDim;               // coalesced read of S[r][j][cc]
            St[cc * dproj + j] = S[(size_t)r * dproj * kDim + i];
        }
        for (int i = t; i < 2 * B * kFdeSumStride; i += 256) sums[i] = 0.0f;
        if (t < 64) {
            cnt[t] = 0;
            first[t] = 0x7fffffff;
        }
        __syncthreads();

        for (int c0 = 0; c0 < n; c0 += kFdeChunk) {
            // 1. codes of rows c0 .. c0 + 63
            const int row = c0 + crow;
            const bool live = row < n;
            float dot[kFdeMaxKsim];
#pragma unroll
            for (int k = 0; k < kFdeMaxKsim; ++k) dot[k] = 0.0f;
            if (live) {
                const bf16x8 *src = reinterpret_cast<const bf16x8 *>(x + (size_t)row * kDim + part * 32);
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const bf16x8 e = src[v];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float xv = elem_to_float<F16>((uint16_t)e[u]);
                        const int col = part * 32 + v * 8 + u;
#pragma unroll
                        for (int k = 0; k < kFdeMaxKsim; ++k)
                            if (k < ksim) dot[k] = __builtin_fmaf(Gs[k * kDim + col], xv, dot[k]);
                    }
                }
            }
            int code = 0;
#pragma unroll
            for (int k = 0; k < kFdeMaxKsim; ++k) {
                float d = dot[k];
                d += __shfl_xor(d, 1);                               // (p0 + p1) + (p2 + p3) in every lane of the four
                d += __shfl_xor(d, 2);
                if (k < ksim && d > 0.0f) code |= 1 << k;
            }
            if (live && part == 0) {
                code_buf[crow] = code;
                atomicAdd(&cnt[code], 1);
                atomicMin(&first[code], row);
                if (codes) codes[(size_t)(r0 + row) * R + r] = (uint8_t)code;
            }
            __syncthreads();
            // 2. bucket sums: lane (c, h) takes rows 32 h .. 32 h + 31 of the chunk, in order
            const int end = n - c0 < kFdeChunk ? n - c0 : kFdeChunk;
            float *mine = sums + h * B * kFdeSumStride + c;
            for (int i = h * 32; i < end && i < h * 32 + 32; ++i) {
                const int b = code_buf[i];
                mine[b * kFdeSumStride] += elem_to_float<F16>(x[(size_t)(c0 + i) * kDim + c]);
            }
            __syncthreads();
        }

        // 3. the vector of every bucket, into sums[0][b]
        for (int b = h; b < B; b += 2) {
            const int nb = cnt[b];
            float v = 0.0f;
            if (nb > 0) {
                v = sums[b * kFdeSumStride + c] + sums[(B + b) * kFdeSumStride + c];
                if (is_doc) v = v / (float)nb;
            } else if (is_doc && fill_empty && n > 0) {
                int best_d = 99, best_row = 0x7fffffff;
                for (int b2 = 0; b2 < B; ++b2) {
                    if (cnt[b2] == 0) continue;
                    const int d = __popc((unsigned)(b ^ b2));
                    const int fr = first[b2];
                    if (d < best_d || (d == best_d && fr < best_row)) {
                        best_d = d;
                        best_row = fr;
                    }
                }
                if (best_row >= 0 && best_row < n) v = elem_to_float<F16>(x[(size_t)best_row * kDim + c]);
            }
            sums[b * kFdeSumStride + c] = v;
        }
        __syncthreads();

        // 4. projection: output (b, j) = sum_c S[r][j][c] v_b[c] / sqrt(d_proj)
        for (int oi = t; oi < B * dproj; oi += 256) {
            const int b = oi / dproj, j = oi - b * dproj;
            const float *vb = sums + b * kFdeSumStride;
            float acc = 0.0f;
            for (int cc = 0; cc < kDim; ++cc) acc = __builtin_fmaf(St[cc * dproj + j], vb[cc], acc);
            o[((size_t)r * B + b) * dproj + j] = fde_store_elem<F16>(acc * inv_sqrt);
        }
        __syncthreads();                                             // LDS is rewritten by the next rep
    }
}

// ---------------------------------------------------------------------------------------------------------------- the scorer
constexpr int kFdeKT = 64;                  // k-tile: 64 elements = one 128-byte row piece
constexpr int kFdeRowBytes = kFdeKT * 2;

template <int QB, int DB, int NBUF>
constexpr int fde_scores_lds_bytes() { return NBUF * (QB + DB) * kFdeRowBytes; }

// byte offset of logical 16-byte chunk `c` of tile row `r`: the chunk XOR-ed with (r >> 1) & 7, so that 16 consecutive rows of one
// chunk (an MFMA operand read) cover all 64 banks
__device__ __forceinline__ int fde_swz(int r, int c) { return r * kFdeRowBytes + ((c ^ ((r >> 1) & 7)) << 4); }

template <int QB, int DB, int NBUF, bool F16>
__global__ __launch_bounds__(256) void fde_scores_kernel(const uint16_t *__restrict__ Fq, int n_q, const uint16_t *__restrict__ Fd,
                                                         int n_d, int F, float *__restrict__ scores, long long ld, int n_qt,
                                                         int vec_store) {
    static_assert(QB % 32 == 0 && DB % 32 == 0 && NBUF >= 2, "tile shape");
    constexpr int MT = DB / 32, NT = QB / 32;          // 16x16 tiles per wave (2 x 2 waves)
    constexpr int LD = DB / 32, LQ = QB / 32;          // LDS-DMA pieces (8 rows x 128 B) per wave and stage
    constexpr int STAGE = (QB + DB) * kFdeRowBytes;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wd = wave >> 1, wq = wave & 1;

    // XCD-aware bijective remap: the query tiles of one page tile run on one XCD, back to back, and share its L2
    const int nwg = gridDim.x, orig = blockIdx.x;
    const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
    const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
    const int qt = wgid % n_qt, dt = wgid / n_qt;
    const int q0 = qt * QB, d0 = dt * DB;
    if (q0 >= n_q || d0 >= n_d) return;
    const int nq_here = n_q - q0 < QB ? n_q - q0 : QB, nd_here = n_d - d0 < DB ? n_d - d0 : DB;
    // bounds-checked descriptors: a row past the tile's last page / query reads zeros
    const __amdgpu_buffer_rsrc_t rs_d =
        __builtin_amdgcn_make_buffer_rsrc((void *)(Fd + (size_t)d0 * F), 0, nd_here * F * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_q =
        __builtin_amdgcn_make_buffer_rsrc((void *)(Fq + (size_t)q0 * F), 0, nq_here * F * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_null = __builtin_amdgcn_make_buffer_rsrc((void *)Fd, 0, 0, 0x00020000);

    // lane's source row within an 8-row piece and the logical chunk that lands in its linear LDS slot
    const int prow = lane >> 3;
    const int KT = F / kFdeKT;
    auto issue = [&](int kt, int slot) {
        const bool live = kt < KT;                     // past the end: empty loads keep the number in flight constant
        char *st = smem + slot * STAGE;
        const int koff = live ? kt * kFdeRowBytes : 0;    // in the VGPR offset: the descriptor's range check covers all of it
#pragma unroll
        for (int i = 0; i < LD; ++i) {
            const int r = wave * (DB / 4) + i * 8 + prow;
            const int voff = r * F * 2 + koff + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(live ? rs_d : rs_null, MSIM_LDS(st + (wave * (DB / 4) + i * 8) * kFdeRowBytes), 16,
                                                     voff, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < LQ; ++i) {
            const int r = wave * (QB / 4) + i * 8 + prow;
            const int voff = r * F * 2 + koff + (((lane & 7) ^ ((r >> 1) & 7)) << 4);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(live ? rs_q : rs_null,
                                                     MSIM_LDS(st + DB * kFdeRowBytes + (wave * (QB / 4) + i * 8) * kFdeRowBytes), 16,
                                                     voff, 0, 0, 0);
        }
    };

    f32x4 acc[MT][NT];
#pragma unroll
    for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int nn = 0; nn < NT; ++nn) acc[m][nn] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s) issue(s, s);
    int slot = 0, nslot = NBUF - 1;
    for (int kt = 0; kt < KT; ++kt) {
        wait_vmcnt<(LD + LQ) * (NBUF - 2)>();          // this wave's pieces of k-tile kt have landed
        __builtin_amdgcn_s_barrier();                  // ... and every wave's; every wave is done reading k-tile kt - 1
        issue(kt + NBUF - 1, nslot);                   // into the slot k-tile kt - 1 used
        const char *st = smem + slot * STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int ch = ks * 4 + (lane >> 4);
            bf16x8 a[MT], b[NT];
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                const int r = wd * (DB / 2) + m * 16 + (lane & 15);
                a[m] = *reinterpret_cast<const bf16x8 *>(st + fde_swz(r, ch));
            }
#pragma unroll
            for (int nn = 0; nn < NT; ++nn) {
                const int r = wq * (QB / 2) + nn * 16 + (lane & 15);
                b[nn] = *reinterpret_cast<const bf16x8 *>(st + DB * kFdeRowBytes + fde_swz(r, ch));
            }
#pragma unroll
            for (int m = 0; m < MT; ++m)
#pragma unroll
                for (int nn = 0; nn < NT; ++nn) acc[m][nn] = mfma16<F16>(a[m], b[nn], acc[m][nn]);
        }
        slot = slot + 1 == NBUF ? 0 : slot + 1;
        nslot = nslot + 1 == NBUF ? 0 : nslot + 1;
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's fragment reads are done before the next barrier
    }
    wait_vmcnt<0>();                                   // the empty loads past the end

    // D: lane holds query (lane & 15) of its 16-query tile and pages 4 (lane >> 4) + {0..3} of its 16-page tile
#pragma unroll
    for (int nn = 0; nn < NT; ++nn) {
        const int q = q0 + wq * (QB / 2) + nn * 16 + (lane & 15);
        if (q >= n_q) continue;
        float *row = scores + (size_t)q * ld;
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            const int d = d0 + wd * (DB / 2) + m * 16 + (lane >> 4) * 4;
            if (vec_store && d + 3 < n_d) {
                *reinterpret_cast<f32x4 *>(row + d) = acc[m][nn];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d + j < n_d) row[d + j] = acc[m][nn][j];
            }
        }
    }
}

}  // namespace msim
