// Rows out of a 320-wide residual-compressed shard, decoded inside the kernel that consumes them, for gfx950 (MI355X)
// (include/maxsim.h: msim_res_wide_align_candidates, msim_res_wide_gather_pages).  The width-320 siblings of residual_align.hip: no
// full-precision copy of a listed page exists in memory at any point.
//
//   res_wide_align_kernel         K1a at DIM = 320 (maxsim_align.hip) with a decoding loader: one 4-wave workgroup per entry (q, j),
//                                 wave w owns the token tiles w and w + 4 in registers (the B operand, 2 x 40 VGPRs), the page streams
//                                 in 16-row chunks (the A operand), ONE chain of ten v_mfma_f32_16x16x32 from zero per (chunk, tile),
//                                 ks ascending 0 .. 9, the tail rows re-read the page's last row and are masked to -inf AFTER the MFMA,
//                                 the running (max, first row) per lane, the lowest-row fold, the map stores and fills and the bad /
//                                 clamp0 / padding-slot epilogue are K1a's, line for line.  Only the loader differs: lane (l16, l4)
//                                 needs dimensions 32 ks + 8 l4 .. + 8 of chunk row l16 (ks = 0 .. 9), and gets them from the row's
//                                 code (compared with K before it becomes an address), the 16-byte chunks 4 ks + l4 of C[code]
//                                 (through L2: K x 640 B is 160 KiB .. 1.25 MiB) and the fields rw_load_field(row, 4 ks + l4), decoded
//                                 by rw_decode_chunk -- the helper res_wide_decode_kernel decodes with, so the operand has the bits of
//                                 the decompressed row and every similarity the bits K1a gives over it.  A code >= K makes the operand
//                                 the NaN pattern res_wide_decode_kernel writes.  The RAW loads of chunk c + 1 (1 code, 10 centroid
//                                 chunks, 10 fields: 51 registers) fly under the MFMAs of chunk c; the decode happens at use.
//                                 Every wave that holds tokens decodes the chunk itself, as res_align_kernel: up to four times the
//                                 decode ALU and L2 traffic per entry, and in exchange no LDS staging and no barrier in the chunk loop.
//                                 Two raw images (102), the two query tiles (80) and the decoded operand (40) are above 128 registers:
//                                 two waves per SIMD (__launch_bounds__(256, 2)), where res_align_kernel has four.
//                                 LDS: the 64-byte weights table, written once before the loop.
//   res_wide_gather_pages_kernel  res_gather_pages_kernel on 40 chunks per row: one workgroup per output slot, id -> page -> offsets
//                                 checked the same way, len = min(rows, pad_rows), one lane per (row, 16-byte chunk) -- piece i is
//                                 chunk i % 40 of row i / 40, a division --, four pieces in flight per lane, exact zeros up to
//                                 pad_rows, lengths[slot] = len.  Every byte of the slot is written.
// Every offset, id and code read from the device is checked before it becomes an address.  All row addressing is 64-bit (row * 320
// elements, row * 80 / row * 160 bytes).
#pragma once
#include "maxsim_align.hip"
#include "residual_wide.hip"

namespace msim {

// the undecoded image of lane (l16, l4)'s share of one 16-row chunk
struct ResWideAlignRaw {
    int code;
    bf16x8 cc[kRwKSteps];
    uint32_t fld[kRwKSteps];
};

template <bool F16>
__device__ __forceinline__ bf16x8 rw_nan_chunk() {
    const short nan = (short)(F16 ? 0x7e00 : 0x7fc0);       // what res_wide_decode_kernel writes for a code >= K
    return bf16x8{nan, nan, nan, nan, nan, nan, nan, nan};
}

template <bool F16, int BITS>
__global__ __launch_bounds__(256, 2) void res_wide_align_kernel(const uint16_t *__restrict__ Qt,       // [q_rows, 320] flat query tokens
                                                                const int32_t *__restrict__ q_off,    // [n_q + 1]
                                                                const uint16_t *__restrict__ codes,   // [d_rows]
                                                                const uint8_t *__restrict__ res,      // [d_rows, 40 BITS]
                                                                const uint16_t *__restrict__ C,       // [K, 320]
                                                                int K, const float *__restrict__ weights,
                                                                const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                                const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                                const int64_t *__restrict__ cand,     // [n_q, ld_cand]
                                                                float *__restrict__ best_sim,         // [n_q, m, T]
                                                                int32_t *__restrict__ best_row,       // [n_q, m, T]
                                                                float *__restrict__ sims,             // [n_q, m, T, R] or null
                                                                AlignArgs a) {
    constexpr int DIM = kRwDim, KS = kRwKSteps;
    __shared__ float wtab[16];
    if (threadIdx.x < (1 << BITS)) wtab[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();                                         // the only barrier: before any wave's chunk loop

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l16 = lane & 15, l4 = lane >> 4;
    const long long e = blockIdx.x;
    const int q = (int)(e / a.m), j = (int)(e - (long long)q * a.m);
    const int T = a.T, R = a.R;

    // ---- the entry: query tokens and page rows, every number checked before it is used as an address
    bool bad = false;
    const int qs = q_off[q], qe = q_off[q + 1];
    if (qs < 0 || qe < qs || (long long)qe > a.q_rows || qe - qs > T) bad = true;
    const int len_q = bad ? 0 : qe - qs;
    const int64_t id = cand[(size_t)q * a.ld_cand + j];
    const long long d = (long long)id - a.id_base;
    const bool has_page = id >= 0 && d >= 0 && d < a.n_d;
    int r0 = 0, len_d = 0;
    bool clamp = false;
    if (has_page && !bad) {
        r0 = d_off[d];
        const int r1 = d_off[d + 1];
        if (r0 < 0 || r1 < r0 || (long long)r1 > a.d_rows || r1 - r0 > R) bad = true;
        else {
            len_d = r1 - r0;
            clamp = clamp0 != nullptr && clamp0[d] != 0;
        }
    }
    if (bad) len_d = 0;

    const size_t obase = (size_t)e * T;    // first (token slot) of the entry in best_sim / best_row; x R in sims

    int tok[2];
    bool tile_out[2], tile_live[2];        // the tile has output slots | it meets the page on the matrix pipe (wave-uniform)
    bf16x8 qf[2][KS];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int tok0 = (wave + 4 * k) * kUnitTok;
        tok[k] = tok0 + l16;
        tile_out[k] = tok0 < T;
        tile_live[k] = tok0 < len_q && len_d > 0;
        const bool valid = tile_live[k] && tok[k] < len_q;
        const uint16_t *p = Qt + (size_t)(valid ? qs + tok[k] : 0) * DIM + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) qf[k][ks] = valid ? *reinterpret_cast<const bf16x8 *>(p + ks * 32) : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }

    float bs[2] = {-INFINITY, -INFINITY};
    int br[2] = {-1, -1};
    const int n_chunks = tile_live[0] ? (len_d + kAlignChunk - 1) / kAlignChunk : 0;      // tile 1 live implies tile 0 live
    const bool want_map = sims != nullptr;

    // the raw loads of chunk c: nothing is decoded here, so they can stay in flight under the MFMAs of chunk c - 1
    auto load_chunk = [&](ResWideAlignRaw &raw, int c) {
        int row = c * kAlignChunk + l16;
        row = row < len_d ? row : len_d - 1;             // len_d > 0 here; the duplicate is masked after the MFMA
        const long long grow = (long long)r0 + row;      // r0 + len_d <= d_rows was checked
        raw.code = codes[grow];
        const int crow = raw.code < K ? raw.code : 0;    // a broken code never becomes an address: the row decodes to NaN
        const uint16_t *p = C + (size_t)crow * DIM + l4 * 8;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            raw.cc[ks] = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
            raw.fld[ks] = rw_load_field<BITS>(res, grow, 4 * ks + l4);
        }
    };
    auto chunk = [&](const ResWideAlignRaw &raw, int c) {
        bf16x8 af[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
            af[ks] = raw.code < K ? rw_decode_chunk<F16, BITS>(raw.cc[ks], raw.fld[ks], [&](int b) { return wtab[b]; })
                                  : rw_nan_chunk<F16>();
        const int row0 = c * kAlignChunk + 4 * l4;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (!tile_live[k]) continue;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) acc = mfma16<F16>(af[ks], qf[k][ks], acc);     // one chain, k ascending
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (row0 + r >= len_d) acc[r] = -INFINITY;                                  // no such row
                else if (br[k] < 0 || acc[r] > bs[k]) {
                    bs[k] = acc[r];
                    br[k] = row0 + r;
                }
            }
            if (want_map && tok[k] < T) {
                if (tok[k] >= len_q) acc = f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};    // no such token
                align_store4(sims + (obase + tok[k]) * R, row0, R, a.vec, acc);
            }
        }
    };

    if (n_chunks > 0) {
        ResWideAlignRaw a0, a1;
        load_chunk(a0, 0);
        for (int c = 0; c < n_chunks; c += 2) {
            if (c + 1 < n_chunks) load_chunk(a1, c + 1);
            chunk(a0, c);
            if (c + 1 < n_chunks) {
                if (c + 2 < n_chunks) load_chunk(a0, c + 2);
                chunk(a1, c + 1);
            }
        }
    }

#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!tile_out[k]) continue;
        // the four 16-lane groups hold the same token over different rows: the larger similarity, then the lower row
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
            const float ov = __shfl_xor(bs[k], o);
            const int orow = __shfl_xor(br[k], o);
            if (orow >= 0 && (br[k] < 0 || ov > bs[k] || (ov == bs[k] && orow < br[k]))) {
                bs[k] = ov;
                br[k] = orow;
            }
        }
        if (tok[k] >= T) continue;
        if (l4 == 0) {
            float v = bs[k];
            int arg = br[k];
            if (bad) {
                v = __builtin_nanf("");
                arg = -1;
            } else if (tok[k] >= len_q) {
                v = 0.0f;                                                  // a padding slot adds nothing
                arg = -1;
            } else if (clamp && !(v >= 0.0f)) {                            // the reference's zero padding row wins
                v = 0.0f;
                arg = -1;
            }
            best_sim[obase + tok[k]] = v;
            best_row[obase + tok[k]] = arg;
        }
        if (want_map) {
            // the columns no chunk wrote: everything for a tile that met no page, else the chunks past the page's end
            const float fill = bad ? __builtin_nanf("") : -INFINITY;
            float *srow = sims + (obase + tok[k]) * R;
            for (int c = tile_live[k] ? n_chunks : 0; c * kAlignChunk < R; ++c)
                align_store4(srow, c * kAlignChunk + 4 * l4, R, a.vec, f32x4{fill, fill, fill, fill});
        }
    }
}

// grid: one workgroup per slot; out [n_slots, pad_rows, 320] in the corpus dtype
template <bool F16, int BITS>
__global__ __launch_bounds__(256) void res_wide_gather_pages_kernel(const uint16_t *__restrict__ codes,   // [d_rows]
                                                                    const uint8_t *__restrict__ res,      // [d_rows, 40 BITS]
                                                                    const uint16_t *__restrict__ C,       // [K, 320]
                                                                    int K, const float *__restrict__ weights, long long d_rows,
                                                                    const int32_t *__restrict__ d_off, int n_d, long long id_base,
                                                                    const int64_t *__restrict__ ids, long long pad_rows,
                                                                    uint16_t *__restrict__ out, int32_t *__restrict__ lengths) {
    constexpr int kInFlight = 4;
    __shared__ float wtab[16];
    if (threadIdx.x < (1 << BITS)) wtab[threadIdx.x] = weights[threadIdx.x];
    __syncthreads();

    const long long slot = blockIdx.x;
    const long long id = ids[slot];
    const long long c = id - id_base;
    long long row0 = 0, len = 0;
    if (id >= 0 && c >= 0 && c < n_d) {
        const long long a = d_off[c], b = d_off[c + 1];
        if (a >= 0 && b >= a && b <= d_rows) {           // broken offsets: no page
            row0 = a;
            len = b - a < pad_rows ? b - a : pad_rows;
        }
    }
    if (threadIdx.x == 0) lengths[slot] = (int32_t)len;
    const long long copy = len * kRwChunks, total = pad_rows * kRwChunks;       // 16-byte pieces: piece i is chunk i % 40 of row i / 40
    bf16x8 *dst = reinterpret_cast<bf16x8 *>(out) + slot * total;
    for (long long i0 = threadIdx.x; i0 < total; i0 += kInFlight * 256) {
        int code[kInFlight], ch[kInFlight];
        long long row[kInFlight];
        bf16x8 cc[kInFlight];
        uint32_t fld[kInFlight];
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const long long i = i0 + u * 256;
            const long long rel = i / kRwChunks;         // i < pad_rows * 40 <= (2^31 - 1) * 40
            row[u] = row0 + rel;
            ch[u] = (int)(i - rel * kRwChunks);
            code[u] = i < copy ? (int)codes[row[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const long long i = i0 + u * 256;
            cc[u] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            fld[u] = 0;
            if (i < copy) {
                const int crow = code[u] < K ? code[u] : 0;              // a broken code never becomes an address
                cc[u] = *reinterpret_cast<const bf16x8 *>(C + (size_t)crow * kRwDim + ch[u] * 8);
                fld[u] = rw_load_field<BITS>(res, row[u], ch[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kInFlight; ++u) {
            const long long i = i0 + u * 256;
            if (i >= total) continue;
            bf16x8 v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};                   // the padding: exact zeros
            if (i < copy)
                v = code[u] < K ? rw_decode_chunk<F16, BITS>(cc[u], fld[u], [&](int b) { return wtab[b]; }) : rw_nan_chunk<F16>();
            dst[i] = v;
        }
    }
}

}  // namespace msim
