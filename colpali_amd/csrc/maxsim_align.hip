// K1a -- token-to-patch alignment of listed (query, page) entries over the resident corpus, for gfx950 (MI355X).
//
// Reference arithmetic: the similarity map of one (query, page) pair,
//   colpali_engine/interpretability/similarity_map_utils.py:9-55      einsum("bnk,bijk->bnij", query, image patches)
// and the arg-max behind MaxSim (colpali_engine/utils/processing_utils.py:179: einsum("bnd,csd->bcns").max(dim=3)), here for the
// entries of a candidate matrix cand [n_q, m] of GLOBAL ids, resolved exactly as msim_fwd_candidates resolves them, against the
// packed corpus: no host read of the list, no slice of the blob per hit, one launch for every hit of every query.
//
// One 4-wave workgroup per entry (q, j).  Wave w owns the 16-token tiles w and w + 4 of the query (T <= 128 tokens: 8 tiles), held in
// registers as the B operand of v_mfma_f32_16x16x32; every wave streams the page in 16-row chunks (the A operand, one chunk loaded
// ahead of the one being multiplied; a row past the page's end is read from the page's last row, never from beyond it).  The
// accumulator of one (chunk, tile) is ONE chain of DIM / 32 MFMAs from zero, k ascending: the bits of <q_i, d_j> depend on the token
// row and the page row alone -- not on the entry's position, the batch, m, or whether the map is written.  Rows past the page's end
// are masked to -inf AFTER the MFMA and before they meet a max (a zero row must never win against an all-negative page).  Each lane
// keeps a running (max, first row) over its rows; the four 16-lane groups are folded at the end, the lowest row winning a tie.
// In the 16x16 accumulator a lane holds four consecutive rows of one token: a map is written as one 16-byte store per lane and chunk.
//
// Every offset read from the device is checked against the row / token counts and the caller's bounds before it becomes an address;
// an entry whose offsets break an invariant, or whose page is longer than max_rows, is written as NaN / -1 and reads nothing.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kAlignMaxTokens = 128;       // tokens per query: 8 tiles of 16, two per wave
constexpr int kAlignChunk = 16;            // page rows per chunk = MFMA M

struct AlignArgs {
    long long ld_cand, id_base, q_rows, d_rows;
    int n_q, m, n_d, T, R;                 // T = max_q_tokens, R = max_rows
    int vec;                               // sims may be written with 16-byte stores (16-byte aligned base, R % 4 == 0)
};

// four map values of token `tok`, rows row0 .. row0 + 3 (row0 a multiple of 4); nothing at or beyond column R is touched
__device__ __forceinline__ void align_store4(float *__restrict__ srow, int row0, int R, int vec, const f32x4 &v) {
    if (vec) {
        if (row0 < R) *reinterpret_cast<f32x4 *>(srow + row0) = v;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (row0 + r < R) srow[row0 + r] = v[r];
    }
}

template <int DIM, bool F16>
__global__ __launch_bounds__(256) void maxsim_align_kernel(const uint16_t *__restrict__ Qt,       // [q_rows, DIM] flat query tokens
                                                           const int32_t *__restrict__ q_off,    // [n_q + 1]
                                                           const uint16_t *__restrict__ D,       // [d_rows, DIM]
                                                           const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                           const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                           const int64_t *__restrict__ cand,     // [n_q, ld_cand]
                                                           float *__restrict__ best_sim,         // [n_q, m, T]
                                                           int32_t *__restrict__ best_row,       // [n_q, m, T]
                                                           float *__restrict__ sims,             // [n_q, m, T, R] or null
                                                           AlignArgs a) {
    constexpr int KS = DIM / 32;
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
    const uint16_t *Dp = D + (size_t)r0 * DIM + l4 * 8;

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

    auto load_chunk = [&](bf16x8 (&af)[KS], int c) {
        int row = c * kAlignChunk + l16;
        row = row < len_d ? row : len_d - 1;             // len_d > 0 here; the duplicate is masked after the MFMA
        const uint16_t *p = Dp + (size_t)row * DIM;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
    };
    auto chunk = [&](const bf16x8 (&af)[KS], int c) {
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
        bf16x8 a0[KS], a1[KS];
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

}  // namespace msim
