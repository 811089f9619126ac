// K1cP -- candidate reranking for embeddings WIDER than 128 (ColQwen3: dim = 320, colpali_engine/models/qwen3/colqwen3/
// modeling_colqwen3.py:48), 16-bit: K1c (maxsim_candidates.hip) with the document stream of the panel kernels (maxsim_panels.hip).
//
// Reference arithmetic (the same per entry as K1sP / K1bPF, no [b,c,n,s] tensor):
//   colpali_engine/utils/processing_utils.py:179
//       einsum("bnd,csd->bcns", Q, D).max(dim=3)[0].sum(dim=2)
// restricted to the documents each query lists.
//
// The inversion of the candidate matrix into work items does not depend on the row width: cand_zero / cand_count / the three scans /
// cand_place / cand_poison, CandItem and the status word are K1c's, unchanged, and so is the cap of eight 16-token units per item.
// Only the scorer of one item is new.  A row of dim * 2 bytes arrives as PANELS column panels of 256 bytes: panel p of a 32-row slab
// is one 8 KiB panel-slab with exactly the LDS image of a width-128 slab (panel_src_off: the XOR swizzle on the source address; in
// the last panel the lanes whose 16-byte chunk lies beyond the row re-read chunk 0 of their row, so no byte outside a row is
// fetched).  The panel-slabs of the item's document go through a wave-private ring of 4 by LDS-DMA through the per-document buffer
// descriptor; the 8 pieces of the panel-slab RING - 1 ahead are issued between the MFMAs of the current one, real or through an empty
// descriptor, so the number of loads in flight is a constant and the waits are counted.
//
// Bits: the MFMA chain of a (slab, unit) runs across the panels in the order p = 0 .. PANELS-1, ks = 0 .. before the tail mask and
// the max fold -- the order of maxsim_batch_panels_flat_kernel (K1bPF) -- and the token sum is reduce_query_tokens, whose order
// depends on the query's length alone.  So every score carries the bits msim_fwd_ragged gives the same query and document when K1bPF
// computes it, whatever the list, the grouping into items or the batch.
//
// Registers: a 16-token unit at width 320 is 10 k-steps of 32 = 40 operand registers, eight units 320.  As K1sP (four 32-token tiles
// of 80), a wave runs alone on its SIMD with the unified 512-register file: __launch_bounds__(256), 4 waves x 32 KiB of ring + the
// token tables = one workgroup per CU.
#pragma once
#include <type_traits>

#include "maxsim_candidates.hip"
#include "maxsim_common.hpp"
#include "maxsim_panels.hip"

namespace msim {

constexpr int kCandPanelRing = 4;                 // panel-slabs in a wave's ring: 32 KiB, one 4-wave workgroup per CU
constexpr int kCandPanelLdsBytes = 4 * (kCandPanelRing * kSlabBytes + kStreamTokBytes);

template <int NU, int PANELS, int KS_LAST, bool F16, int AUX>
__device__ __forceinline__ void cand_item_panels(const uint16_t *__restrict__ Qt, const int32_t *__restrict__ q_off,
                                                 const uint16_t *__restrict__ D, const int32_t *__restrict__ d_off,
                                                 const uint8_t *__restrict__ clamp0, const int2 *__restrict__ entries, const CandItem &h,
                                                 int n_q, int m, float *__restrict__ scores, long long ld, bool ref_bf16, bool &bad,
                                                 char *ring, char *tokmax, const int (&src_full)[4], const int (&src_last)[4],
                                                 const int (&rd_off)[2][kKSteps16], int lane) {
    constexpr int RING = kCandPanelRing;
    constexpr int KT32 = ((PANELS - 1) * 8 + KS_LAST) / 2;      // k-steps of 32 elements
    constexpr int DIM = KT32 * 32;
    constexpr int ROW_BYTES = DIM * 2;
    static_assert(KS_LAST % 2 == 0 && KS_LAST >= 2 && KS_LAST <= 8, "the last panel holds whole k-steps of 32");
    const int r0 = d_off[h.doc];
    const int len = d_off[h.doc + 1] - r0;
    const int n_slabs = (len + kSlabRows - 1) / kSlabRows;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(D + (size_t)r0 * DIM), 0, len * ROW_BYTES, 0x00020000);
    const __amdgpu_buffer_rsrc_t null_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)D, 0, 0, 0x00020000);

    // piece i (rows 4i .. 4i+3) of panel `pan` of slab `slab`; every request is 8 loads, real or through an empty descriptor.  A row at
    // or past the document's end lies outside the descriptor and reads as zeros; its products are masked to -inf behind the MFMAs
    auto request_piece = [&](int slab, int pan, int slot, int i) {
        const bool live = slab < n_slabs;
        const int voff = pan == PANELS - 1 ? src_last[i & 3] : src_full[i & 3];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(live ? rsrc : null_rsrc, MSIM_LDS(ring + slot * kSlabBytes + i * 1024), 16, voff,
                                                 live ? slab * (kSlabRows * ROW_BYTES) + pan * kPanelBytes + i * (4 * ROW_BYTES) : 0, 0, AUX);
    };
    int p_slot = 0;
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) request_piece(k / PANELS, k % PANELS, p_slot, i);
        p_slot = p_slot + 1 == RING ? 0 : p_slot + 1;
    }

    // the item's query units, behind the first panel-slabs' DMA: unit u = unit (u mod nu) of entry u / nu
    bf16x8 qf[NU][KT32];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int ei = u / h.nu;
        int q = __builtin_amdgcn_readfirstlane(entries[h.e0 + ei].x);
        if (q < 0 || q >= n_q) {                         // never trust a device-built index with an address: reported, the call's
            bad = true;                                  // scores become NaN
            q = 0;
        }
        const int qs = q_off[q], qe = q_off[q + 1];
        const int row = qs + (u - ei * h.nu) * kUnitTok + (lane & 15);
        const bool valid = row >= 0 && row < qe;
        const uint16_t *p = Qt + (size_t)(valid ? row : 0) * DIM + (lane >> 4) * 8;
#pragma unroll
        for (int ks = 0; ks < KT32; ++ks) {
            const bf16x8 v = *reinterpret_cast<const bf16x8 *>(p + ks * 32);
            qf[u][ks] = valid ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    wait_vmcnt<0>();
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int ks = 0; ks < KT32; ++ks) asm volatile("" : "+v"(qf[u][ks]));

    float mx[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) mx[u] = -INFINITY;
    int c_slot = 0;
    auto slab = [&](auto tail_c, int s, int rows_left) {
        constexpr bool kTail = decltype(tail_c)::value;
        UnitAcc acc[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int g = 0; g < 2; ++g) acc[u].a[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < PANELS; ++p) {
            const int nks = p == PANELS - 1 ? KS_LAST / 2 : kKSteps16;     // k-steps of 32 in this panel
            const int tot = NU * 2 * nks;                                  // its MFMAs: the 8 DMA pieces are spread over them
            wait_vmcnt<8 * (RING - 2)>();     // RING - 1 requests are outstanding: all but the oldest may stay in flight
            // the panel-slab RING - 1 ahead goes into the slot that was read in the previous step
            const int nx_slab = s + (p + RING - 1) / PANELS, nx_pan = (p + RING - 1) % PANELS, nx_slot = p_slot;
            const char *src = ring + c_slot * kSlabBytes;
            c_slot = c_slot + 1 == RING ? 0 : c_slot + 1;
            bf16x8 af[2][kKSteps16];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int ks = 0; ks < kKSteps16; ++ks)
                    if (ks < nks) af[g][ks] = *reinterpret_cast<const bf16x8 *>(src + rd_off[g][ks]);
#pragma unroll
            for (int ks = 0; ks < kKSteps16; ++ks)
                if (ks < nks) {
#pragma unroll
                    for (int u = 0; u < NU; ++u)
#pragma unroll
                        for (int g = 0; g < 2; ++g) {
                            const int mf = (ks * NU + u) * 2 + g;
#pragma unroll
                            for (int i = 0; i < 8; ++i)
                                if (i * tot / 8 == mf) request_piece(nx_slab, nx_pan, nx_slot, i);
                            acc[u].a[g] = mfma16<F16>(af[g][ks], qf[u][p * kKSteps16 + ks], acc[u].a[g]);
                        }
                }
            p_slot = p_slot + 1 == RING ? 0 : p_slot + 1;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            if constexpr (kTail) unit_mask_tail(acc[u], rows_left, lane);
            unit_fold(mx[u], acc[u]);
        }
    };
    const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
    for (int s = 0; s < n_full; ++s) slab(std::false_type{}, s, kSlabRows);
    if (rem > 0) slab(std::true_type{}, n_full, rem);
    wait_vmcnt<0>();                      // the empty requests behind the document: the ring is free for the next item

    bool clamp = false;
    if (clamp0 != nullptr) {
        const uint64_t addr = reinterpret_cast<uint64_t>(clamp0) + (uint64_t)h.doc;
        clamp = ((scalar_load_u32(addr & ~3ull) >> ((addr & 3) * 8)) & 0xffu) != 0;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], lane);
    const int rq = lane >> 3, ri = lane & 7;
    const int2 ent = rq < h.n ? entries[h.e0 + rq] : make_int2(0, 0);
    if (rq < h.n && (ent.x < 0 || ent.x >= n_q || ent.y < 0 || ent.y >= m)) bad = true;
    else if (rq < h.n) {
        const int s = rq * h.nu * kUnitTok;
        float tot = reduce_query_tokens<F16>(tokmax, s, s + (q_off[ent.x + 1] - q_off[ent.x]), ri, clamp, ref_bf16);
        if (ref_bf16) tot = round_to_input<F16>(tot);
        if (ri == 0) scores[(size_t)ent.x * ld + ent.y] = tot;
    }
}

// one wave per SIMD (no second launch bound): eight resident units are 320 operand registers of the unified 512
template <int PANELS, int KS_LAST, bool F16, int AUX>
__global__ __launch_bounds__(256) void maxsim_candidates_panels_kernel(const uint16_t *__restrict__ Qt,      // [T, dim] flat query tokens
                                                                       const int32_t *__restrict__ q_off,   // [n_q + 1]
                                                                       const uint16_t *__restrict__ D,      // [rows, dim]
                                                                       const int32_t *__restrict__ d_off,   // [n_d + 1]
                                                                       const uint8_t *__restrict__ clamp0,  // [n_d] or null
                                                                       const int2 *__restrict__ entries,    // (query, column) by item
                                                                       const CandItem *__restrict__ items,
                                                                       const int32_t *__restrict__ n_items_p, int n_entries, int n_q,
                                                                       int m, int n_d, float *__restrict__ scores, long long ld,
                                                                       unsigned flags, int32_t *__restrict__ status) {
    constexpr int ROW_BYTES = ((PANELS - 1) * 8 + KS_LAST) * 32;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wave * (kCandPanelRing * kSlabBytes);
    char *tokmax = smem + 4 * (kCandPanelRing * kSlabBytes) + wave * kStreamTokBytes;
    const int gw = blockIdx.x * 4 + wave;
    const int GW = gridDim.x * 4;
    const bool ref_bf16 = (flags & kFlagRefBf16) != 0;

    int src_full[4], src_last[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        src_full[j] = panel_src_off(lane, j, ROW_BYTES, 16);
        src_last[j] = panel_src_off(lane, j, ROW_BYTES, 2 * KS_LAST);
    }
    int rd_off[2][kKSteps16];
    slab_rd_offsets16(lane, rd_off);

    // the item list is data of the preceding kernels: every header is checked before it becomes an address (at most one item per entry)
    int n_items = __builtin_amdgcn_readfirstlane(*n_items_p);
    bool bad = n_items < 0 || n_items > n_entries;
    n_items = bad ? 0 : n_items;
    for (int it = gw; it < n_items; it += GW) {
        const CandItem *hp = items + it;
        CandItem h;
        h.doc = __builtin_amdgcn_readfirstlane(hp->doc);
        h.e0 = __builtin_amdgcn_readfirstlane(hp->e0);
        h.n = __builtin_amdgcn_readfirstlane(hp->n);
        h.nu = __builtin_amdgcn_readfirstlane(hp->nu);
        if (h.doc < 0 || h.doc >= n_d || h.nu < 1 || h.nu > kStreamMaxUnits || h.n < 1 || h.n * h.nu > kStreamMaxUnits || h.e0 < 0 ||
            h.e0 > n_entries - h.n) {
            bad = true;
            continue;
        }
        switch (h.n * h.nu) {
#define MSIM_CAND_CASE(U) \
            case U: cand_item_panels<U, PANELS, KS_LAST, F16, AUX>(Qt, q_off, D, d_off, clamp0, entries, h, n_q, m, scores, ld, ref_bf16, bad, ring, tokmax, src_full, src_last, rd_off, lane); break;
            MSIM_CAND_CASE(1)
            MSIM_CAND_CASE(2)
            MSIM_CAND_CASE(3)
            MSIM_CAND_CASE(4)
            MSIM_CAND_CASE(5)
            MSIM_CAND_CASE(6)
            MSIM_CAND_CASE(7)
            MSIM_CAND_CASE(8)
#undef MSIM_CAND_CASE
            default: break;
        }
    }
    if (bad && lane == 0) atomicOr(status, kCandBadItem);
}

}  // namespace msim
