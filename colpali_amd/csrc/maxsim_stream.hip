// K1s -- "stream" MaxSim kernel for gfx950 (MI355X), the HBM-bound regime:
// a handful of queries (<= 8 token tiles of 32 tokens) scored against a large
// resident corpus.  Every byte of the corpus is read from HBM exactly once.
//
// Reference arithmetic replaced (no [b,c,n,s] tensor is ever materialised):
//   colpali_engine/utils/processing_utils.py:179
//       einsum("bnd,csd->bcns", Q, D).max(dim=3)[0].sum(dim=2)
//
// Structure (one wave = one independent pipeline, no workgroup barriers at all):
//   * the queries' tokens -- ONE flat token matrix, every query's real tokens back to back
//     (maxsim_common.hpp: the flat layout) -- live in registers for the whole kernel as the MFMA
//     B operand (16 VGPRs per 16-token unit, at most 8 units);
//   * each wave walks its own documents; a document is streamed in 32-patch
//     slabs (8 KiB) into a wave-private LDS ring (RING slabs: 4, or 2 for 3-4 token tiles
//     so that two workgroups share a CU -- see launch_stream in maxsim_abi.hip) by LDS-DMA
//     (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction, fully
//     coalesced, bounds-checked by a per-document buffer descriptor);
//   * the slab image is XOR-swizzled on the SOURCE address so the ds_read_b128
//     operand fetches are bank-conflict free (cdna_hip_programming.md T2 /
//     rule 21: linear destination, swizzled source, same swizzle on the read);
//   * swapped product mfma_f32_16x16x32_bf16(D_slab rows, Q^T) (maxsim_common.hpp: the
//     16x16x32 tiling -- half the accumulator traffic of 32x32x16, which is what counts
//     on a chip that clocks to its power budget): the C layout puts one query token per
//     lane column, so the max over patches is 4 v_max3 per 16-token unit and slab in
//     registers; per document the maxima pass through a wave-private LDS table where 8 lanes
//     per query add that query's tokens (whatever units they sit in) and one lane stores.
#pragma once
#include <type_traits>

#include "maxsim_common.hpp"

namespace msim {

struct StreamArgs {
    long long ld;   // leading dimension of scores
    FlatQ fq;       // where the queries sit in the flat token matrix
    int n_q;        // queries (<= 8: one 8-lane group of every wave per query)
    int n_d;
    unsigned flags;
#ifdef MSIM_TRACE
    unsigned long long *trace;   // tools/trace_stream.py: per wave of the first and the last kStreamTraceWgs workgroups {s_memtime ticks in the wait, in the rest of the body, slabs, s_memrealtime ticks of the wave, HW_ID | XCC_ID << 32 | workgroup << 40, s_memrealtime at its start}; or null
#endif
};

// ---- where a slab body puts the eight LDS-DMA pieces of the next request (ORDER of K1s and K1s13).  Every order drains the ring to
// its depth at the top of the body unless it says otherwise; measured on MI355X in profiles/stream_request_order.md.
//   hook      : the pieces are handed to slab_units' hook, "one per NU MFMAs" -- and hipcc does not keep them there: it gathers all
//               eight behind the body's last ds_read (an LDS-DMA write and an LDS read may alias as far as it knows): in K1s13 at 8
//               units behind MFMA 16, in raw K1s at MFMAs 33..37.  Raw K1s (a tie with the pinned orders at 5-8 units) and every
//               4-slot form (three requests in flight whatever the order) keep it.
//   paced half: one piece in front of every (NU / 2)th MFMA, each pinned between two scheduling barriers, so all eight are out by the
//               middle of the body and each one's issue cost falls behind MFMAs.  K1s13 at 5-8 units: 4.41 -> 4.23 ms at the headline.
//   paced     : the same, one piece per NU MFMAs -- the documented order made real (measurement builds; 0.03 ms behind paced half).
//   early     : all eight in front of the wait, then vmcnt(8 more): the target slot is the one the PREVIOUS body consumed, free since
//               that body's operand reads returned, so a wave has two slabs in flight while it waits (measurement builds: SLOWER
//               than hook by 0.04-0.09 ms in K1s13 and in raw K1s -- the wait at the top is not where these waves lose their time).
//   split     : four pieces in front of the wait, four behind the first row group's operand reads (measurement builds: as hook).
constexpr int kOrderHook = 0, kOrderEarly = 1, kOrderPaced = 2, kOrderSplit = 3, kOrderPacedHalf = 4;
constexpr int stream_order(int) { return kOrderHook; }                                                       // what the shipped library runs: raw K1s,
constexpr int stream13_order(int ring) { return ring == 2 ? kOrderPacedHalf : kOrderHook; }                 // K1s13
constexpr int stream_order_early(int order) { return order == kOrderEarly ? 8 : order == kOrderSplit ? 4 : 0; }   // pieces in front of the wait
constexpr int stream_order_stride(int order, int nu) {                                                       // MFMAs from one pinned piece to the next (0: none pinned)
    return order == kOrderPaced ? nu : order == kOrderPacedHalf ? (nu >= 2 ? nu / 2 : 1) : 0;
}

// s_getreg_b32 operands: where a wave sits (K1s13's priority phase; the trace)
constexpr int kHwRegHwId = 4 | (31 << 11);        // hwreg(HW_REG_HW_ID, 0, 32): wave slot [3:0], SIMD [5:4], pipe [7:6], CU [11:8], SH [12], SE [15:13]
constexpr int kHwRegXccId = 20 | (3 << 11);       // hwreg(HW_REG_XCC_ID, 0, 4): the XCD

// MSIM_TRACE builds only: s_memtime stamps around the wait of every slab body (wave-uniform, SGPRs only), for the waves of the first
// and of the last kStreamTraceWgs workgroups of the grid (the oldest and the youngest): kStreamTraceWords words per wave, the first
// workgroups' waves in rows 0 .. 4 * kStreamTraceWgs - 1, the last ones' behind them
#ifdef MSIM_TRACE
constexpr int kStreamTraceWgs = 64;
constexpr int kStreamTraceWords = 6;
#define MSIM_STREAM_TRACE_BEGIN() \
    const int tr_last0 = (int)gridDim.x - kStreamTraceWgs < kStreamTraceWgs ? kStreamTraceWgs : (int)gridDim.x - kStreamTraceWgs; \
    const int tr_wg = (int)blockIdx.x < kStreamTraceWgs ? (int)blockIdx.x : (int)blockIdx.x - tr_last0 + kStreamTraceWgs; \
    const bool tracing = a.trace != nullptr && ((int)blockIdx.x < kStreamTraceWgs || (int)blockIdx.x >= tr_last0); \
    unsigned long long tr_wait = 0, tr_body = 0, tr_n = 0, tr_t0 = 0, tr_t1 = 0; \
    const unsigned long long tr_r0 = tracing ? __builtin_amdgcn_s_memrealtime() : 0
#define MSIM_STREAM_TRACE_TOP() do { if (tracing) tr_t0 = __builtin_amdgcn_s_memtime(); } while (0)
#define MSIM_STREAM_TRACE_WAITED() do { if (tracing) tr_t1 = __builtin_amdgcn_s_memtime(); } while (0)
#define MSIM_STREAM_TRACE_END() \
    do { if (tracing) { const unsigned long long t2 = __builtin_amdgcn_s_memtime(); tr_wait += tr_t1 - tr_t0; tr_body += t2 - tr_t1; ++tr_n; } } while (0)
#define MSIM_STREAM_TRACE_WRITE() \
    do { if (tracing && lane == 0) { unsigned long long *t = a.trace + (size_t)(tr_wg * 4 + wave) * kStreamTraceWords; t[0] = tr_wait; t[1] = tr_body; t[2] = tr_n; t[3] = __builtin_amdgcn_s_memrealtime() - tr_r0; \
        t[4] = (unsigned long long)__builtin_amdgcn_s_getreg(kHwRegHwId) | ((unsigned long long)__builtin_amdgcn_s_getreg(kHwRegXccId) << 32) | ((unsigned long long)blockIdx.x << 40); t[5] = tr_r0; } } while (0)
#else
#define MSIM_STREAM_TRACE_BEGIN() do {} while (0)
#define MSIM_STREAM_TRACE_TOP() do {} while (0)
#define MSIM_STREAM_TRACE_WAITED() do {} while (0)
#define MSIM_STREAM_TRACE_END() do {} while (0)
#define MSIM_STREAM_TRACE_WRITE() do {} while (0)
#endif

constexpr unsigned kFlagRefBf16 = 1u;
constexpr unsigned kFlagPartial = 2u;     // internal (long queries scored in 128-token pieces): the token sum is a PARTIAL sum, not rounded here

constexpr int kStreamMaxUnits = 8;      // (nine / ten units with eight of them in AGPRs, as in K1b's ten-unit form, were tried in round 4:
                                        // next to the interleaved LDS-DMA issue the slab body does not fit 128 VGPRs and spills into the counted-vmcnt stream)
constexpr int kStreamTokBytes = kStreamMaxUnits * kUnitTok * 16 + 64;   // wave-private: per-token max table (8 units x 16 tokens x 4 lane groups x 4 B) + 8 token ranges

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// NU  : 16-token units of the flat token matrix held by every wave (1..8) = ceil(total tokens / 16)
// RING: slabs in the wave-private LDS ring
// F16 : embeddings are IEEE half instead of bfloat16
// AUX : cache-policy bits of the LDS-DMA loads (0 = default, 2 = nt: streamed once, do not keep in L2 / MALL)
// LIST: the launch scores the documents doc_list[0 .. a.n_d) instead of 0 .. a.n_d-1 (the flagged documents behind the packed form,
//       maxsim_stream13.hip); doc_list is null and unread without it
// ORDER: where the body issues the 8 LDS-DMA pieces of the next slab (above; the shipped library has the hook order only).
// At most 8 units (4 token tiles of 32): launch bounds ask for two waves per SIMD (<= 256 registers), which the 2-slab ring needs to
// put two workgroups on a CU; without the bound hipcc gives every unit an accumulator of its own and lands at 290 registers.
template <int NU, int RING, bool F16, int AUX = 0, bool LIST = false, int ORDER = stream_order(RING)>
__global__ __launch_bounds__(256, 2) void maxsim_stream_kernel(const uint16_t *__restrict__ Qt,      // [T, 128] flat query tokens
                                                            const uint16_t *__restrict__ D,       // [rows, 128] bf16
                                                            const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                            const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                            float *__restrict__ scores,           // [n_q, ld]
                                                            StreamArgs a,
                                                            const int32_t *__restrict__ doc_list = nullptr) {   // [a.n_d] (LIST)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wave * (RING * kSlabBytes);
    char *tokmax = smem + 4 * (RING * kSlabBytes) + wave * kStreamTokBytes;
    const int gw = blockIdx.x * 4 + wave;  // global wave id: this wave owns documents gw, gw+GW, ...
    const int GW = gridDim.x * 4;
    auto doc_id = [&](int i) -> int {      // the document behind position i of this launch (wave-uniform)
        if constexpr (LIST) return doc_list[i];
        else return i;
    };

    // ---- query fragments: B operands, resident for the whole kernel (16 VGPRs per 16-token unit)
    const int n_tok = flat_qoff(a.fq, a.n_q);
    QueryUnit qu[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) load_query_unit(qu[u], Qt, u * kUnitTok, n_tok, lane, true);
    // 8 lanes per query in the reduction; the queries' token ranges wait in LDS behind the table, written here by the lanes that read
    // them back (nothing derived from the lane id needs to stay in registers across the slab loop)
    int *const rtab = reinterpret_cast<int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    if ((lane >> 3) < a.n_q) {
        rtab[2 * (lane >> 3)] = flat_qoff(a.fq, lane >> 3);
        rtab[2 * (lane >> 3) + 1] = flat_qoff(a.fq, (lane >> 3) + 1);
    }

    // the query loads are ordinary VMEM loads: retire them before the LDS-DMA stream starts so that the
    // compiler's own vmcnt waits for them never drain the ring later on
    wait_vmcnt<0>();
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int ks = 0; ks < kKSteps16; ++ks) asm volatile("" : "+v"(qu[u].f[ks]));

    // ---- per-lane address constants
    // LDS-DMA source: wave-instruction i of a slab fills LDS rows 4i..4i+3 linearly; lane (l4 = lane>>4,
    // l16 = lane&15) lands on physical chunk l16 of row 4i+l4, which must hold logical chunk
    // l16 ^ (row & 15) = l16 ^ l4 ^ ((i&3)<<2).
    const int l16 = lane & 15, l4 = lane >> 4;
    int src_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) src_off[j] = l4 * kRowBytes + (((l16 ^ l4) ^ (j << 2)) << 4);
    // operand fetch: fragment (g, ks) = rows 16g + (lane & 15), logical chunk 4 * ks + (lane >> 4)
    int rd_off[2][kKSteps16];
    slab_rd_offsets16(lane, rd_off);

    // ---- producer cursor (wave-uniform): next slab to request
    int p_idx = gw, p_row = 0, p_len = 0;
    __amdgpu_buffer_rsrc_t p_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)D, 0, 0, 0x00020000);
    auto p_open = [&]() {  // position on the next non-empty document at or after p_idx
        while (p_idx < a.n_d) {
            const int p_doc = doc_id(p_idx);
            const int r0 = d_off[p_doc], r1 = d_off[p_doc + 1];
            p_len = r1 - r0;
            if (p_len > 0) {
                p_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(D + (size_t)r0 * kDim), 0,
                                                           p_len * kRowBytes, 0x00020000);
                p_row = 0;
                return;
            }
            p_idx += GW;
        }
    };
    p_open();
    int p_slot = 0;

    // every request is 8 loads, real or through an empty descriptor (out-of-range lanes fetch nothing and count like any
    // other load), so the number of outstanding loads is a constant and the instruction stream has no branches
    const __amdgpu_buffer_rsrc_t null_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)D, 0, 0, 0x00020000);
    auto advance = [&](bool live) {
        p_slot = (p_slot + 1 == RING) ? 0 : p_slot + 1;
        if (live) {
            p_row += kSlabRows;
            if (p_row >= p_len) {
                p_idx += GW;
                p_open();
            }
        }
    };
    // prologue: RING-1 slabs in flight
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
        const bool live = p_idx < a.n_d;
        const __amdgpu_buffer_rsrc_t rs = live ? p_rsrc : null_rsrc;
        char *dst = ring + p_slot * kSlabBytes;
        const int soff = live ? p_row * kRowBytes : 0;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MSIM_LDS(dst + i * 1024), 16, src_off[i & 3], soff + i * 1024, 0, AUX);
        advance(live);
    }

    constexpr int kOrd = ORDER;
    constexpr int kEarly = stream_order_early(kOrd);     // pieces of the next request issued in front of the wait
    static_assert(7 * stream_order_stride(kOrd, NU) < 8 * NU, "the eighth pinned piece must stand in front of an MFMA of the body");
    auto piece = [&](const __amdgpu_buffer_rsrc_t &rs, char *dst, int soff, int i) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MSIM_LDS(dst + i * 1024), 16, src_off[i & 3], soff + i * 1024, 0, AUX);
    };
    const bool ref_bf16 = (a.flags & kFlagRefBf16) != 0;
    int c_slot = 0;
    for (int c_pos = gw; c_pos < a.n_d; c_pos += GW) {
        const int c_idx = doc_id(c_pos);
        const int len = d_off[c_idx + 1] - d_off[c_idx];
        float m[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) m[u] = -INFINITY;

        // one slab: request the next one (ORDER says where its 8 pieces go out), fetch the 8 operand fragments once, then the
        // MFMAs of all units (maxsim_common.hpp: slab_units, folds one group late).  kTail (rows past the document end masked to
        // -inf) is a compile-time variant so that the full-slab body has no branch in it.
        auto slab = [&](auto tail_c, int rows_left) {
            constexpr bool kTail = decltype(tail_c)::value;
            // next slab to request (its slot is the one consumed in the previous iteration: free again)
            // DO NOT REORDER: these four are declared in front of the wait and assigned behind it.  Declared behind it, hipcc swaps two
            // scalar selects in every slab step of every instantiation; check any change here with tools/kernel_diff.py.
            bool nx_live = false;
            char *nx_dst = ring;
            int nx_soff = 0;
            __amdgpu_buffer_rsrc_t nx_rsrc = p_rsrc;
            if constexpr (!kEarly) wait_vmcnt<8 * (RING - 2)>();     // RING - 1 requests are outstanding: all but the oldest may stay in flight
            nx_live = p_idx < a.n_d;
            nx_dst = ring + p_slot * kSlabBytes;
            nx_soff = nx_live ? p_row * kRowBytes : 0;
            nx_rsrc = nx_live ? p_rsrc : null_rsrc;
            if constexpr (kEarly) {
                // every ds_read of the target slot was waited on before the previous body's MFMAs used it: the request goes out in
                // front of the wait for the current slab.  Loads retire in order, so behind the wait all but the kEarly youngest of
                // this request and the RING - 2 requests before it have landed.  The barriers pin the order against the scheduler.
#pragma unroll
                for (int i = 0; i < kEarly; ++i) piece(nx_rsrc, nx_dst, nx_soff, i);
                __builtin_amdgcn_sched_barrier(0);
                wait_vmcnt<8 * (RING - 2) + kEarly>();
                __builtin_amdgcn_sched_barrier(0);
            }

            const char *src = ring + c_slot * kSlabBytes;
            c_slot = (c_slot + 1 == RING) ? 0 : c_slot + 1;
            bf16x8 af[2][kKSteps16];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
#pragma unroll
                for (int ks = 0; ks < kKSteps16; ++ks) af[g][ks] = *reinterpret_cast<const bf16x8 *>(src + rd_off[g][ks]);
                if constexpr (kOrd == kOrderSplit) {
                    if (g == 0) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int i = kEarly; i < 8; ++i) piece(nx_rsrc, nx_dst, nx_soff, i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            slab_units<F16, NU, kTail, true>(m, af, qu, rows_left, lane, [&](int mf) {
                if constexpr (kOrd == kOrderHook) {
                    if (mf % NU == 0) {                 // one DMA piece per NU MFMAs: 8 per slab (a slab is 8 * NU MFMAs)
                        const int i = mf / NU;
                        __builtin_amdgcn_raw_ptr_buffer_load_lds(nx_rsrc, MSIM_LDS(nx_dst + i * 1024), 16, src_off[i & 3],
                                                                 nx_soff + i * 1024, 0, AUX);
                    }
                } else if constexpr (stream_order_stride(kOrd, NU) > 0) {
                    constexpr int kStride = stream_order_stride(kOrd, NU);
                    if (mf % kStride == 0 && mf / kStride < 8) {
                        __builtin_amdgcn_sched_barrier(0);
                        piece(nx_rsrc, nx_dst, nx_soff, mf / kStride);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            });
            advance(nx_live);                                  // the 8 pieces are out: advance the cursor
        };
        const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
        for (int s = 0; s < n_full; ++s) slab(std::false_type{}, kSlabRows);
        if (rem > 0) slab(std::true_type{}, rem);

        // ---- document epilogue: the per-token maxima go to the wave's table in LDS (no barrier: the table is wave-private and a
        // wave's LDS operations complete in order), then 8 lanes per query add their query's tokens and one of them stores.
        // clamp0 is a byte array; fetch the aligned dword around the byte with an explicit scalar load
        // (a vector byte load would make the compiler wait vmcnt(0), i.e. drain the whole LDS-DMA ring)
        bool clamp = false;
        if (clamp0 != nullptr) {
            const uint64_t addr = reinterpret_cast<uint64_t>(clamp0) + (uint64_t)c_idx;
            clamp = ((scalar_load_u32(addr & ~3ull) >> ((addr & 3) * 8)) & 0xffu) != 0;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, m[u], lane);
        int ln = lane;
        asm volatile("" : "+v"(ln));            // opaque: no row pointer or table address is hoisted out of the document loop
        const int rq = ln >> 3, ri = ln & 7;
        if (rq < a.n_q) {
            float tot = reduce_query_tokens<F16>(tokmax, rtab[2 * rq], rtab[2 * rq + 1], ri, clamp, ref_bf16);
            if (ref_bf16 && !(a.flags & kFlagPartial)) tot = round_to_input<F16>(tot);
            if (ri == 0) scores[(size_t)rq * a.ld + c_idx] = tot;
        }
    }
}

}  // namespace msim
