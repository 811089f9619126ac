// K1s over the 13-bit image of a bf16 corpus (pack13.hip): the stream kernel of maxsim_stream.hip with 6656-byte slabs and a decode
// step between the LDS reads and the MFMAs.  0.8125 x the bytes from HBM; the MFMA operands are the very bits the blob holds, so the
// scores are K1s's bit for bit.  Everything behind the operand fetch is shared with K1s: slab_units, the token table, the epilogue,
// clamp0, kFlagRefBf16 and kFlagPartial.
//
// What differs:
//   * a slab request is 8 LDS-DMA instructions as before -- six of 1 KiB (16 bytes per lane: the low bytes and the nibbles) and two of
//     256 B (one dword per lane: the signs of one row group each).  Every instruction is a full-wave linear copy, none writes past its
//     slot, and the counted vmcnt stays 8 per request; where in the slab body they go out is K1s's ORDER (maxsim_stream.hip);
//   * the image is lane-major (pack13.hip), so neither the DMA source nor the ds_reads are swizzled: per row group two ds_read_b128
//     of low bytes, one of nibbles and one ds_read_b32 of signs, all at lane * 16 (lane * 4);
//   * documents flagged by the encoder (a value the code cannot hold) are skipped; the host scores them from the blob with a
//     list-driven launch of the raw K1s into the same score columns.
#pragma once
#include "maxsim_stream.hip"
#include "pack13_format.hpp"

namespace msim {

// four high bytes at byte positions (H) and four low bytes (L) -> two dwords of two bf16 each
__device__ __forceinline__ void pack13_interleave(uint32_t H, uint32_t L, int &o0, int &o1) {
    o0 = (int)__builtin_amdgcn_perm(H, L, 0x05010400u);     // L0 H0 L1 H1
    o1 = (int)__builtin_amdgcn_perm(H, L, 0x07030602u);     // L2 H2 L3 H3
}

// how the high bytes are put together (DECODE of the kernel).  High byte = 0 0 1 1 nibble under the sign:
//   or3: H = ((nib >> 4h) & 0x0f0f0f0f) | 0x30303030 | ((sign << q) & 0x80808080)      v_and, v_and, v_or3 + the shifts: 6.5 VALU per four values
//   bfi: X = ((sign << q) & 0x80808080) | k30;  H = (nib >> 4h) under 0x0f0f0f0f, X elsewhere    v_and_or, v_bfi + the shifts: 5.5
// (with the two v_perm of the interleave; a shift by 0 is not there).  The same bits either way.  hipcc turns every C++ spelling of
// the second form back into the first as long as it can see through X (the bits under the mask are known), so X and the constant
// k30 = 0x30303030 pass through EMPTY asm statements that only hide their values: no instruction is written by hand, the selector
// emits v_and_or_b32 (one scalar operand per VOP3 on gfx9: k30 lives in a register) and v_bfi_b32 itself, and the hazard recognizer
// sees every instruction next to the MFMAs.  (The two instructions written out as asm text were measured and dropped: hipcc does not
// look into asm text for the MFMA hazards -- profiles/stream13_issue.md.)
constexpr int kDecodeOr3 = 0, kDecodeBfi = 1;
constexpr int stream13_decode() { return kDecodeBfi; }
__device__ __forceinline__ uint32_t pack13_hidden(uint32_t x) {
    asm("" : "+v"(x));
    return x;
}

// the four A fragments of one 16-row group from the lane's raw 52 bytes; k30: pack13_hidden(0x30303030), made once per kernel (bfi)
template <int DECODE>
__device__ __forceinline__ void pack13_decode_group(bf16x8 (&af)[kKSteps16], const i32x4 &lo01, const i32x4 &lo23, const i32x4 &nib,
                                                    uint32_t sign, uint32_t k30) {
#pragma unroll
    for (int ks = 0; ks < kKSteps16; ++ks) {
        i32x4 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = 2 * ks + h;
            const uint32_t L = (uint32_t)(ks < 2 ? lo01[2 * ks + h] : lo23[2 * (ks - 2) + h]);
            uint32_t H;
            if constexpr (DECODE == kDecodeBfi) {
                const uint32_t X = pack13_hidden(((q ? sign << q : sign) & 0x80808080u) | k30);
                H = ((h ? (uint32_t)nib[ks] >> 4 : (uint32_t)nib[ks]) & 0x0f0f0f0fu) | (X & 0xf0f0f0f0u);
            } else {
                H = (((uint32_t)nib[ks] >> (4 * h)) & 0x0f0f0f0fu) | 0x30303030u;
                H |= (sign << q) & 0x80808080u;
            }
            int o0, o1;
            pack13_interleave(H, L, o0, o1);
            o[2 * h] = o0;
            o[2 * h + 1] = o1;
        }
        af[ks] = __builtin_bit_cast(bf16x8, o);
    }
}

// ---- PRIO of the kernel, 2-slot forms only (two workgroups on a CU, so two waves on a SIMD): how the two partners share the SIMD's
// vector issue, which goes to the higher s_setprio and then to the OLDER wave -- left alone, the older workgroup of a CU runs nearly
// unimpeded, finishes early, and the younger one ends the scan alone at one wave per SIMD.  The phase is the parity of the wave's
// slot on its SIMD (HW_ID, read once into an SGPR): on MI355X the traced waves report slots 0 and 1 only, the first workgroup of a
// CU on 0 and the second on 1 (tools/trace_stream.py prints the slots per generation).
//   none   : both at priority 0
//   doc    : priority (documents scored ^ phase) & 1, set at every document's start: the partners take turns
//   slabs  : the same per kPrioSlabCount consumed slabs, so that ragged shards keep the partners out of step (shipped)
//   static : the wave of odd phase at priority 1 for the whole kernel (cdna_hip_programming.md T5, static form): no gain here
// Every form is back at priority 0 before the wave ends.  Measured in profiles/stream13_issue.md; the forms not shipped exist in
// measurement builds only (MSIM_STREAM13_PRIO).
constexpr int kPrioNone = 0, kPrioDoc = 1, kPrioSlabs = 2, kPrioStatic = 3;
constexpr int kPrioSlabCount = 32;
constexpr int stream13_prio(int ring) { return ring == 2 ? kPrioSlabs : kPrioNone; }      // what the shipped library runs
// s_setprio takes an immediate and ignores EXEC: the choice is a scalar branch on a value made wave-uniform by construction
__device__ __forceinline__ void stream13_setprio(unsigned odd) {
    if (__builtin_amdgcn_readfirstlane(odd & 1u)) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
}

template <int NU, int RING, int AUX = 2, int ORDER = stream13_order(RING), int DECODE = stream13_decode(), int PRIO = stream13_prio(RING)>
__global__ __launch_bounds__(256, 2) void maxsim_stream13_kernel(const uint16_t *__restrict__ Qt,      // [T, 128] flat query tokens
                                                                 const int32_t *__restrict__ d_off,    // [n_d + 1]
                                                                 const uint8_t *__restrict__ clamp0,   // [n_d] or null
                                                                 float *__restrict__ scores,           // [n_q, ld]
                                                                 StreamArgs a,
                                                                 const uint8_t *__restrict__ image,    // slab_off[n_d] slabs of kSlab13Bytes
                                                                 const int32_t *__restrict__ slab_off, // [n_d + 1]
                                                                 const uint8_t *__restrict__ flagged) { // [n_d]: 1 = not in this launch
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wave * (RING * kSlab13Bytes);
    char *tokmax = smem + 4 * (RING * kSlab13Bytes) + wave * kStreamTokBytes;
    const int gw = blockIdx.x * 4 + wave;
    const int GW = gridDim.x * 4;
    // a byte of a wave-uniform byte array through the scalar cache (a vector byte load would drain the LDS-DMA ring: see clamp0 in K1s)
    auto byte_at = [&](const uint8_t *p, int i) -> bool {
        const uint64_t addr = reinterpret_cast<uint64_t>(p) + (uint64_t)i;
        return ((scalar_load_u32(addr & ~3ull) >> ((addr & 3) * 8)) & 0xffu) != 0;
    };

    const int n_tok = flat_qoff(a.fq, a.n_q);
    QueryUnit qu[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) load_query_unit(qu[u], Qt, u * kUnitTok, n_tok, lane, true);
    int *const rtab = reinterpret_cast<int *>(tokmax + kStreamMaxUnits * kUnitTok * 16);
    if ((lane >> 3) < a.n_q) {
        rtab[2 * (lane >> 3)] = flat_qoff(a.fq, lane >> 3);
        rtab[2 * (lane >> 3) + 1] = flat_qoff(a.fq, (lane >> 3) + 1);
    }
    wait_vmcnt<0>();
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int ks = 0; ks < kKSteps16; ++ks) asm volatile("" : "+v"(qu[u].f[ks]));

    const int off16 = lane * 16, off4 = lane * 4;
    uint32_t k30 = 0x30303030u;
    if constexpr (DECODE == kDecodeBfi) asm volatile("" : "+v"(k30));      // hidden once, in front of the loops: stays in its register

    // ---- producer cursor (wave-uniform): next slab to request
    int p_idx = gw, p_s = 0, p_n = 0;
    const __amdgpu_buffer_rsrc_t null_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)image, 0, 0, 0x00020000);
    __amdgpu_buffer_rsrc_t p_rsrc = null_rsrc;
    auto p_open = [&]() {  // position on the next document at or after p_idx that has slabs and is not flagged
        while (p_idx < a.n_d) {
            // explicit scalar loads, one wait for the three: left to the compiler these wave-uniform reads become vector loads inside
            // the slab loop, and its vmcnt(0) for them drains the LDS-DMA ring
            const uint64_t fa = reinterpret_cast<uint64_t>(flagged) + (uint64_t)p_idx;
            uint32_t s0u, s1u, fw;
            asm volatile("s_load_dword %0, %3, 0x0\n\ts_load_dword %1, %3, 0x4\n\ts_load_dword %2, %4, 0x0\n\ts_waitcnt lgkmcnt(0)"
                         : "=&s"(s0u), "=&s"(s1u), "=&s"(fw)
                         : "s"(reinterpret_cast<uint64_t>(slab_off + p_idx)), "s"(fa & ~3ull)
                         : "memory");
            const int s0 = (int)s0u, s1 = (int)s1u;
            p_n = s1 - s0;
            if (p_n > 0 && ((fw >> ((fa & 3) * 8)) & 0xffu) == 0) {
                p_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(image + (size_t)s0 * kSlab13Bytes), 0, p_n * kSlab13Bytes, 0x00020000);
                p_s = 0;
                return;
            }
            p_idx += GW;
        }
    };
    p_open();
    int p_slot = 0;
    auto advance = [&](bool live) {
        p_slot = (p_slot + 1 == RING) ? 0 : p_slot + 1;
        if (live) {
            if (++p_s >= p_n) {
                p_idx += GW;
                p_open();
            }
        }
    };
    // piece i of a request: 0..5 = 1 KiB each of [0, 6144), 6..7 = the two 256-byte sign blocks
    auto piece = [&](const __amdgpu_buffer_rsrc_t &rs, char *dst, int soff, int i) {
        if (i < 6)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MSIM_LDS(dst + i * 1024), 16, off16, soff + i * 1024, 0, AUX);
        else
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, MSIM_LDS(dst + kSlab13Sign + (i - 6) * 256), 4, off4,
                                                     soff + kSlab13Sign + (i - 6) * 256, 0, AUX);
    };
    // prologue: RING - 1 requests in flight (real or through the empty descriptor: the count of outstanding loads is a constant)
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
        const bool live = p_idx < a.n_d;
        const __amdgpu_buffer_rsrc_t rs = live ? p_rsrc : null_rsrc;
        char *dst = ring + p_slot * kSlab13Bytes;
        const int soff = live ? p_s * kSlab13Bytes : 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) piece(rs, dst, soff, i);
        advance(live);
    }

    constexpr int kOrd = ORDER;
    constexpr int kEarly = stream_order_early(kOrd);     // pieces of the next request issued in front of the wait
    static_assert(7 * stream_order_stride(kOrd, NU) < 8 * NU, "the eighth pinned piece must stand in front of an MFMA of the body");
    static_assert(PRIO == kPrioNone || RING == 2, "one workgroup per CU is one wave per SIMD: nobody to take turns with");
    MSIM_STREAM_TRACE_BEGIN();
    unsigned prio_turn = 0;            // wave-uniform: the phase, plus the documents (doc) or the blocks of slabs (slabs) behind the wave
    int prio_slabs = 0;
    if constexpr (PRIO != kPrioNone) {
        prio_turn = __builtin_amdgcn_readfirstlane(__builtin_amdgcn_s_getreg(kHwRegHwId)) & 1u;
        if constexpr (PRIO != kPrioDoc) stream13_setprio(prio_turn);
    }
    const bool ref_bf16 = (a.flags & kFlagRefBf16) != 0;
    int c_slot = 0;
    for (int c_idx = gw; c_idx < a.n_d; c_idx += GW) {
        if (byte_at(flagged, c_idx)) continue;
        const int len = d_off[c_idx + 1] - d_off[c_idx];
        float m[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) m[u] = -INFINITY;
        if constexpr (PRIO == kPrioDoc) stream13_setprio(prio_turn++);

        auto slab = [&](auto tail_c, int rows_left) {
            constexpr bool kTail = decltype(tail_c)::value;
            MSIM_STREAM_TRACE_TOP();
            if constexpr (!kEarly) wait_vmcnt<8 * (RING - 2)>();
            const bool nx_live = p_idx < a.n_d;
            char *nx_dst = ring + p_slot * kSlab13Bytes;
            const int nx_soff = nx_live ? p_s * kSlab13Bytes : 0;
            const __amdgpu_buffer_rsrc_t nx_rsrc = nx_live ? p_rsrc : null_rsrc;
            if constexpr (kEarly) {
                // measurement builds: the target slot is the one the previous body consumed -- every ds_read of it was waited on
                // before that body's MFMAs used it -- so the request may go out BEFORE the wait for the current slab.  Loads retire
                // in order: all but the kEarly youngest have landed behind the wait, i.e. the current slab.
#pragma unroll
                for (int i = 0; i < kEarly; ++i) piece(nx_rsrc, nx_dst, nx_soff, i);
                __builtin_amdgcn_sched_barrier(0);
                wait_vmcnt<8 * (RING - 2) + kEarly>();
                __builtin_amdgcn_sched_barrier(0);
            }
            MSIM_STREAM_TRACE_WAITED();

            const char *src = ring + c_slot * kSlab13Bytes;
            c_slot = (c_slot + 1 == RING) ? 0 : c_slot + 1;
            bf16x8 af[2][kKSteps16];
#pragma unroll
            for (int g = 0; g < 2; ++g) {          // one row group at a time: 13 raw registers become 16 decoded ones
                const i32x4 lo01 = *reinterpret_cast<const i32x4 *>(src + (2 * g) * 1024 + off16);
                const i32x4 lo23 = *reinterpret_cast<const i32x4 *>(src + (2 * g + 1) * 1024 + off16);
                const i32x4 nib = *reinterpret_cast<const i32x4 *>(src + kSlab13Nib + g * 1024 + off16);
                const uint32_t sign = *reinterpret_cast<const uint32_t *>(src + kSlab13Sign + g * 256 + off4);
                pack13_decode_group<DECODE>(af[g], lo01, lo23, nib, sign, k30);
                if constexpr (kOrd == kOrderSplit) {
                    if (g == 0) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int i = kEarly; i < 8; ++i) piece(nx_rsrc, nx_dst, nx_soff, i);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            slab_units<false, NU, kTail, true>(m, af, qu, rows_left, lane, [&](int mf) {
                if constexpr (kOrd == kOrderHook) {
                    if (mf % NU == 0) piece(nx_rsrc, nx_dst, nx_soff, mf / NU);
                } else if constexpr (stream_order_stride(kOrd, NU) > 0) {
                    constexpr int kStride = stream_order_stride(kOrd, NU);
                    if (mf % kStride == 0 && mf / kStride < 8) {
                        __builtin_amdgcn_sched_barrier(0);
                        piece(nx_rsrc, nx_dst, nx_soff, mf / kStride);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            });
            advance(nx_live);
            if constexpr (PRIO == kPrioSlabs) {
                if (++prio_slabs == kPrioSlabCount) {
                    prio_slabs = 0;
                    stream13_setprio(++prio_turn);
                }
            }
            MSIM_STREAM_TRACE_END();
        };
        const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
        for (int s = 0; s < n_full; ++s) slab(std::false_type{}, kSlabRows);
        if (rem > 0) slab(std::true_type{}, rem);

        bool clamp = false;
        if (clamp0 != nullptr) clamp = byte_at(clamp0, c_idx);
#pragma unroll
        for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, m[u], lane);
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int rq = ln >> 3, ri = ln & 7;
        if (rq < a.n_q) {
            float tot = reduce_query_tokens<false>(tokmax, rtab[2 * rq], rtab[2 * rq + 1], ri, clamp, ref_bf16);
            if (ref_bf16 && !(a.flags & kFlagPartial)) tot = round_to_input<false>(tot);
            if (ri == 0) scores[(size_t)rq * a.ld + c_idx] = tot;
        }
    }
    if constexpr (PRIO != kPrioNone) __builtin_amdgcn_s_setprio(0);
    MSIM_STREAM_TRACE_WRITE();
}

}  // namespace msim
