// The 13-bit image of a bf16 corpus (DESIGN.md sections 2 and 3): format, encoder and a test-only decoder.
//
// Every row the scorers see is L2-normalised, so the exponent field of a bf16 value is at most 127, and for all but exact zeros
// (about one value in 10^7) at least 96.  For such a pattern u bits 14..12 are the constant 011, and the other 13 bits are kept:
//     representable(u)  <=>  96 <= ((u >> 7) & 0xff) <= 127
//     code              =   low byte u & 0xff | nibble (u >> 8) & 0xf | sign u >> 15
//     decode            =   (sign << 15) | 0x3000 | (nibble << 8) | low byte
// Lossless for every representable value: the packed K1s (maxsim_stream13.hip) hands the MFMA the very bits the blob holds.  A
// document with ONE value outside the range (zero, denormal, |x| < 2^-31, |x| >= 2, inf, NaN) is flagged and scored from the blob.
//
// A document of len rows is ceil(len / 32) slabs of 6656 bytes, document c's first slab is slab_off[c].  A slab is laid out in the
// order one wave consumes it as the A operand of v_mfma_f32_16x16x32 (maxsim_common.hpp: slab_rd_offsets16) -- lane L, row group g,
// k-step ks, element j stand for
//     row 16 g + (L & 15) of the slab, column 32 ks + 8 (L >> 4) + j
// and the slab holds
//     [   0, 4096)  low bytes : block 2 g + (ks >> 1) of 1 KiB, lane L's 16 bytes at 16 L, byte 8 (ks & 1) + j
//     [4096, 6144)  nibbles   : block g of 1 KiB, lane L's 16 bytes at 16 L, dword ks, byte j & 3, bits 4 (j >> 2) .. +3
//     [6144, 6656)  signs     : block g of 256 B, lane L's dword at 4 L, bit 8 (j & 3) + 7 - (2 ks + (j >> 2))
// so that the LDS-DMA is a linear copy, every operand read is a linear ds_read, `(N >> 4 h) & 0x0f0f0f0f` are the high bytes' nibbles
// of elements 4 h .. 4 h + 3 at byte positions and `(S << q) & 0x80808080` their signs (q = 2 ks + h): two v_perm_b32 per four values
// interleave them with the low bytes.  Rows past the document's end hold code 0.
#pragma once
#include "maxsim_common.hpp"
#include "pack13_format.hpp"

namespace msim {


__device__ __forceinline__ bool pack13_representable(uint32_t u) {
    const uint32_t e = (u >> 7) & 0xffu;
    return e >= 96u && e <= 127u;
}

// first c with slab_off[c + 1] > s: the document that owns slab s (empty documents own none)
__device__ __forceinline__ int pack13_doc_of_slab(const int32_t *__restrict__ slab_off, int n_d, int s) {
    int lo = 0, hi = n_d - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (slab_off[mid + 1] > s) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// One workgroup of 128 threads per slab: thread (g, L) gathers its 32 values from the blob and writes its 52 bytes of the image.
__global__ __launch_bounds__(128) void pack13_encode_kernel(const uint16_t *__restrict__ D, const int32_t *__restrict__ d_off,
                                                            const int32_t *__restrict__ slab_off, int n_d,
                                                            uint8_t *__restrict__ image, uint8_t *__restrict__ flags) {
    const int s = blockIdx.x;
    const int c = pack13_doc_of_slab(slab_off, n_d, s);
    const int r0 = d_off[c], len = d_off[c + 1] - r0;
    const int g = threadIdx.x >> 6, L = threadIdx.x & 63;
    const int row = (s - slab_off[c]) * kSlabRows + 16 * g + (L & 15);
    uint32_t low[8], nib[4], sign = 0;
    bool bad = false;
#pragma unroll
    for (int ks = 0; ks < kKSteps16; ++ks) {
        i32x4 v = i32x4{0, 0, 0, 0};
        if (row < len) v = *reinterpret_cast<const i32x4 *>(D + (size_t)(r0 + row) * kDim + 32 * ks + 8 * (L >> 4));
        uint32_t lo0 = 0, lo1 = 0, n = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t u = ((uint32_t)v[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            if (row < len && !pack13_representable(u)) bad = true;
            const uint32_t code_lo = row < len ? (u & 0xffu) : 0u, code_n = row < len ? ((u >> 8) & 0xfu) : 0u;
            const uint32_t code_s = row < len ? (u >> 15) : 0u;
            if (j < 4) lo0 |= code_lo << (8 * j);
            else lo1 |= code_lo << (8 * (j - 4));
            n |= code_n << (8 * (j & 3) + 4 * (j >> 2));
            sign |= code_s << (8 * (j & 3) + 7 - (2 * ks + (j >> 2)));
        }
        low[2 * ks] = lo0;
        low[2 * ks + 1] = lo1;
        nib[ks] = n;
    }
    uint8_t *slab = image + (size_t)s * kSlab13Bytes;
#pragma unroll
    for (int h = 0; h < 2; ++h)
        *reinterpret_cast<i32x4 *>(slab + (2 * g + h) * 1024 + 16 * L) =
            i32x4{(int)low[4 * h], (int)low[4 * h + 1], (int)low[4 * h + 2], (int)low[4 * h + 3]};
    *reinterpret_cast<i32x4 *>(slab + kSlab13Nib + g * 1024 + 16 * L) = i32x4{(int)nib[0], (int)nib[1], (int)nib[2], (int)nib[3]};
    *reinterpret_cast<uint32_t *>(slab + kSlab13Sign + g * 256 + 4 * L) = sign;
    if (bad) flags[c] = 1;         // every writer stores the same byte
}

// The flagged ids in ascending order and their number: one workgroup, thread t owns a contiguous run of documents.
__global__ __launch_bounds__(1024) void pack13_list_kernel(const uint8_t *__restrict__ flags, int n_d, int32_t *__restrict__ list,
                                                           int32_t *__restrict__ count) {
    __shared__ int part[1024];
    const int t = threadIdx.x;
    const int per = (n_d + 1023) / 1024;
    const int c0 = t * per < n_d ? t * per : n_d, c1 = c0 + per < n_d ? c0 + per : n_d;
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += flags[c] != 0;
    part[t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {       // inclusive scan
        const int v = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int w = part[t] - mine;
    for (int c = c0; c < c1; ++c)
        if (flags[c] != 0) list[w++] = c;
    if (t == 1023) *count = part[1023];
}

// Test-only inverse of the encoder: rows of the image back into a [rows, 128] bf16 blob (the rows of flagged documents come back
// as whatever their codes decode to).
__global__ __launch_bounds__(128) void pack13_decode_kernel(const uint8_t *__restrict__ image, const int32_t *__restrict__ d_off,
                                                            const int32_t *__restrict__ slab_off, int n_d, uint16_t *__restrict__ out) {
    const int s = blockIdx.x;
    const int c = pack13_doc_of_slab(slab_off, n_d, s);
    const int r0 = d_off[c], len = d_off[c + 1] - r0;
    const int g = threadIdx.x >> 6, L = threadIdx.x & 63;
    const int row = (s - slab_off[c]) * kSlabRows + 16 * g + (L & 15);
    if (row >= len) return;
    const uint8_t *slab = image + (size_t)s * kSlab13Bytes;
    const uint32_t sign = *reinterpret_cast<const uint32_t *>(slab + kSlab13Sign + g * 256 + 4 * L);
    const i32x4 nib = *reinterpret_cast<const i32x4 *>(slab + kSlab13Nib + g * 1024 + 16 * L);
#pragma unroll
    for (int ks = 0; ks < kKSteps16; ++ks) {
        const i32x4 lw = *reinterpret_cast<const i32x4 *>(slab + (2 * g + (ks >> 1)) * 1024 + 16 * L);
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t lo = ((uint32_t)lw[2 * (ks & 1) + (j >> 2)] >> (8 * (j & 3))) & 0xffu;
            const uint32_t n = ((uint32_t)nib[ks] >> (8 * (j & 3) + 4 * (j >> 2))) & 0xfu;
            const uint32_t sg = (sign >> (8 * (j & 3) + 7 - (2 * ks + (j >> 2)))) & 1u;
            const uint32_t u = (sg << 15) | 0x3000u | (n << 8) | lo;
            if (j & 1) o[j >> 1] |= u << 16;
            else o[j >> 1] = u;
        }
        *reinterpret_cast<i32x4 *>(out + (size_t)(r0 + row) * kDim + 32 * ks + 8 * (L >> 4)) = i32x4{(int)o[0], (int)o[1], (int)o[2], (int)o[3]};
    }
}

}  // namespace msim
