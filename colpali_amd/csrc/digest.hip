// msim_digest (include/maxsim.h, "PERSISTENCE"): the two-lane additive digest of a byte range in HBM -- what a saved shard's chunks
// are verified against after they have landed on the device.  One pass over the bytes: 16 B per lane per load on the aligned body,
// per-lane uint64 accumulators, a wave fold, one partial per workgroup, two integer atomics per workgroup.  Integer addition
// commutes, so the result does not depend on the launch plan or on the order the atomics arrive in.
// Defined and launched in abi_persist.hip and in no other translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/maxsim.h"

namespace msim {

constexpr int kDigestBlock = 256;        // lanes per workgroup
constexpr int kDigestMaxBlocks = 2048;   // 8 workgroups per CU; the rest of the range is grid-strided
constexpr int kDigestUnroll = 4;         // independent 16-byte loads per lane in flight

__host__ __device__ inline uint64_t digest_mix(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// word `w` into the two lanes, its position terms k0 = (g + 1) * C0 and k1 = (g + 1) * C1 given
__host__ __device__ inline void digest_add(uint64_t w, uint64_t k0, uint64_t k1, uint64_t &a0, uint64_t &a1) {
    a0 += digest_mix(w + k0);
    a1 += digest_mix((w ^ MSIM_DIGEST_K) + k1);
}

// word `w` at absolute word index `g` into the two lanes
__host__ __device__ inline void digest_word(uint64_t w, uint64_t g, uint64_t &a0, uint64_t &a1) {
    digest_add(w, (g + 1) * MSIM_DIGEST_C0, (g + 1) * MSIM_DIGEST_C1, a0, a1);
}

// words:   the range's first byte (8-byte aligned)
// n_full:  whole 8-byte words in the range; tail: bytes behind them (0 .. 7)
// head:    1 when `words` is not 16-byte aligned and n_full > 0: word 0 is taken on its own and the 16-byte body starts at word 1
// g0:      absolute index of word 0 (pos / 8)
// Every lane reads inside [words, words + n_full * 8 + tail): the body covers words head .. head + 2 * n_pairs - 1, the odd word
// behind it (if any) is word n_full - 1, the tail is read byte by byte.
__global__ __launch_bounds__(kDigestBlock) void digest_kernel(const uint64_t *__restrict__ words, uint64_t n_full, int tail, int head,
                                                              uint64_t g0, unsigned long long *__restrict__ acc) {
    uint64_t a0 = 0, a1 = 0;
    const uint64_t n_pairs = (n_full - (uint64_t)head) >> 1;
    const ulonglong2 *__restrict__ body = reinterpret_cast<const ulonglong2 *>(words + head);
    const uint64_t gb = g0 + (uint64_t)head;                                   // absolute index of the body's first word
    const uint64_t stride = (uint64_t)gridDim.x * kDigestBlock;
    uint64_t i = (uint64_t)blockIdx.x * kDigestBlock + threadIdx.x;
    // the position terms of pair i's first word, carried by addition: one 64-bit multiply per lane here instead of two per word
    uint64_t k0 = (gb + 2 * i + 1) * MSIM_DIGEST_C0, k1 = (gb + 2 * i + 1) * MSIM_DIGEST_C1;
    const uint64_t s0 = 2 * stride * MSIM_DIGEST_C0, s1 = 2 * stride * MSIM_DIGEST_C1;
    for (; i + (kDigestUnroll - 1) * stride < n_pairs; i += kDigestUnroll * stride) {
        ulonglong2 v[kDigestUnroll];
#pragma unroll
        for (int u = 0; u < kDigestUnroll; ++u) v[u] = body[i + u * stride];
#pragma unroll
        for (int u = 0; u < kDigestUnroll; ++u) {
            digest_add(v[u].x, k0, k1, a0, a1);
            digest_add(v[u].y, k0 + MSIM_DIGEST_C0, k1 + MSIM_DIGEST_C1, a0, a1);
            k0 += s0;
            k1 += s1;
        }
    }
    for (; i < n_pairs; i += stride, k0 += s0, k1 += s1) {
        const ulonglong2 v = body[i];
        digest_add(v.x, k0, k1, a0, a1);
        digest_add(v.y, k0 + MSIM_DIGEST_C0, k1 + MSIM_DIGEST_C1, a0, a1);
    }
    if (blockIdx.x == 0) {                                                     // the three pieces the 16-byte body leaves out
        const uint64_t done = (uint64_t)head + 2 * n_pairs;
        if (threadIdx.x == 0 && head) digest_word(words[0], g0, a0, a1);
        if (threadIdx.x == 1 && done < n_full) digest_word(words[done], g0 + done, a0, a1);
        if (threadIdx.x == 2 && tail) {                                        // the last word, zero-padded past the range
            const uint8_t *p = reinterpret_cast<const uint8_t *>(words + n_full);
            uint64_t w = 0;
            for (int b = 0; b < tail; ++b) w |= (uint64_t)p[b] << (8 * b);
            digest_word(w, g0 + n_full, a0, a1);
        }
    }
    // wave fold, then one partial per workgroup
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a0 += __shfl_down((unsigned long long)a0, off, 64);
        a1 += __shfl_down((unsigned long long)a1, off, 64);
    }
    __shared__ unsigned long long part[2][kDigestBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        part[0][wave] = a0;
        part[1][wave] = a1;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kDigestBlock / 64; ++w) s += part[threadIdx.x][w];
        atomicAdd(&acc[threadIdx.x], s);
    }
}

}  // namespace msim
