// msim_query_compact's kernel.  A file of its own because it is not a template: a non-template kernel must be defined in exactly
// one translation unit of the library, and maxsim_abi.hip -- where msim_query_compact launches it -- is the only one that includes this.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

// Zero rows of a [n_q, Lq, dim] query box add exactly 0 to every score (the model multiplies padded positions by the attention mask:
// modeling_colpali.py:72, modeling_colqwen2.py:69): the flat layout drops them.  One workgroup per query.  counts != null: the number
// of rows that are not all-zero goes to counts[q].  out != null: those rows are copied, in order, to rows q_off[q] .. of `out`.
constexpr int kCompactMaxRows = 4096;
__global__ __launch_bounds__(256) void query_compact_kernel(const char *__restrict__ box, int Lq, int row_bytes,
                                                            const int32_t *__restrict__ q_off, int32_t *__restrict__ counts,
                                                            char *__restrict__ out) {
    __shared__ int pos[kCompactMaxRows + 1];
    const int q = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const char *src = box + (size_t)q * Lq * row_bytes;
    const int pieces = row_bytes >> 4;
    for (int r = wave; r < Lq; r += 4) {
        uint32_t acc = 0;
        for (int p = lane; p < pieces; p += 64) {
            const i32x4 v = *reinterpret_cast<const i32x4 *>(src + (size_t)r * row_bytes + (p << 4));
            acc |= (uint32_t)(v[0] | v[1] | v[2] | v[3]);
        }
        const bool nz = __ballot(acc != 0) != 0;
        if (lane == 0) pos[r + 1] = nz ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pos[0] = 0;
        for (int r = 0; r < Lq; ++r) pos[r + 1] += pos[r];
        if (counts) counts[q] = pos[Lq];
    }
    __syncthreads();
    if (out == nullptr) return;
    char *dst = out + (size_t)q_off[q] * row_bytes;
    for (int r = wave; r < Lq; r += 4) {
        if (pos[r + 1] == pos[r]) continue;
        for (int p = lane; p < pieces; p += 64)
            *reinterpret_cast<i32x4 *>(dst + (size_t)pos[r] * row_bytes + (p << 4)) =
                *reinterpret_cast<const i32x4 *>(src + (size_t)r * row_bytes + (p << 4));
    }
}

}  // namespace msim
