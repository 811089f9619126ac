// The total order of every selection in this project, (score descending, id ascending), as the selection kernels compute it:
// a 32-bit order-preserving image of the score and an unsigned compare of the ids.  Shared by topk_select.hip (k <= 1024),
// topk_deep.hip (k <= 8192) and group.hip; stated once, here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace msim {

// order-preserving map float -> uint32 (ascending); -0.0 is folded onto +0.0 so that equal
// floats always tie and the id decides
__device__ __forceinline__ uint32_t score_key(float s) {
    if (s == 0.0f) s = 0.0f;
    uint32_t u = __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_score(uint32_t k) {
    uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(u);
}

// a ranks before b: higher score first, then lower id (ids compared unsigned so the -1 padding id ranks last)
__device__ __forceinline__ bool ranks_before(uint32_t ka, uint64_t ia, uint32_t kb, uint64_t ib) {
    return (ka > kb) || (ka == kb && ia < ib);
}

}  // namespace msim
