// Shape predicates, argument checks and the call struct of the row-layout kernels that more than one family of entry points uses
// (maxsim_abi.hip, abi_train.hip, abi_head_pool.hip).  Host-only, hidden visibility like abi_common.hpp.
#pragma once
#include "abi_common.hpp"
#include "maxsim_common.hpp"

#pragma GCC visibility push(hidden)
namespace msim_abi {

// tuned = the dim=128 16-bit kernels (K1s / K1b / pair-list); everything else goes to the generic kernels (K1g)
inline bool is_tuned(int dtype, int dim, int Lq) {
    return (dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) && dim == msim::kDim &&
           (Lq + msim::kTokTile - 1) / msim::kTokTile <= 4;
}

// queries longer than 128 tokens in the tuned dtype / width: scored as 128-token segments on K1b (MaxSim is a sum over query
// tokens) when the caller passes scratch for the partial sums; otherwise (and for every other shape) the generic kernels take them
constexpr int kLongSegRows = 4 * msim::kTokTile;
inline bool is_long_tuned(int dtype, int dim, int Lq) {
    return (dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) && dim == msim::kDim && Lq > kLongSegRows;
}
inline int long_segments(int Lq) { return (Lq + kLongSegRows - 1) / kLongSegRows; }

inline int check_common(const void *Q, const void *D, const int32_t *d_off, int dtype, int dim, int Lq) {
    if (!Q || !D || !d_off) return fail(MSIM_EINVAL, "null pointer argument");
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16 && dtype != MSIM_DTYPE_F32)
        return fail(MSIM_EUNSUPPORTED, "dtype code %d: the gfx950 kernels take bfloat16 (0), float16 (1) or float32 (2) embeddings",
                    dtype);
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D)) & 15)
        return fail(MSIM_EINVAL, "Q and D must be 16-byte aligned");
    if (dim <= 0) return fail(MSIM_EINVAL, "dim=%d", dim);
    if (!is_tuned(dtype, dim, Lq)) {
        const long long row_bytes = (long long)dim * elem_bytes(dtype);
        if (row_bytes % 32 != 0)
            return fail(MSIM_EUNSUPPORTED, "dim=%d: an embedding row must be a multiple of 32 bytes (pad the width with zero columns)", dim);
        if (row_bytes > msim::kGenericMaxRowBytes)
            return fail(MSIM_EUNSUPPORTED, "dim=%d: embedding rows above %d bytes are not supported", dim, msim::kGenericMaxRowBytes);
    }
    return MSIM_OK;
}

// the row-layout contract of the generic kernels (K1g), the smooth-max kernels, the plain similarity matrix and the token pooling
inline int check_smooth(const void *Q, const void *D, const int32_t *d_off, int dtype, int dim, int Lq, float tau) {
    if (!Q || !D || !d_off) return fail(MSIM_EINVAL, "null pointer argument");
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16 && dtype != MSIM_DTYPE_F32)
        return fail(MSIM_EUNSUPPORTED, "dtype code %d", dtype);
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D)) & 15)
        return fail(MSIM_EINVAL, "Q and D must be 16-byte aligned");
    if (!(tau > 0.0f)) return fail(MSIM_EINVAL, "tau must be positive");
    if (dim <= 0 || Lq <= 0) return fail(MSIM_EINVAL, "bad size (dim=%d Lq=%d)", dim, Lq);
    const long long row_bytes = (long long)dim * elem_bytes(dtype);
    if (row_bytes % 32 != 0)
        return fail(MSIM_EUNSUPPORTED, "dim=%d: an embedding row must be a multiple of 32 bytes (pad the width with zero columns)", dim);
    if (row_bytes > msim::kGenericMaxRowBytes)
        return fail(MSIM_EUNSUPPORTED, "dim=%d: embedding rows above %d bytes are not supported", dim, msim::kGenericMaxRowBytes);
    return MSIM_OK;
}

// one call of the generic forward kernels (maxsim_abi.hip) or of the smooth-max forward, which has the same launch shape (abi_train.hip)
struct GenericCall {
    const char *Q, *D;
    const int32_t *d_off;
    const uint8_t *clamp0;
    float *scores;
    long long ld;
    int n_q, Lq, n_d, row_bytes;
    unsigned flags;
    const DeviceInfo *di;
    hipStream_t st;
};

}  // namespace msim_abi
#pragma GCC visibility pop
