// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the fixed-dimensional-encoding encoders at width 320 (msim_fdew_*).
// Host-side dispatch only: argument validation and launch on the caller's stream.  Nothing here allocates, frees or synchronises,
// so every entry point is hipGraph-capturable.  The kernel of fde_wide.hip is defined and launched in this translation unit and in
// no other: a unit of its own, so that no kernel of another unit is compiled beside it.  The encodings are
// scored by msim_fde_scores (abi_index.hip), which depends on F alone.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fde_wide.hip"

using namespace msim_abi;

namespace {

// the encoding's configuration: what the kernel implements, or MSIM_EUNSUPPORTED / MSIM_EINVAL
int fdew_check_config(const char *who, int dtype, int dim, int reps, int ksim, int dproj, long long *F_out) {
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != msim::kFdwDim)
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 embeddings of width %d (dtype code %d, dim %d)", who, msim::kFdwDim,
                    dtype, dim);
    if (reps < 1) return fail(MSIM_EINVAL, "%s: reps=%d < 1", who, reps);
    if (ksim < 1 || ksim > msim::kFdwMaxKsim) return fail(MSIM_EUNSUPPORTED, "%s: k_sim=%d outside 1..%d", who, ksim, msim::kFdwMaxKsim);
    if (!(dproj == 8 || dproj == 16 || dproj == 32 || dproj == 64))
        return fail(MSIM_EUNSUPPORTED, "%s: d_proj=%d is not 8, 16, 32 or 64", who, dproj);
    const long long F = (long long)reps * (1LL << ksim) * dproj;
    if (F % 256 != 0 || F > 65536)
        return fail(MSIM_EUNSUPPORTED, "%s: F = reps x 2^k_sim x d_proj = %lld must be a multiple of 256 and at most 65536", who, F);
    *F_out = F;
    return MSIM_OK;
}

int fdew_encode(const char *who, int dtype, const void *X, const int32_t *off, int n, int64_t n_rows, int dim, const float *G,
                const float *S, int reps, int ksim, int dproj, int is_doc, int fill_empty, void *out, uint8_t *codes, void *stream) {
    if (n < 0 || n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (n=%d rows=%lld)", who, n, (long long)n_rows);
    long long F = 0;
    if (int rc = fdew_check_config(who, dtype, dim, reps, ksim, dproj, &F)) return rc;
    if (n == 0) return MSIM_OK;
    if ((!X && n_rows > 0) || !off || !G || !S || !out) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(X, 16) || misaligned(out, 2))
        return fail(MSIM_EINVAL, "%s: the rows must be 16-byte aligned and the output 2-byte aligned", who);
    if (fill_empty != 0 && fill_empty != 1) return fail(MSIM_EINVAL, "%s: fill_empty=%d is not 0 or 1", who, fill_empty);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = f16 ? msim::fde_wide_encode_kernel<true> : msim::fde_wide_encode_kernel<false>;
    static std::atomic<int> configured_bf16[kMaxDevices], configured_f16[kMaxDevices];
    constexpr int kMaxLds = msim::fde_wide_encode_lds_bytes(msim::kFdwMaxKsim, 64);
    static_assert(kMaxLds <= 160 * 1024, "fde_wide_encode_kernel: the largest configuration must fit the CU's LDS");
    if (int rc = allow_lds(kern, kMaxLds, f16 ? configured_f16 : configured_bf16)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(msim::kFdwThreads), msim::fde_wide_encode_lds_bytes(ksim, dproj), st,
                       static_cast<const uint16_t *>(X), off, n, (long long)n_rows, G, S, reps, ksim, dproj, is_doc, fill_empty,
                       static_cast<uint16_t *>(out), codes);
    return launch_failed("fde_wide_encode_kernel");
}

}  // namespace

extern "C" {

int msim_fdew_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, const float *G, const float *S,
                          int reps, int ksim, int dproj, int fill_empty, void *out, uint8_t *codes, void *stream) {
    return fdew_encode("msim_fdew_encode_docs", dtype, D, d_off, n_d, n_rows, dim, G, S, reps, ksim, dproj, 1, fill_empty, out, codes,
                       stream);
}

int msim_fdew_encode_queries(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t n_rows, int dim, const float *G,
                             const float *S, int reps, int ksim, int dproj, void *out, uint8_t *codes, void *stream) {
    return fdew_encode("msim_fdew_encode_queries", dtype, Qt, q_off, n_q, n_rows, dim, G, S, reps, ksim, dproj, 0, 0, out, codes, stream);
}

}  // extern "C"
