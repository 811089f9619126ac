// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the embedding head at width 320 (msim_embed_head_wide*).
// Host-side dispatch only: argument validation and launch on the caller's stream.  Nothing here allocates, frees or synchronises,
// so every entry point is hipGraph-capturable.  The kernels of embed_head_wide.hip are defined and launched in this translation
// unit and in no other: a unit of its own, so that no kernel of another unit is compiled beside them.  The
// row maps come from msim_embed_head_row_map / msim_embed_head_writer_map (abi_head_pool.hip), which do not depend on the width.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "embed_head_wide.hip"

using namespace msim_abi;

namespace {

int head_wide_check_kind(const char *who, int dtype, int n_out) {
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16)
        return fail(MSIM_EUNSUPPORTED, "%s: dtype code %d: the embedding head takes bfloat16 (0) or float16 (1)", who, dtype);
    if (n_out != msim::kHwN)
        return fail(MSIM_EUNSUPPORTED, "%s: n_out=%d: this entry is built for 320 output columns (msim_embed_head takes 128)", who, n_out);
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_embed_head_wide(int dtype, const void *X, int64_t M, int H, const void *W, const void *bias, int n_out,
                         const int32_t *row_map, void *out, int64_t ld_out, void *stream) {
    const char *who = "msim_embed_head_wide";
    if (M < 0 || H <= 0) return fail(MSIM_EINVAL, "%s: bad size (M=%lld H=%d)", who, (long long)M, H);
    if (M == 0) return MSIM_OK;
    if (!X || !W || !row_map || !out) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (int rc = head_wide_check_kind(who, dtype, n_out)) return rc;
    if (H % msim::kHwBK != 0 || H > msim::kHwMaxH)
        return fail(MSIM_EUNSUPPORTED, "%s: H=%d: hidden size must be a multiple of 64, <= %d", who, H, msim::kHwMaxH);
    if (misaligned(X, 16) || misaligned(W, 16) || misaligned(out, 16))
        return fail(MSIM_EINVAL, "%s: X, W and out must be 16-byte aligned", who);
    if (ld_out < msim::kHwN || ld_out % 8 != 0)
        return fail(MSIM_EINVAL, "%s: ld_out=%lld must be at least 320 and a multiple of 8", who, (long long)ld_out);
    if (M > 0x7ffffffdLL) return fail(MSIM_EUNSUPPORTED, "%s: too many rows for an int32 row map", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::HeadWideArgs a;
    a.M = M;
    a.H = H;
    a.ld_out = ld_out;
    const long long tiles = (M + msim::kHwBM - 1) / msim::kHwBM;
    const int grid = tiles < di->cus ? (int)tiles : di->cus;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = f16 ? msim::embed_head_wide_kernel<true> : msim::embed_head_wide_kernel<false>;
    static std::atomic<int> configured_bf16[kMaxDevices], configured_f16[kMaxDevices];
    if (int rc = allow_lds(kern, msim::kHwLds, f16 ? configured_f16 : configured_bf16)) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(msim::kHwThreads), msim::kHwLds, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(X), static_cast<const uint16_t *>(W), static_cast<const uint16_t *>(bias), row_map,
                       static_cast<uint16_t *>(out), a);
    return launch_failed("embed_head_wide_kernel");
}

int msim_embed_head_wide_bwd(int dtype, const void *proj, const void *grad_out, const int32_t *row_map, int64_t M, int n_out,
                             void *dproj, void *stream) {
    const char *who = "msim_embed_head_wide_bwd";
    if (M < 0) return fail(MSIM_EINVAL, "%s: bad size (M=%lld)", who, (long long)M);
    if (M == 0) return MSIM_OK;
    if (!proj || !grad_out || !row_map || !dproj) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (int rc = head_wide_check_kind(who, dtype, n_out)) return rc;
    if (misaligned(proj, 16) || misaligned(grad_out, 16) || misaligned(dproj, 16))
        return fail(MSIM_EINVAL, "%s: proj, grad_out and dproj must be 16-byte aligned", who);
    if (M > 0x7ffffffdLL) return fail(MSIM_EUNSUPPORTED, "%s: too many rows for an int32 row map", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const long long blocks = (M + 31) / 32;
    const int grid = (int)(blocks < (long long)di->cus * 16 ? blocks : (long long)di->cus * 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *p = static_cast<const uint16_t *>(proj), *g = static_cast<const uint16_t *>(grad_out);
    uint16_t *o = static_cast<uint16_t *>(dproj);
    if (dtype == MSIM_DTYPE_F16)
        hipLaunchKernelGGL(msim::embed_head_wide_bwd_rows_kernel<true>, dim3(grid), dim3(256), 0, st, p, g, row_map, (long long)M, o);
    else
        hipLaunchKernelGGL(msim::embed_head_wide_bwd_rows_kernel<false>, dim3(grid), dim3(256), 0, st, p, g, row_map, (long long)M, o);
    return launch_failed("embed_head_wide_bwd_rows_kernel");
}

}  // extern "C"
