// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the 13-bit image of a bf16 corpus -- its size, the encoder and the test-only
// decoder.  Host-side dispatch only: argument validation and launch on the caller's stream.  Nothing here allocates, frees or
// synchronises.  The kernels included below are defined and launched in this translation unit and in no other;
// the scorer that reads the image is K1s's packed form (maxsim_stream13.hip, launched from maxsim_abi.hip).
#include <hip/hip_runtime.h>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "pack13.hip"

using namespace msim_abi;

extern "C" {

size_t msim_pack13_image_bytes(int64_t n_slabs) { return n_slabs <= 0 ? 0 : (size_t)n_slabs * msim::kSlab13Bytes; }

int msim_pack13_encode(const void *D, const int32_t *d_off, const int32_t *slab_off, int n_d, int64_t n_slabs, void *image,
                       uint8_t *flags, int32_t *list, int32_t *count, void *stream) {
    if (n_d < 0 || n_slabs < 0 || n_slabs > 0x7fffffff) return fail(MSIM_EINVAL, "msim_pack13_encode: bad size (n_d=%d n_slabs=%lld)", n_d, (long long)n_slabs);
    if (!count || (n_d > 0 && (!d_off || !slab_off || !flags || !list)) || (n_slabs > 0 && (!D || !image)))
        return fail(MSIM_EINVAL, "msim_pack13_encode: null pointer argument");
    if (misaligned(D, 16) || misaligned(image, 16)) return fail(MSIM_EINVAL, "msim_pack13_encode: D and image must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(count, 0, sizeof(int32_t), st) != hipSuccess || (n_d > 0 && hipMemsetAsync(flags, 0, (size_t)n_d, st) != hipSuccess))
        return fail(MSIM_ELAUNCH, "msim_pack13_encode: hipMemsetAsync failed");
    if (n_d == 0) return MSIM_OK;
    if (n_slabs > 0) {
        hipLaunchKernelGGL(msim::pack13_encode_kernel, dim3((unsigned)n_slabs), dim3(128), 0, st, static_cast<const uint16_t *>(D), d_off,
                           slab_off, n_d, static_cast<uint8_t *>(image), flags);
        if (int rc = launch_failed("pack13_encode_kernel")) return rc;
    }
    hipLaunchKernelGGL(msim::pack13_list_kernel, dim3(1), dim3(1024), 0, st, flags, n_d, list, count);
    return launch_failed("pack13_list_kernel");
}

int msim_pack13_decode(const void *image, const int32_t *d_off, const int32_t *slab_off, int n_d, int64_t n_slabs, void *out,
                       void *stream) {
    if (n_d < 0 || n_slabs < 0 || n_slabs > 0x7fffffff) return fail(MSIM_EINVAL, "msim_pack13_decode: bad size (n_d=%d n_slabs=%lld)", n_d, (long long)n_slabs);
    if (n_d == 0 || n_slabs == 0) return MSIM_OK;
    if (!image || !d_off || !slab_off || !out) return fail(MSIM_EINVAL, "msim_pack13_decode: null pointer argument");
    if (misaligned(out, 16) || misaligned(image, 16)) return fail(MSIM_EINVAL, "msim_pack13_decode: out and image must be 16-byte aligned");
    hipLaunchKernelGGL(msim::pack13_decode_kernel, dim3((unsigned)n_slabs), dim3(128), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint8_t *>(image), d_off, slab_off, n_d, static_cast<uint16_t *>(out));
    return launch_failed("pack13_decode_kernel");
}

}  // extern "C"
