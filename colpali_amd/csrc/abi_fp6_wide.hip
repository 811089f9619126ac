// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): e2m3 query tokens against the FP4 index at width 320 (msim_f6w_encode_rows,
// msim_f4w_scores_q6).  Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing
// here allocates, frees or synchronises, so every entry point is hipGraph-capturable.  The kernels of fp6_wide_query.hip are
// defined and launched in this translation unit and in no other; the wide FP4 kernels it shares constants
// and helpers with are templates that this unit never instantiates, so the unit of abi_fp4_wide.hip compiles to the kernels it had.
#include <hip/hip_runtime.h>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fp6_wide_query.hip"
#include "abi_fp4_wide_plan.hpp"

using namespace msim_abi;

namespace {

template <int GW>
int f6w_scores_launch(const F4wPlan &p, const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows,
                      const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows,
                      float *scores, int64_t ld, hipStream_t st) {
    const long long n_gb = (p.n_groups + GW - 1) / GW;
    const long long n_ranges = ((long long)n_d + p.ppw - 1) / p.ppw, n_pb = (n_ranges + 4 / GW - 1) / (4 / GW);
    if (n_gb * n_pb > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "msim_f4w_scores_q6: %lld workgroups exceed one launch", n_gb * n_pb);
    hipLaunchKernelGGL((msim::f4w_scores_q6_kernel<F4wPlan::NT, GW, F4wPlan::D>), dim3((unsigned)(n_gb * n_pb)), dim3(256), 0, st, q6, qs,
                       q_off, n_q, (long long)q_rows, p.QG, p.TPQ, p.passes, d4, ds, d_off, clamp0, n_d, (long long)d_rows, p.ppw,
                       (int)p.n_groups, (int)n_gb, scores, (long long)ld);
    return launch_failed("f4w_scores_q6_kernel");
}

}  // namespace

extern "C" {

int msim_f6w_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes, uint8_t *scales, void *stream) {
    const char *who = "msim_f6w_encode_rows";
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (dim != msim::kF4wDim)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the wide fp4 index takes width %d", who, dim, msim::kF4wDim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    if (n_rows == 0) return MSIM_OK;
    if (!X || !codes || !scales) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(X, 16) || misaligned(codes, 16)) return fail(MSIM_EINVAL, "%s: rows and codes must be 16-byte aligned", who);
    if ((n_rows + 31) / 32 > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::f6w_encode_rows_kernel<true> : msim::f6w_encode_rows_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_rows + 31) / 32)), dim3(256), 0, st, static_cast<const uint16_t *>(X), (long long)n_rows,
                       codes, scales);
    return launch_failed("f6w_encode_rows_kernel");
}

int msim_f4w_scores_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                       const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim,
                       float *scores, int64_t ld_scores, void *stream) {
    const char *who = "msim_f4w_scores_q6";
    if (n_q < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, n_q, n_d,
                    (long long)q_rows, (long long)d_rows, max_q_tokens);
    if (dim != msim::kF4wDim)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the wide fp4 index takes width %d", who, dim, msim::kF4wDim);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if ((!q6 && q_rows > 0) || (!qs && q_rows > 0) || !q_off || (!d4 && d_rows > 0) || (!ds && d_rows > 0) || !d_off || !scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q6, 16) || misaligned(d4, 16) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(scores, 4))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; offsets and scores 4-byte aligned", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (max_q_tokens > (1 << 20)) return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, 1 << 20);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const F4wPlan p = f4w_plan(n_q, max_q_tokens, n_d, di->cus);
    if (p.GW == 1)
        return f6w_scores_launch<1>(p, q6, qs, q_off, n_q, q_rows, d4, ds, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
    if (p.GW == 2)
        return f6w_scores_launch<2>(p, q6, qs, q_off, n_q, q_rows, d4, ds, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
    return f6w_scores_launch<4>(p, q6, qs, q_off, n_q, q_rows, d4, ds, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
}

}  // extern "C"
