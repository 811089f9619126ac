// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): e2m3 query tokens against the FP4 index (msim_f6_encode_rows,
// msim_f4_scores_q6).  Host-side dispatch only: argument validation (the family's checks and plans, abi_fp4_family.hpp), kernel
// selection and launch on the caller's stream.  Nothing here allocates, frees or synchronises, so every entry point is
// hipGraph-capturable.  The kernels of fp6_query.hip are defined and launched in this translation unit and in no other (DESIGN.md
// section 1); the FP4 kernels it shares constants with are templates that this unit never instantiates, so the unit of abi_fp4.hip
// compiles to the kernels it had.
#include <hip/hip_runtime.h>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fp6_query.hip"
#include "abi_fp4_plan.hpp"

using namespace msim_abi;

namespace {

constexpr int kEncodeRows = 16;                 // rows per workgroup of f6_encode_rows_kernel

template <int GW>
int f6_scores_launch(const F4Plan &p, const F4Queries &q, const F4Pages &d, float *scores, int64_t ld, hipStream_t st) {
    hipLaunchKernelGGL((msim::f4_scores_q6_kernel<F4Plan::NT, GW, F4Plan::D>), dim3((unsigned)(p.n_gb * p.n_pb)), dim3(256), 0, st, q.codes, q.scales,
                       q.off, q.n_q, (long long)q.rows, p.QG, p.TPQ, p.passes, d.codes, d.scales, d.off, d.clamp0, d.n_d, (long long)d.rows,
                       p.ppw, (int)p.n_groups, (int)p.n_gb, scores, (long long)ld);
    return launch_failed("f4_scores_q6_kernel");
}

}  // namespace

extern "C" {

int msim_f6_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes, uint8_t *scales, void *stream) {
    if (int rc = f4_encode_check("msim_f6_encode_rows", kF4Narrow, kEncodeRows, dtype, X, n_rows, dim, codes, scales); rc != kF4Launch) return rc;
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::f6_encode_rows_kernel<true> : msim::f6_encode_rows_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_rows + kEncodeRows - 1) / kEncodeRows)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(X), (long long)n_rows, codes, scales);
    return launch_failed("f6_encode_rows_kernel");
}

int msim_f4_scores_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                      const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim,
                      float *scores, int64_t ld_scores, void *stream) {
    const F4Queries qa{q6, qs, q_off, n_q, q_rows, max_q_tokens};
    const F4Pages da{d4, ds, d_off, clamp0, n_d, d_rows, dim};
    F4Plan p;
    if (int rc = f4_scan_check("msim_f4_scores_q6", kF4Narrow, qa, da, scores, ld_scores, &p); rc != kF4Launch) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.GW == 1) return f6_scores_launch<1>(p, qa, da, scores, ld_scores, st);
    if (p.GW == 2) return f6_scores_launch<2>(p, qa, da, scores, ld_scores, st);
    return f6_scores_launch<4>(p, qa, da, scores, ld_scores, st);
}

}  // extern "C"
