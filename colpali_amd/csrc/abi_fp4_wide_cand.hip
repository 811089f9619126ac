// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the list form of the wide FP4 index's scorer (msim_f4w_candidates_plan,
// msim_f4w_candidates).  Host-side dispatch only: argument validation (the family's checks and plans, abi_fp4_family.hpp), kernel
// selection and launch on the caller's stream. Nothing here allocates, frees or synchronises, and nothing reads the list, so both
// entry points are hipGraph-capturable.  The kernels of fp4_wide_candidates.hip are defined and launched in this translation unit
// and in no other; the wide scan kernels it shares constants and helpers with are templates that this unit
// never instantiates, so the unit of abi_fp4_wide.hip compiles to the kernels it had.
#include <hip/hip_runtime.h>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fp4_wide_candidates.hip"
#include "abi_fp4_family.hpp"

using namespace msim_abi;

constexpr F4CandLimits kLimits{msim::kF4wCandMaxTokens, msim::kF4wTile, msim::kF4wCandWaves};
static_assert(kF4Wide.dim == msim::kF4wDim, "the family's refusals name the kernels' row width");

extern "C" {

int msim_f4w_candidates_plan(int n_q, int max_q_tokens, int m, int32_t *plan) {
    return f4_cand_plan_entry("msim_f4w_candidates_plan", kLimits, msim::f4w_cand_depth, n_q, max_q_tokens, m, plan);
}

int msim_f4w_candidates(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                        const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim,
                        const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids,
                        void *stream) {
    const F4Queries qa{q4, qs, q_off, n_q, q_rows, max_q_tokens};
    const F4Pages da{d4, ds, d_off, clamp0, n_d, d_rows, dim};
    F4CandPlan p;
    if (int rc = f4_cand_check("msim_f4w_candidates", kF4Wide, kLimits, qa, da, cand, m, ld_cand, out_scores, ld_scores, out_ids, &p); rc != kF4Launch)
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MSIM_CAND_LAUNCH(N)                                                                                                              \
    case N:                                                                                                                              \
        hipLaunchKernelGGL((msim::f4w_candidates_kernel<N>), dim3((unsigned)p.wgs), dim3(256), 0, st, q4, qs, q_off, n_q,                \
                           (long long)q_rows, d4, ds, d_off, clamp0, n_d, (long long)d_rows, cand, m, (long long)ld_cand,                \
                           (long long)id_base, out_scores, (long long)ld_scores, out_ids);                                               \
        break;
    switch (p.NT) {
        MSIM_CAND_LAUNCH(1)
        MSIM_CAND_LAUNCH(2)
        MSIM_CAND_LAUNCH(4)
        MSIM_CAND_LAUNCH(8)
        default: break;
    }
#undef MSIM_CAND_LAUNCH
    return launch_failed("f4w_candidates_kernel");
}

}  // extern "C"
