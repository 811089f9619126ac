// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the list form of the wide FP4 index's scorer (msim_f4w_candidates_plan,
// msim_f4w_candidates).  Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.
// Nothing here allocates, frees or synchronises, and nothing reads the list, so both entry points are hipGraph-capturable.  The
// kernels of fp4_wide_candidates.hip are defined and launched in this translation unit and in no other; the
// wide scan kernels it shares constants and helpers with are templates that this unit never instantiates, so the unit of
// abi_fp4_wide.hip compiles to the kernels it had.
#include <hip/hip_runtime.h>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fp4_wide_candidates.hip"
#include "abi_fp4_wide_cand_plan.hpp"

using namespace msim_abi;

extern "C" {

int msim_f4w_candidates_plan(int n_q, int max_q_tokens, int m, int32_t *plan) {
    const char *who = "msim_f4w_candidates_plan";
    if (!plan) return fail(MSIM_EINVAL, "%s: null plan", who);
    F4wCandPlan p;
    if (int rc = f4w_cand_plan(who, n_q, max_q_tokens, m, &p)) return rc;
    plan[0] = p.NT;
    plan[1] = p.D;
    plan[2] = msim::kF4wCandWaves;
    plan[3] = (int32_t)p.wgs;
    return MSIM_OK;
}

int msim_f4w_candidates(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                        const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim,
                        const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores,
                        int64_t *out_ids, void *stream) {
    const char *who = "msim_f4w_candidates";
    if (n_q < 0 || n_d < 0 || m < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d m=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, n_q, n_d, m,
                    (long long)q_rows, (long long)d_rows, max_q_tokens);
    if (dim != msim::kF4wDim)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the wide fp4 index takes width %d", who, dim, msim::kF4wDim);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if ((!q4 && q_rows > 0) || (!qs && q_rows > 0) || !q_off || (!d4 && d_rows > 0) || (!ds && d_rows > 0) || (!d_off && n_d > 0) || !cand ||
        !out_scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q4, 16) || misaligned(d4, 16) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(out_scores, 4) ||
        misaligned(cand, 8) || misaligned(out_ids, 8))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; ids 8-byte aligned; offsets and scores 4-byte aligned", who);
    if (ld_cand < m || ld_scores < m)
        return fail(MSIM_EINVAL, "%s: ld_cand=%lld / ld_scores=%lld < m=%d", who, (long long)ld_cand, (long long)ld_scores, m);
    F4wCandPlan p;
    if (int rc = f4w_cand_plan(who, n_q, max_q_tokens, m, &p)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
#define MSIM_F4W_CAND_LAUNCH(N)                                                                                                         \
    case N:                                                                                                                              \
        hipLaunchKernelGGL((msim::f4w_candidates_kernel<N>), dim3((unsigned)p.wgs), dim3(256), 0, st, q4, qs, q_off, n_q,                \
                           (long long)q_rows, d4, ds, d_off, clamp0, n_d, (long long)d_rows, cand, m, (long long)ld_cand,                \
                           (long long)id_base, out_scores, (long long)ld_scores, out_ids);                                               \
        break;
    switch (p.NT) {
        MSIM_F4W_CAND_LAUNCH(1)
        MSIM_F4W_CAND_LAUNCH(2)
        MSIM_F4W_CAND_LAUNCH(4)
        MSIM_F4W_CAND_LAUNCH(8)
        default: break;
    }
#undef MSIM_F4W_CAND_LAUNCH
    return launch_failed("f4w_candidates_kernel");
}

}  // extern "C"
