// The launch form of the list forms of the wide FP4 index's scorers (msim_f4w_candidates in abi_fp4_wide_cand.hip,
// msim_f4w_candidates_q6 in abi_fp6_wide_cand.hip): one plan and one set of refusals for both, which is what
// msim_f4w_candidates_plan reports.  Host code only.
#pragma once
#include "abi_common.hpp"
#include "fp4_wide_candidates.hip"

namespace msim_abi {

// the launch form: NT = the 16-token tiles a wave holds (the smallest of 1, 2, 4, 8 that covers max_q_tokens), D = the chunks it
// loads ahead, one workgroup of four waves per four entries
struct F4wCandPlan {
    int NT, D;
    long long wgs;
};

// MSIM_OK, or the refusal both the plan entry and the scorer give
inline int f4w_cand_plan(const char *who, int n_q, int max_q_tokens, int m, F4wCandPlan *p) {
    if (n_q < 0 || m < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d max_q_tokens=%d)", who, n_q, m, max_q_tokens);
    if (max_q_tokens > msim::kF4wCandMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, msim::kF4wCandMaxTokens);
    const int tiles = (max_q_tokens + msim::kF4wTile - 1) / msim::kF4wTile;
    p->NT = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
    p->D = msim::f4w_cand_depth(p->NT);
    p->wgs = ((long long)n_q * m + msim::kF4wCandWaves - 1) / msim::kF4wCandWaves;
    if (p->wgs > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld workgroups exceed one launch", who, p->wgs);
    return MSIM_OK;
}

}  // namespace msim_abi
