// The launch form of the wide FP4 index's scorers (msim_f4w_scores in abi_fp4_wide.hip, msim_f4w_scores_q6 in abi_fp6_wide.hip):
// one plan for both, which is what msim_f4w_scores_plan reports.  Host code only.
#pragma once
#include "fp4_wide_index.hip"

namespace msim_abi {

// the launch form of a shape: every query gets TPQ 16-token tiles, QG queries fill one wave's NT tiles, a longer query takes
// several passes; GW = the waves that share a page range
struct F4wPlan {
    static constexpr int NT = 4, D = 4;                                // (8, 4) and (8, 2) were measured and are slower
    int QG, TPQ, passes, GW, ppw;
    long long n_groups;
};

inline F4wPlan f4w_plan(int n_q, int max_q_tokens, int n_d, int cus) {
    F4wPlan p;
    const int tiles = max_q_tokens ? (max_q_tokens + msim::kF4wTile - 1) / msim::kF4wTile : 1;
    p.QG = 1, p.TPQ = F4wPlan::NT, p.passes = 1;
    if (tiles <= F4wPlan::NT) {
        p.TPQ = tiles;
        p.QG = F4wPlan::NT / tiles;
    } else {
        p.passes = (tiles + F4wPlan::NT - 1) / F4wPlan::NT;
    }
    p.n_groups = ((long long)n_q + p.QG - 1) / p.QG;
    p.GW = p.n_groups <= 1 ? 1 : p.n_groups == 2 ? 2 : 4;
    // page ranges: enough waves to fill the chip (8 per CU, ~4 rounds); at most 16 pages a range when several query groups re-read it
    const long long want = (long long)(cus > 0 ? cus : 1) * 32;
    const long long work = p.n_groups * n_d;
    const int cap = p.n_groups <= 1 ? msim::kF4wMaxRange : 16;
    long long ppw = (work + want - 1) / want;
    p.ppw = (int)(ppw < 1 ? 1 : ppw > cap ? cap : ppw);
    return p;
}

}  // namespace msim_abi
