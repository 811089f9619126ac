// The launch form of the FP4 index's scorers (msim_f4_scores in abi_fp4.hip, msim_f4_scores_q6 in abi_fp6.hip): one plan for both,
// which is what msim_f4_scores_plan reports.  Host code only.
#pragma once
#include "fp4_index.hip"

namespace msim_abi {

// the launch form of a shape: every query gets TPQ 16-token tiles, QG queries fill one wave's NT tiles, a longer query takes
// several passes; GW = the waves that share a page range
struct F4Plan {
    static constexpr int NT = 8, D = 4;
    int QG, TPQ, passes, GW, ppw;
    long long n_groups;
};

inline F4Plan f4_plan(int n_q, int max_q_tokens, int n_d, int cus) {
    F4Plan p;
    const int tiles = max_q_tokens ? (max_q_tokens + msim::kF4Tile - 1) / msim::kF4Tile : 1;
    p.QG = 1, p.TPQ = F4Plan::NT, p.passes = 1;
    if (tiles <= F4Plan::NT) {
        p.TPQ = tiles;
        p.QG = F4Plan::NT / tiles;
    } else {
        p.passes = (tiles + F4Plan::NT - 1) / F4Plan::NT;
    }
    p.n_groups = ((long long)n_q + p.QG - 1) / p.QG;
    p.GW = p.n_groups <= 1 ? 1 : p.n_groups == 2 ? 2 : 4;
    // page ranges: enough waves to fill the chip (8 per CU, ~4 rounds); at most 16 pages a range when several query groups re-read it
    const long long want = (long long)(cus > 0 ? cus : 1) * 32;
    const long long work = p.n_groups * n_d;
    const int cap = p.n_groups <= 1 ? msim::kF4MaxRange : 16;
    long long ppw = (work + want - 1) / want;
    p.ppw = (int)(ppw < 1 ? 1 : ppw > cap ? cap : ppw);
    return p;
}

}  // namespace msim_abi
