// The query groups of the full scan of a residual-compressed shard (residual_scan.hip at width 128, residual_wide_scan.hip at width
// 320): the group table in the workspace and the greedy rule that fills it, applied by the host to q_off_host and by each scan's
// prologue kernel to the device q_off.  Nothing here depends on the row width, and no kernel lives here: each translation unit
// defines and launches its own.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kResScanGroupQueries = 8;                   // 8 reduction lanes per query: at most 8 queries share a wave
constexpr int kResScanStatusBytes = 16;                   // status word, device group count, two spare words
struct ResScanGroup {                                     // 16 bytes of the workspace per group
    int q0, nq;                                           // queries q0 .. q0 + nq - 1
    int tok0, tok1;                                       // their tokens: rows tok0 .. tok1 - 1 of the flat token matrix
};

// the greedy rule, one query at a time: does query (tokens prev .. e - 1) open a new group?
__host__ __device__ inline bool res_scan_new_group(int cur_nq, int cur_tok0, int e, int cap_units) {
    return cur_nq > 0 && (cur_nq + 1 > kResScanGroupQueries || e - cur_tok0 > cap_units * kUnitTok);
}

}  // namespace msim
