// F4Plan, the launch form of the FP4 index's scorers (msim_f4_scores in abi_fp4.hip, msim_f4_scores_q6 in abi_fp6.hip): one plan
// for both, which is what msim_f4_scores_plan reports.  The family's plan (abi_fp4_family.hpp) at this kernel file's constants.
#pragma once
#include "abi_fp4_family.hpp"
#include "fp4_index.hip"

namespace msim_abi {
using F4Plan = F4ScanPlan<8, msim::kF4Tile, msim::kF4MaxRange>;
static_assert(kF4Narrow.dim == msim::kDim, "the family's refusals name the kernels' row width");
}  // namespace msim_abi
