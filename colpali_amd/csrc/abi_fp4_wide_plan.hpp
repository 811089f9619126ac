// F4wPlan, the launch form of the wide FP4 index's scorers (msim_f4w_scores in abi_fp4_wide.hip, msim_f4w_scores_q6 in
// abi_fp6_wide.hip): one plan for both, which is what msim_f4w_scores_plan reports.  The family's plan (abi_fp4_family.hpp) at this
// kernel file's constants.
#pragma once
#include "abi_fp4_family.hpp"
#include "fp4_wide_index.hip"

namespace msim_abi {
using F4wPlan = F4ScanPlan<4, msim::kF4wTile, msim::kF4wMaxRange>;   // NT = 4: (8, 4) and (8, 2) were measured and are slower
static_assert(kF4Wide.dim == msim::kF4wDim, "the family's refusals name the kernels' row width");
}  // namespace msim_abi
