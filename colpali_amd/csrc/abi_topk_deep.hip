// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the deep top-k, msim_topk_deep_f32 (1 <= k <= 8192).
// Host-side dispatch only: argument validation, the plan and the launches on the caller's stream.  Nothing here allocates, frees,
// synchronises or reads anything back, and the launch sequence is a function of (n_q, n, k, ids == NULL) alone: the call is
// hipGraph-capturable.  The kernels of topk_deep.hip are defined and launched in this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "topk_deep.hip"

using namespace msim_abi;

static_assert(msim::kDeepMaxK == MSIM_TOPK_DEEP_MAX_K, "the header states the kernels' limit");

namespace {

// The plan, pure arithmetic.  Split rows: implicit ids, fewer rows than half the chip's CUs, rows long enough for eight segments;
// everything else is one workgroup per row, which needs no workspace.
struct DeepPlan {
    bool split;
    long long segs;        // workgroups per row of the split passes
    int cap;               // entries of the LDS sort: the power of two >= max(64, min(k, n))
    size_t zero_bytes;     // head of the workspace: the counts, zeroed on the stream in every call
    size_t seg_hist_bytes;
    size_t surv_bytes;     // each of the two survivor arrays
    size_t bytes;
};

constexpr int kDeepSplitMaxRows = 128;
constexpr long long kDeepSplitMinN = 8LL * msim::kDeepSplitSeg;

DeepPlan deep_plan(bool implicit_ids, int n_q, long long n, int k) {
    DeepPlan p{};
    const long long live = n < k ? n : k;
    p.cap = 64;
    while (p.cap < live) p.cap <<= 1;
    p.split = implicit_ids && n_q < kDeepSplitMaxRows && n >= kDeepSplitMinN;
    if (p.split) {
        p.segs = (n + msim::kDeepSplitSeg - 1) / msim::kDeepSplitSeg;
        p.zero_bytes = align16((size_t)n_q * msim::kDeepRowWords * 4);
        p.seg_hist_bytes = align16((size_t)n_q * p.segs * 256 * 4);
        p.surv_bytes = align16((size_t)n_q * k * 4);
        p.bytes = p.zero_bytes + p.seg_hist_bytes + 2 * p.surv_bytes;
    }
    return p;
}

}  // namespace

extern "C" {

size_t msim_topk_deep_workspace_bytes(int n_q, int64_t n, int k) {
    if (n_q <= 0 || n < 0 || n > 0x7fffffffLL || k <= 0 || k > msim::kDeepMaxK) return 0;
    return deep_plan(true, n_q, n, k).bytes;     // explicit ids always take the row form, which needs none
}

int msim_topk_deep_f32(const float *scores, const int64_t *ids, int n_q, int64_t n, int64_t ld, int k, int64_t id_base,
                       float *out_scores, int64_t *out_ids, void *workspace, void *stream) {
    const char *who = "msim_topk_deep_f32";
    static std::atomic<int> row_configured[kMaxDevices], sort_configured[kMaxDevices];
    if (n_q < 0 || n < 0 || k <= 0) return fail(MSIM_EINVAL, "%s: bad size (n_q=%d n=%lld k=%d)", who, n_q, (long long)n, k);
    if (n_q == 0) return MSIM_OK;
    if (!out_scores || !out_ids || (n > 0 && !scores)) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (k > msim::kDeepMaxK) return fail(MSIM_EUNSUPPORTED, "%s: k=%d > %d", who, k, msim::kDeepMaxK);
    if (n > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: n=%lld >= 2^31", who, (long long)n);
    if (ld < n) return fail(MSIM_EINVAL, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    if (misaligned(scores, 4) || misaligned(out_scores, 4) || misaligned(ids, 8) || misaligned(out_ids, 8))
        return fail(MSIM_EINVAL, "%s: scores must be 4-byte aligned, ids 8-byte aligned", who);
    const DeepPlan p = deep_plan(ids == nullptr, n_q, n, k);
    if (p.bytes > 0 && !workspace) return fail(MSIM_EINVAL, "%s: workspace required (msim_topk_deep_workspace_bytes)", who);
    if (p.bytes > 0 && misaligned(workspace, 16)) return fail(MSIM_EINVAL, "%s: workspace must be 16-byte aligned", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t max_lds = (size_t)msim::kDeepMaxK * msim::kDeepEntryBytes + msim::kDeepLdsTail;
    const size_t lds = (size_t)p.cap * msim::kDeepEntryBytes + msim::kDeepLdsTail;

    if (!p.split) {
        if (int rc = allow_lds(msim::deep_row_kernel, (int)max_lds, row_configured)) return rc;
        int first_id_digit = 0;                  // explicit ids: all eight bytes can differ
        if (!ids) {
            first_id_digit = 8;
            for (long long v = n > 0 ? n - 1 : 0; v; v >>= 8) --first_id_digit;
        }
        hipLaunchKernelGGL(msim::deep_row_kernel, dim3((unsigned)n_q), dim3(msim::kDeepRowThreads), lds, st, scores, ids, (long long)n,
                           (long long)ld, (long long)id_base, k, p.cap, first_id_digit, out_scores, out_ids);
        return launch_failed("deep_row_kernel");
    }

    if (int rc = allow_lds(msim::deep_split_sort_kernel, (int)max_lds, sort_configured)) return rc;
    char *w = static_cast<char *>(workspace);
    uint32_t *counts = reinterpret_cast<uint32_t *>(w);
    uint32_t *seg_hist = reinterpret_cast<uint32_t *>(w + p.zero_bytes);
    uint32_t *surv_key = reinterpret_cast<uint32_t *>(w + p.zero_bytes + p.seg_hist_bytes);
    uint32_t *surv_col = reinterpret_cast<uint32_t *>(w + p.zero_bytes + p.seg_hist_bytes + p.surv_bytes);
    hipError_t e = hipMemsetAsync(counts, 0, p.zero_bytes, st);
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    const dim3 grid((unsigned)p.segs, (unsigned)n_q);
    for (int d = 0; d < 4; ++d)
        hipLaunchKernelGGL(msim::deep_split_hist_kernel, grid, dim3(msim::kDeepSplitThreads), 0, st, scores, (long long)n, (long long)ld, k, d,
                           counts, seg_hist);
    hipLaunchKernelGGL(msim::deep_split_gather_kernel, grid, dim3(msim::kDeepSplitThreads), 0, st, scores, (long long)n, (long long)ld, k,
                       counts, seg_hist, surv_key, surv_col);
    hipLaunchKernelGGL(msim::deep_split_sort_kernel, dim3((unsigned)n_q), dim3(msim::kDeepRowThreads), lds, st, counts, surv_key, surv_col, k,
                       p.cap, (long long)id_base, out_scores, out_ids);
    return launch_failed("deep_split kernels");
}

}  // extern "C"
