// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the residual-compressed shard at width 320 (msim_cent_wide_*, msim_res_wide_*)
// -- the centroid-code encoder and query table, the residual codec, the candidate rerank, the full scan, and align / gather_pages over
// the compressed rows.
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates, frees or
// synchronises, so every entry point is hipGraph-capturable.  The kernels of residual_wide.hip, residual_wide_scan.hip and
// residual_wide_align.hip are defined and launched in this translation unit and in no other.  The table msim_cent_wide_table writes is scanned by msim_cent_scores
// (abi_index.hip), which depends on the table and the codes alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "residual_wide.hip"
#include "residual_wide_align.hip"
#include "residual_wide_scan.hip"

using namespace msim_abi;

namespace {

// the split of the 128 entries: another width or dtype is a format the kernels do not have, a centroid count outside the range a bad argument
int cw_check_format(const char *who, int dtype, int dim, int K) {
    if (dim != msim::kRwDim)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the wide centroid index takes width %d", who, dim, msim::kRwDim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    if (K < msim::kRwMinK || K > msim::kRwMaxK || K % 256 != 0)
        return fail(MSIM_EINVAL, "%s: %d centroids; the count is a multiple of 256 from %d to %d", who, K, msim::kRwMinK, msim::kRwMaxK);
    return MSIM_OK;
}

int rw_check_format(const char *who, int dtype, int dim, int K, int bits) {
    if (int rc = cw_check_format(who, dtype, dim, K)) return rc;
    if (!(bits == 2 || bits == 4)) return fail(MSIM_EUNSUPPORTED, "%s: %d residual bits; the codec stores 2 or 4 per dimension", who, bits);
    return MSIM_OK;
}

int cw_blocks(int max_q_tokens) { return max_q_tokens > 0 ? (max_q_tokens + msim::kRwBlockTok - 1) / msim::kRwBlockTok : 1; }

}  // namespace

extern "C" {

int msim_cent_wide_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows,
                               const void *C, int K, uint16_t *codes, int32_t *status, void *stream) {
    const char *who = "msim_cent_wide_encode_docs";
    if (n_d < 0 || n_rows < 0 || max_doc_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_d=%d rows=%lld max_doc_rows=%d)", who, n_d, (long long)n_rows, max_doc_rows);
    if (int rc = cw_check_format(who, dtype, dim, K)) return rc;
    if (n_d == 0 || max_doc_rows == 0) return MSIM_OK;
    if ((!D && n_rows > 0) || !d_off || !C || (!codes && n_rows > 0)) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(C, 16) || misaligned(codes, 16) || misaligned(d_off, 4) || misaligned(status, 4))
        return fail(MSIM_EINVAL, "%s: rows, centroids and codes must be 16-byte aligned, offsets and status 4-byte aligned", who);
    const long long gy = ((long long)max_doc_rows + msim::kRwEncRows - 1) / msim::kRwEncRows;
    if (gy > 65535) return fail(MSIM_EUNSUPPORTED, "%s: max_doc_rows=%d above %d", who, max_doc_rows, 65535 * msim::kRwEncRows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::cent_wide_encode_kernel<true> : msim::cent_wide_encode_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_d, (unsigned)gy), dim3(256), 0, st, static_cast<const uint16_t *>(D), d_off, n_d,
                       (long long)n_rows, max_doc_rows, static_cast<const uint16_t *>(C), K, codes, status);
    return launch_failed("cent_wide_encode_kernel");
}

int msim_cent_wide_table(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int dim,
                         const void *C, int K, void *table, void *stream) {
    const char *who = "msim_cent_wide_table";
    if (n_q < 0 || q_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d q_rows=%lld max_q_tokens=%d)", who, n_q, (long long)q_rows, max_q_tokens);
    if (int rc = cw_check_format(who, dtype, dim, K)) return rc;
    if (max_q_tokens > msim::kRwMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, msim::kRwMaxTokens);
    if (n_q == 0) return MSIM_OK;
    if ((!Qt && q_rows > 0) || !q_off || !C || !table) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(table, 16) || misaligned(q_off, 4))
        return fail(MSIM_EINVAL, "%s: tokens, centroids and table must be 16-byte aligned, offsets 4-byte aligned", who);
    const int nb = cw_blocks(max_q_tokens);
    if ((long long)n_q * nb > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld blocks exceed one launch", who, (long long)n_q * nb);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::cent_wide_table_kernel<true> : msim::cent_wide_table_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n_q * nb), (unsigned)(K / 256)), dim3(256), 0, st, static_cast<const uint16_t *>(Qt), q_off,
                       n_q, (long long)q_rows, nb, static_cast<const uint16_t *>(C), K, static_cast<_Float16 *>(table));
    return launch_failed("cent_wide_table_kernel");
}

int msim_res_wide_encode_docs(int dtype, const void *D, int64_t n_rows, int dim, const uint16_t *codes, const void *C, int K,
                              const float *cutoffs, int bits, uint8_t *residuals, void *stream) {
    const char *who = "msim_res_wide_encode_docs";
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (n_rows == 0) return MSIM_OK;
    if (!D || !codes || !C || !cutoffs || !residuals) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(codes, 2) || misaligned(cutoffs, 4))
        return fail(MSIM_EINVAL, "%s: rows, centroids and residuals must be 16-byte aligned, codes 2-byte and cutoffs 4-byte aligned", who);
    if (n_rows > 0x7fffffffLL * 256 / msim::kRwChunks) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const long long blocks = (n_rows * msim::kRwChunks + 255) / 256;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_encode_kernel<true, 2> : msim::res_wide_encode_kernel<false, 2>)
                          : (f16 ? msim::res_wide_encode_kernel<true, 4> : msim::res_wide_encode_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(D), codes,
                       (long long)n_rows, static_cast<const uint16_t *>(C), K, cutoffs, residuals);
    return launch_failed("res_wide_encode_kernel");
}

int msim_res_wide_decode_rows(int dtype, const uint16_t *codes, const uint8_t *residuals, int64_t n_rows, int64_t row0, int64_t row1,
                              const void *C, int K, const float *weights, int bits, int dim, void *out, void *stream) {
    const char *who = "msim_res_wide_decode_rows";
    if (n_rows < 0 || row0 < 0 || row1 < row0 || row1 > n_rows)
        return fail(MSIM_EINVAL, "%s: rows %lld .. %lld of %lld", who, (long long)row0, (long long)row1, (long long)n_rows);
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (row1 == row0) return MSIM_OK;
    if (!codes || !residuals || !C || !weights || !out) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(out, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(codes, 2) || misaligned(weights, 4))
        return fail(MSIM_EINVAL, "%s: out, centroids and residuals must be 16-byte aligned, codes 2-byte and weights 4-byte aligned", who);
    if (row1 - row0 > 0x7fffffffLL * 256 / msim::kRwChunks)
        return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)(row1 - row0));
    const long long blocks = ((row1 - row0) * msim::kRwChunks + 255) / 256;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_decode_kernel<true, 2> : msim::res_wide_decode_kernel<false, 2>)
                          : (f16 ? msim::res_wide_decode_kernel<true, 4> : msim::res_wide_decode_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), codes, residuals, (long long)row0,
                       (long long)row1, static_cast<const uint16_t *>(C), K, weights, static_cast<uint16_t *>(out));
    return launch_failed("res_wide_decode_kernel");
}

// one wave scores one entry from the page's own rows: nothing is inverted, so the workspace is the status word alone
size_t msim_res_wide_candidates_workspace_bytes(int n_q, int m, int n_d) {
    if (n_q <= 0 || m <= 0 || n_d < 0) return 0;
    return 16;
}

int msim_res_wide_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                             const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                             const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand,
                             int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids, void *workspace, void *stream) {
    const char *who = "msim_res_wide_candidates";
    if (n_q < 0 || m < 0 || n_d < 0 || d_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d n_d=%d d_rows=%lld)", who, n_q, m, n_d, (long long)d_rows);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (!Qt || !q_off || !q_off_host || ((!codes || !residuals) && d_rows > 0) || !C || !weights || !d_off || !cand || !out_scores ||
        !workspace)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(workspace, 16) || misaligned(codes, 2) ||
        misaligned(weights, 4) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(out_scores, 4) || misaligned(cand, 8) ||
        misaligned(out_ids, 8))
        return fail(MSIM_EINVAL, "%s: Qt, centroids, residuals and workspace must be 16-byte aligned; the rest by their element size", who);
    if (ld_cand < m) return fail(MSIM_EINVAL, "%s: ld_cand=%lld < m=%d", who, (long long)ld_cand, m);
    if (ld_scores < m) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < m=%d", who, (long long)ld_scores, m);
    if ((long long)n_q * m > 0x7fffffff) return fail(MSIM_EUNSUPPORTED, "%s: more than 2^31 - 1 entries (n_q=%d x m=%d)", who, n_q, m);
    if (d_rows > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld exceeds 32-bit page offsets", who, (long long)d_rows);
    if (q_off_host[0] != 0) return fail(MSIM_EINVAL, "%s: q_off[0] must be 0", who);
    for (int i = 0; i < n_q; ++i) {
        const int len = q_off_host[i + 1] - q_off_host[i];
        if (len < 0) return fail(MSIM_EINVAL, "%s: q_off must be non-decreasing (query %d)", who, i);
        if (len > msim::kStreamMaxUnits * msim::kUnitTok)
            return fail(MSIM_EUNSUPPORTED, "query %d has %d tokens: %s takes queries of at most %d", i, len, who,
                        msim::kStreamMaxUnits * msim::kUnitTok);
    }
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *status = static_cast<int32_t *>(workspace);
    const long long E = (long long)n_q * m;
    const unsigned eblocks = (unsigned)((E + 255) / 256);
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_candidates_kernel<true, 2> : msim::res_wide_candidates_kernel<false, 2>)
                          : (f16 ? msim::res_wide_candidates_kernel<true, 4> : msim::res_wide_candidates_kernel<false, 4>);
    static_assert(msim::kRwLdsBytes <= 160 * 1024, "res_wide_candidates_kernel: four waves' panel-slabs must fit the CU's LDS");
    static std::atomic<int> configured[2][2][kMaxDevices];
    if (int rc = allow_lds(kern, msim::kRwLdsBytes, configured[bits == 4][f16])) return rc;
    hipLaunchKernelGGL(msim::res_wide_zero_status_kernel, dim3(1), dim3(64), 0, st, status);
    // a persistent grid: one entry per wave at a time, one workgroup per CU (its LDS holds one, and a wave runs alone on its SIMD)
    const long long wg_needed = (E + 3) / 4;
    const long long wg_cap = (long long)di->cus;
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), msim::kRwLdsBytes, st,
                       static_cast<const uint16_t *>(Qt), q_off, n_q, (long long)q_off_host[n_q], codes, residuals,
                       static_cast<const uint16_t *>(C), K, weights, d_off, d_clamp0, n_d, (long long)d_rows, cand, (long long)ld_cand, m,
                       (long long)id_base, out_scores, (long long)ld_scores, out_ids, status);
    hipLaunchKernelGGL(msim::res_wide_poison_kernel, dim3(eblocks), dim3(256), 0, st, status, n_q, m, out_scores, (long long)ld_scores);
    return launch_failed("res_wide_candidates_kernel");
}

// the full scan: the status words plus one 16-byte group per query at most -- a function of n_q alone, never of the row count
size_t msim_res_wide_scores_workspace_bytes(int n_q, int n_d) {
    if (n_q <= 0 || n_d <= 0) return 0;
    return align16(msim::kResScanStatusBytes + (size_t)n_q * sizeof(msim::ResScanGroup));
}

int msim_res_wide_scores(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                         const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                         const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, float *out_scores, int64_t ld_scores, void *workspace,
                         void *stream) {
    const char *who = "msim_res_wide_scores";
    if (n_q < 0 || n_d < 0 || d_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d d_rows=%lld)", who, n_q, n_d, (long long)d_rows);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (!Qt || !q_off || !q_off_host || ((!codes || !residuals) && d_rows > 0) || !C || !weights || !d_off || !out_scores || !workspace)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(workspace, 16) || misaligned(codes, 2) ||
        misaligned(weights, 4) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(out_scores, 4))
        return fail(MSIM_EINVAL, "%s: Qt, centroids, residuals and workspace must be 16-byte aligned; the rest by their element size", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (d_rows > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld exceeds 32-bit page offsets", who, (long long)d_rows);
    if (q_off_host[0] != 0) return fail(MSIM_EINVAL, "%s: q_off[0] must be 0", who);
    // the checks of the offsets and, by the rule the device applies to its own copy (residual_scan_groups.hpp), the number of query groups
    const int cap_units = std::min(std::max(ab_env("MSIM_RES_SCAN_UNITS", msim::kRwScanGroupUnits), 1), msim::kStreamMaxUnits);
    int n_groups = 0, cur_nq = 0, cur_tok0 = 0;
    for (int i = 0; i < n_q; ++i) {
        const int len = q_off_host[i + 1] - q_off_host[i];
        if (len < 0) return fail(MSIM_EINVAL, "%s: q_off must be non-decreasing (query %d)", who, i);
        if (len > msim::kStreamMaxUnits * msim::kUnitTok)
            return fail(MSIM_EUNSUPPORTED, "query %d has %d tokens: %s takes queries of at most %d", i, len, who,
                        msim::kStreamMaxUnits * msim::kUnitTok);
        if (msim::res_scan_new_group(cur_nq, cur_tok0, q_off_host[i + 1], cap_units)) {
            ++n_groups;
            cur_nq = 0;
            cur_tok0 = q_off_host[i];
        }
        ++cur_nq;
    }
    ++n_groups;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *status = static_cast<int32_t *>(workspace);
    auto *groups = reinterpret_cast<msim::ResScanGroup *>(static_cast<char *>(workspace) + msim::kResScanStatusBytes);
    const long long q_rows = q_off_host[n_q];
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_scan_kernel<true, 2> : msim::res_wide_scan_kernel<false, 2>)
                          : (f16 ? msim::res_wide_scan_kernel<true, 4> : msim::res_wide_scan_kernel<false, 4>);
    static std::atomic<int> configured[2][2][kMaxDevices];
    if (int rc = allow_lds(kern, msim::kRwLdsBytes, configured[bits == 4][f16])) return rc;
    hipLaunchKernelGGL(msim::res_wide_scan_groups_kernel, dim3(1), dim3(64), 0, st, q_off, n_q, q_rows, cap_units, n_groups, groups, status);
    // a persistent grid: every wave walks pages of its own, one workgroup per CU (its LDS holds one, and a wave runs alone on its SIMD)
    const long long wg_needed = ((long long)n_d + 3) / 4;
    const long long wg_cap = (long long)di->cus;
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), msim::kRwLdsBytes, st,
                       static_cast<const uint16_t *>(Qt), q_off, n_q, q_rows, codes, residuals, static_cast<const uint16_t *>(C), K, weights,
                       d_off, d_clamp0, n_d, (long long)d_rows, out_scores, (long long)ld_scores, groups, n_groups, status);
    const long long pblocks = ((long long)n_q * n_d + 255) / 256;
    hipLaunchKernelGGL(msim::res_wide_scan_poison_kernel, dim3((unsigned)(pblocks < wg_cap * 8 ? pblocks : wg_cap * 8)), dim3(256), 0, st,
                       status, n_q, n_d, out_scores, (long long)ld_scores);
    return launch_failed("res_wide_scan_kernel");
}

// K1a's contract at width 320 over the compressed rows: every wave decodes the chunks it multiplies, nothing is staged or allocated
int msim_res_wide_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                                   const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights, int bits,
                                   const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, const int64_t *cand,
                                   int m, int64_t ld_cand, int64_t id_base, float *best_sim, int32_t *best_row, float *sims, int max_rows,
                                   void *stream) {
    const char *who = "msim_res_wide_align_candidates";
    if (n_q < 0 || m < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0 || max_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d max_rows=%d)", who, n_q,
                    m, n_d, (long long)q_rows, (long long)d_rows, max_q_tokens, max_rows);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (max_q_tokens > msim::kAlignMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d: queries of at most %d tokens", who, max_q_tokens, msim::kAlignMaxTokens);
    if ((!Qt && q_rows > 0) || !q_off || ((!codes || !residuals) && d_rows > 0) || !C || !weights || !d_off || !cand ||
        ((!best_sim || !best_row) && max_q_tokens > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(residuals, 16))
        return fail(MSIM_EINVAL, "%s: Qt, centroids and residuals must be 16-byte aligned", who);
    if (misaligned(codes, 2) || misaligned(weights, 4) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(cand, 8) ||
        misaligned(best_sim, 4) || misaligned(best_row, 4) || misaligned(sims, 4))
        return fail(MSIM_EINVAL, "%s: codes must be 2-byte aligned; weights, offsets and outputs 4-byte aligned, cand 8-byte aligned", who);
    if (ld_cand < m) return fail(MSIM_EINVAL, "%s: ld_cand=%lld < m=%d", who, (long long)ld_cand, m);
    if ((long long)n_q * m > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: more than 2^31 - 1 entries (n_q=%d x m=%d)", who, n_q, m);
    if (d_rows > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld exceeds 32-bit page offsets", who, (long long)d_rows);
    if (max_q_tokens == 0) return MSIM_OK;                       // no token slot: nothing to write
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::AlignArgs a;
    a.ld_cand = ld_cand;
    a.id_base = id_base;
    a.q_rows = q_rows;
    a.d_rows = d_rows;
    a.n_q = n_q;
    a.m = m;
    a.n_d = n_d;
    a.T = max_q_tokens;
    a.R = max_rows;
    a.vec = sims && !misaligned(sims, 16) && max_rows % 4 == 0;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_align_kernel<true, 2> : msim::res_wide_align_kernel<false, 2>)
                          : (f16 ? msim::res_wide_align_kernel<true, 4> : msim::res_wide_align_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)n_q * m)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(Qt), q_off, codes, residuals, static_cast<const uint16_t *>(C), K, weights, d_off,
                       d_clamp0, cand, best_sim, best_row, sims, a);
    return launch_failed("res_wide_align_kernel");
}

// msim_gather_pages' contract (row_bytes 640) over the compressed rows: the box is decoded into, never copied from a decoded page
int msim_res_wide_gather_pages(int dtype, const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights,
                               int bits, int dim, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base, const int64_t *ids,
                               int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream) {
    const char *who = "msim_res_wide_gather_pages";
    if (n_slots < 0 || n_d < 0 || d_rows < 0 || pad_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_slots=%lld n_d=%d d_rows=%lld pad_rows=%lld)", who, (long long)n_slots, n_d,
                    (long long)d_rows, (long long)pad_rows);
    if (n_slots == 0) return MSIM_OK;
    if (int rc = rw_check_format(who, dtype, dim, K, bits)) return rc;
    if (d_rows > 0x7fffffffLL || pad_rows > 0x7fffffffLL || n_slots > 0x7fffffffLL)
        return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld, pad_rows=%lld or n_slots=%lld above 2^31 - 1", who, (long long)d_rows,
                    (long long)pad_rows, (long long)n_slots);
    if (!ids || !lengths || !d_off || ((!codes || !residuals) && d_rows > 0) || !C || !weights || (!out && pad_rows > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(out, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(codes, 2) || misaligned(weights, 4) ||
        misaligned(ids, 8) || misaligned(d_off, 4) || misaligned(lengths, 4))
        return fail(MSIM_EINVAL, "%s: out, centroids and residuals must be 16-byte aligned, ids 8-byte, codes 2-byte, weights, d_off and "
                    "lengths 4-byte aligned", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_wide_gather_pages_kernel<true, 2> : msim::res_wide_gather_pages_kernel<false, 2>)
                          : (f16 ? msim::res_wide_gather_pages_kernel<true, 4> : msim::res_wide_gather_pages_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream), codes, residuals,
                       static_cast<const uint16_t *>(C), K, weights, (long long)d_rows, d_off, n_d, (long long)id_base, ids,
                       (long long)pad_rows, static_cast<uint16_t *>(out), lengths);
    return launch_failed("res_wide_gather_pages_kernel");
}

}  // extern "C"
