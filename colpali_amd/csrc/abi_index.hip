// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the first-stage indexes -- fixed dimensional encodings, the int8
// token-level index, the 1-bit sign index and the centroid-code index -- and the residual-compressed corpus built on the centroid
// codes, with the fused append-encode of its live form.
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates,
// frees or synchronises, so every entry point is hipGraph-capturable.  The kernels included below are defined and launched in
// this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "fde.hip"
#include "int8_index.hip"
#include "binary_index.hip"
#include "centroid_index.hip"
#include "residual_codec.hip"
#include "residual_scan.hip"
#include "residual_live.hip"
#include "residual_align.hip"

using namespace msim_abi;

// ---------------------------------------------------------------- fixed dimensional encodings (fde.hip)
namespace {

// the encoding's configuration: what the kernels implement, or MSIM_EUNSUPPORTED / MSIM_EINVAL
int fde_check_config(const char *who, int dtype, int dim, int reps, int ksim, int dproj, long long *F_out) {
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != msim::kDim)
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 embeddings of width %d (dtype code %d, dim %d)", who, msim::kDim,
                    dtype, dim);
    if (reps < 1) return fail(MSIM_EINVAL, "%s: reps=%d < 1", who, reps);
    if (ksim < 1 || ksim > msim::kFdeMaxKsim) return fail(MSIM_EUNSUPPORTED, "%s: k_sim=%d outside 1..%d", who, ksim, msim::kFdeMaxKsim);
    if (!(dproj == 8 || dproj == 16 || dproj == 32 || dproj == 64))
        return fail(MSIM_EUNSUPPORTED, "%s: d_proj=%d is not 8, 16, 32 or 64", who, dproj);
    const long long F = (long long)reps * (1LL << ksim) * dproj;
    if (F % 256 != 0 || F > 65536)
        return fail(MSIM_EUNSUPPORTED, "%s: F = reps x 2^k_sim x d_proj = %lld must be a multiple of 256 and at most 65536", who, F);
    *F_out = F;
    return MSIM_OK;
}

int fde_encode(const char *who, int dtype, const void *X, const int32_t *off, int n, int64_t n_rows, int dim, const float *G,
               const float *S, int reps, int ksim, int dproj, int is_doc, int fill_empty, void *out, uint8_t *codes, void *stream) {
    if (n < 0 || n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (n=%d rows=%lld)", who, n, (long long)n_rows);
    long long F = 0;
    if (int rc = fde_check_config(who, dtype, dim, reps, ksim, dproj, &F)) return rc;
    if (n == 0) return MSIM_OK;
    if ((!X && n_rows > 0) || !off || !G || !S || !out) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(out) & 1))
        return fail(MSIM_EINVAL, "%s: the rows must be 16-byte aligned and the output 2-byte aligned", who);
    if (fill_empty != 0 && fill_empty != 1) return fail(MSIM_EINVAL, "%s: fill_empty=%d is not 0 or 1", who, fill_empty);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = f16 ? msim::fde_encode_kernel<true> : msim::fde_encode_kernel<false>;
    static std::atomic<int> configured_bf16[kMaxDevices], configured_f16[kMaxDevices];
    constexpr int kMaxLds = msim::fde_encode_lds_bytes(msim::kFdeMaxKsim, 64);
    if (int rc = allow_lds(kern, kMaxLds, f16 ? configured_f16 : configured_bf16)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kern, dim3((unsigned)n), dim3(256), msim::fde_encode_lds_bytes(ksim, dproj), st, static_cast<const uint16_t *>(X),
                       off, n, (long long)n_rows, G, S, reps, ksim, dproj, is_doc, fill_empty, static_cast<uint16_t *>(out), codes);
    return launch_failed("fde_encode_kernel");
}

template <int QB, int DB, int NBUF>
int fde_scores_launch(bool f16, const void *Fq, int n_q, const void *Fd, int n_d, int F, float *scores, int64_t ld, hipStream_t st) {
    auto kern = f16 ? msim::fde_scores_kernel<QB, DB, NBUF, true> : msim::fde_scores_kernel<QB, DB, NBUF, false>;
    constexpr int lds = msim::fde_scores_lds_bytes<QB, DB, NBUF>();
    static std::atomic<int> configured_bf16[kMaxDevices], configured_f16[kMaxDevices];
    if (int rc = allow_lds(kern, lds, f16 ? configured_f16 : configured_bf16)) return rc;
    const long long n_qt = (n_q + QB - 1) / QB, n_dt = ((long long)n_d + DB - 1) / DB;
    if (n_qt * n_dt > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "msim_fde_scores: %lld tiles exceed one launch", n_qt * n_dt);
    const int vec = (reinterpret_cast<uintptr_t>(scores) & 15) == 0 && (ld & 3) == 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n_qt * n_dt)), dim3(256), lds, st, static_cast<const uint16_t *>(Fq), n_q,
                       static_cast<const uint16_t *>(Fd), n_d, F, scores, (long long)ld, (int)n_qt, vec);
    return launch_failed("fde_scores_kernel");
}

}  // namespace

extern "C" {

int msim_fde_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, const float *G, const float *S,
                         int reps, int ksim, int dproj, int fill_empty, void *out, uint8_t *codes, void *stream) {
    return fde_encode("msim_fde_encode_docs", dtype, D, d_off, n_d, n_rows, dim, G, S, reps, ksim, dproj, 1, fill_empty, out, codes,
                      stream);
}

int msim_fde_encode_queries(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t n_rows, int dim, const float *G,
                            const float *S, int reps, int ksim, int dproj, void *out, uint8_t *codes, void *stream) {
    return fde_encode("msim_fde_encode_queries", dtype, Qt, q_off, n_q, n_rows, dim, G, S, reps, ksim, dproj, 0, 0, out, codes, stream);
}

int msim_fde_scores(int dtype, const void *Fq, int n_q, const void *Fd, int n_d, int F, float *scores, int64_t ld_scores, void *stream) {
    if (n_q < 0 || n_d < 0 || F < 0) return fail(MSIM_EINVAL, "msim_fde_scores: negative size (n_q=%d n_d=%d F=%d)", n_q, n_d, F);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "msim_fde_scores takes bfloat16 / float16 encodings (dtype code %d)", dtype);
    if (F % 256 != 0 || F == 0 || F > 65536)
        return fail(MSIM_EUNSUPPORTED, "msim_fde_scores: F=%d must be a positive multiple of 256, at most 65536", F);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!Fq || !Fd || !scores) return fail(MSIM_EINVAL, "msim_fde_scores: null pointer argument");
    if ((reinterpret_cast<uintptr_t>(Fq) | reinterpret_cast<uintptr_t>(Fd)) & 15)
        return fail(MSIM_EINVAL, "msim_fde_scores: Fq and Fd must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(scores) & 3)) return fail(MSIM_EINVAL, "msim_fde_scores: scores must be 4-byte aligned");
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "msim_fde_scores: ld_scores=%lld < n_d=%d", (long long)ld_scores, n_d);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool f16 = dtype == MSIM_DTYPE_F16;
    // a few queries: a narrow query tile and a 4-deep ring (HBM-bound: Fd streams once); many: 128 x 128 tiles (MFMA-bound)
    if (n_q <= 64) return fde_scores_launch<32, 128, 4>(f16, Fq, n_q, Fd, n_d, F, scores, ld_scores, st);
    return fde_scores_launch<128, 128, 2>(f16, Fq, n_q, Fd, n_d, F, scores, ld_scores, st);
}

}  // extern "C"

// ---------------------------------------------------------------- the int8 token-level index (int8_index.hip)
namespace {

int i8_check_rows(const char *who, int dtype, int dim) {
    if (dim != msim::kDim) return fail(MSIM_EINVAL, "%s: rows of width %d; the int8 index takes width %d", who, dim, msim::kDim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    return MSIM_OK;
}

template <int NT, int GW, int D>
int i8_scores_launch(const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows, int QG, int TPQ, int passes,
                     const int8_t *d8, const float *sd, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int ppw,
                     int n_groups, float *scores, int64_t ld, hipStream_t st) {
    const long long n_gb = (n_groups + GW - 1) / GW;
    const long long n_ranges = ((long long)n_d + ppw - 1) / ppw, n_pb = (n_ranges + 4 / GW - 1) / (4 / GW);
    if (n_gb * n_pb > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "msim_i8_scores: %lld workgroups exceed one launch", n_gb * n_pb);
    hipLaunchKernelGGL((msim::i8_scores_kernel<NT, GW, D>), dim3((unsigned)(n_gb * n_pb)), dim3(256), 0, st, q8, sq, q_off, n_q,
                       (long long)q_rows, QG, TPQ, passes, d8, sd, d_off, clamp0, n_d, (long long)d_rows, ppw, n_groups, (int)n_gb,
                       scores, (long long)ld);
    return launch_failed("i8_scores_kernel");
}

}  // namespace

extern "C" {

int msim_i8_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int8_t *codes, float *scales,
                        void *stream) {
    const char *who = "msim_i8_encode_docs";
    if (n_d < 0 || n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (n_d=%d rows=%lld)", who, n_d, (long long)n_rows);
    if (int rc = i8_check_rows(who, dtype, dim)) return rc;
    if (n_d == 0) return MSIM_OK;
    if ((!D && n_rows > 0) || !d_off || (!codes && n_rows > 0) || !scales) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(codes, 16) || misaligned(d_off, 4) || misaligned(scales, 4))
        return fail(MSIM_EINVAL, "%s: rows and codes must be 16-byte aligned, offsets and scales 4-byte aligned", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::i8_encode_docs_kernel<true> : msim::i8_encode_docs_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_d), dim3(256), 0, st, static_cast<const uint16_t *>(D), d_off, n_d, (long long)n_rows, codes,
                       scales);
    return launch_failed("i8_encode_docs_kernel");
}

int msim_i8_encode_queries(int dtype, const void *Qt, int64_t n_rows, int dim, int8_t *codes, float *scales, void *stream) {
    const char *who = "msim_i8_encode_queries";
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (int rc = i8_check_rows(who, dtype, dim)) return rc;
    if (n_rows == 0) return MSIM_OK;
    if (!Qt || !codes || !scales) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(codes, 16) || misaligned(scales, 4))
        return fail(MSIM_EINVAL, "%s: rows and codes must be 16-byte aligned, scales 4-byte aligned", who);
    if ((n_rows + 15) / 16 > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::i8_encode_rows_kernel<true> : msim::i8_encode_rows_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, st, static_cast<const uint16_t *>(Qt), (long long)n_rows,
                       codes, scales);
    return launch_failed("i8_encode_rows_kernel");
}

int msim_i8_scores(const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, const int8_t *d8,
                   const float *sd, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim, float *scores,
                   int64_t ld_scores, void *stream) {
    const char *who = "msim_i8_scores";
    if (n_q < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, n_q, n_d,
                    (long long)q_rows, (long long)d_rows, max_q_tokens);
    if (dim != msim::kDim) return fail(MSIM_EINVAL, "%s: rows of width %d; the int8 index takes width %d", who, dim, msim::kDim);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if ((!q8 && q_rows > 0) || (!sq && q_rows > 0) || !q_off || (!d8 && d_rows > 0) || !sd || !d_off || !scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q8, 16) || misaligned(d8, 16) || misaligned(sq, 4) || misaligned(sd, 4) || misaligned(q_off, 4) ||
        misaligned(d_off, 4) || misaligned(scores, 4))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; scales, offsets and scores 4-byte aligned", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (max_q_tokens > (1 << 20)) return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, 1 << 20);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // the query plan: every query gets TPQ 16-token tiles, QG queries fill one wave's NT tiles; a longer query takes several passes
    constexpr int NT = 8;
    const int tiles = max_q_tokens ? (max_q_tokens + msim::kI8Tile - 1) / msim::kI8Tile : 1;
    int QG = 1, TPQ = NT, passes = 1;
    if (tiles <= NT) {
        TPQ = tiles;
        QG = NT / tiles;
    } else {
        passes = (tiles + NT - 1) / NT;
    }
    const long long n_groups = ((long long)n_q + QG - 1) / QG;
    // page ranges: enough waves to fill the chip (8 per CU, ~4 rounds); at most 16 pages a range when several query groups re-read it
    const long long want = (long long)di->cus * 32;
    const long long work = n_groups * n_d;
    const int cap = n_groups == 1 ? msim::kI8MaxRange : 16;
    long long ppw = (work + want - 1) / want;
    ppw = ppw < 1 ? 1 : ppw > cap ? cap : ppw;
    if (n_groups == 1)
        return i8_scores_launch<NT, 1, 4>(q8, sq, q_off, n_q, q_rows, QG, TPQ, passes, d8, sd, d_off, clamp0, n_d, d_rows, (int)ppw, 1,
                                          scores, ld_scores, st);
    if (n_groups == 2)
        return i8_scores_launch<NT, 2, 4>(q8, sq, q_off, n_q, q_rows, QG, TPQ, passes, d8, sd, d_off, clamp0, n_d, d_rows, (int)ppw, 2,
                                          scores, ld_scores, st);
    return i8_scores_launch<NT, 4, 4>(q8, sq, q_off, n_q, q_rows, QG, TPQ, passes, d8, sd, d_off, clamp0, n_d, d_rows, (int)ppw,
                                      (int)n_groups, scores, ld_scores, st);
}

}  // extern "C"

// ---------------------------------------------------------------- the 1-bit sign index (binary_index.hip)
namespace {

// the launch form of a shape: the int8 scorer's query plan (every query gets TPQ 16-token tiles, QG queries fill one wave's NT
// tiles, a longer query takes several passes) and GW = the waves that share a page range
struct BinPlan {
    static constexpr int NT = 8, D = 4;
    int QG, TPQ, passes, GW, ppw;
    long long n_groups;
};

BinPlan bin_plan(int n_q, int max_q_tokens, int n_d, int cus) {
    BinPlan p;
    const int tiles = max_q_tokens ? (max_q_tokens + msim::kI8Tile - 1) / msim::kI8Tile : 1;
    p.QG = 1, p.TPQ = BinPlan::NT, p.passes = 1;
    if (tiles <= BinPlan::NT) {
        p.TPQ = tiles;
        p.QG = BinPlan::NT / tiles;
    } else {
        p.passes = (tiles + BinPlan::NT - 1) / BinPlan::NT;
    }
    p.n_groups = ((long long)n_q + p.QG - 1) / p.QG;
    p.GW = p.n_groups <= 1 ? 1 : p.n_groups == 2 ? 2 : 4;
    // page ranges: enough waves to fill the chip (8 per CU, ~4 rounds); at most 16 pages a range when several query groups re-read it
    const long long want = (long long)(cus > 0 ? cus : 1) * 32;
    const long long work = p.n_groups * n_d;
    const int cap = p.n_groups <= 1 ? msim::kI8MaxRange : 16;
    long long ppw = (work + want - 1) / want;
    p.ppw = (int)(ppw < 1 ? 1 : ppw > cap ? cap : ppw);
    return p;
}

template <int GW>
int bin_scores_launch(const BinPlan &p, const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows,
                      const uint8_t *codes, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, float *scores,
                      int64_t ld, hipStream_t st) {
    const long long n_gb = (p.n_groups + GW - 1) / GW;
    const long long n_ranges = ((long long)n_d + p.ppw - 1) / p.ppw, n_pb = (n_ranges + 4 / GW - 1) / (4 / GW);
    if (n_gb * n_pb > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "msim_bin_scores: %lld workgroups exceed one launch", n_gb * n_pb);
    hipLaunchKernelGGL((msim::bin_scores_kernel<BinPlan::NT, GW, BinPlan::D>), dim3((unsigned)(n_gb * n_pb)), dim3(256), 0, st, q8, sq,
                       q_off, n_q, (long long)q_rows, p.QG, p.TPQ, p.passes, codes, d_off, clamp0, n_d, (long long)d_rows, p.ppw,
                       (int)p.n_groups, (int)n_gb, scores, (long long)ld);
    return launch_failed("bin_scores_kernel");
}

}  // namespace

extern "C" {

int msim_bin_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes, void *stream) {
    const char *who = "msim_bin_encode_rows";
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (dim != msim::kDim) return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the sign index takes width %d", who, dim, msim::kDim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    if (n_rows == 0) return MSIM_OK;
    if (!X || !codes) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(X, 16) || misaligned(codes, 16)) return fail(MSIM_EINVAL, "%s: rows and codes must be 16-byte aligned", who);
    if ((n_rows + 15) / 16 > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::bin_encode_rows_kernel<true> : msim::bin_encode_rows_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, st, static_cast<const uint16_t *>(X), (long long)n_rows,
                       codes);
    return launch_failed("bin_encode_rows_kernel");
}

int msim_bin_scores_plan(int n_q, int max_q_tokens, int n_d, int64_t d_rows, int32_t *plan) {
    const char *who = "msim_bin_scores_plan";
    if (n_q < 0 || n_d < 0 || d_rows < 0 || max_q_tokens < 0 || max_q_tokens > (1 << 20) || !plan)
        return fail(MSIM_EINVAL, "%s: bad argument", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const BinPlan p = bin_plan(n_q, max_q_tokens, n_d, di->cus);
    plan[0] = BinPlan::NT;
    plan[1] = p.GW;
    plan[2] = BinPlan::D;
    plan[3] = p.ppw;
    return MSIM_OK;
}

int msim_bin_scores(const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                    const uint8_t *codes, const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, int dim, float *scores,
                    int64_t ld_scores, void *stream) {
    const char *who = "msim_bin_scores";
    if (n_q < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, n_q, n_d,
                    (long long)q_rows, (long long)d_rows, max_q_tokens);
    if (dim != msim::kDim) return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the sign index takes width %d", who, dim, msim::kDim);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if ((!q8 && q_rows > 0) || (!sq && q_rows > 0) || !q_off || (!codes && d_rows > 0) || !d_off || !scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q8, 16) || misaligned(codes, 16) || misaligned(sq, 4) || misaligned(q_off, 4) || misaligned(d_off, 4) ||
        misaligned(scores, 4))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; scales, offsets and scores 4-byte aligned", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (max_q_tokens > (1 << 20)) return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, 1 << 20);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BinPlan p = bin_plan(n_q, max_q_tokens, n_d, di->cus);
    if (p.GW == 1) return bin_scores_launch<1>(p, q8, sq, q_off, n_q, q_rows, codes, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
    if (p.GW == 2) return bin_scores_launch<2>(p, q8, sq, q_off, n_q, q_rows, codes, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
    return bin_scores_launch<4>(p, q8, sq, q_off, n_q, q_rows, codes, d_off, clamp0, n_d, d_rows, scores, ld_scores, st);
}

}  // extern "C"

// ---------------------------------------------------------------- the centroid-code index (centroid_index.hip)
namespace {

int cent_check_format(const char *who, int dtype, int dim, int K) {
    if (dim != msim::kDim) return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; the centroid index takes width %d", who, dim, msim::kDim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    if (K < msim::kCentMinK || K > msim::kCentMaxK || K % 256 != 0)
        return fail(MSIM_EINVAL, "%s: %d centroids; the count is a multiple of 256 from %d to %d", who, K, msim::kCentMinK, msim::kCentMaxK);
    return MSIM_OK;
}

int cent_blocks(int max_q_tokens) {
    return max_q_tokens > 0 ? (max_q_tokens + msim::kCentBlockTok - 1) / msim::kCentBlockTok : 1;
}

struct CentPlan {
    int nb, ppw, n_pr;
    long long wgs;
};

// pages per wave: enough rows behind every table load (K x 64 B per workgroup and block) that the load is a small part of the
// workgroup's LDS traffic (16 K rows = 16 x the table), but never so many that the chip has fewer than 2 workgroups per CU to run
CentPlan cent_plan(int n_q, int max_q_tokens, int K, int n_d, int64_t d_rows, int cus) {
    CentPlan p;
    p.nb = cent_blocks(max_q_tokens);
    const long long avg = n_d > 0 && d_rows / n_d > 0 ? d_rows / n_d : 1;
    const long long amort = (2LL * K + avg - 1) / avg;
    const long long fill = (long long)n_q * n_d / ((long long)msim::kCentWaves * 2 * (cus > 0 ? cus : 1));
    long long ppw = amort < fill ? amort : fill;
    ppw = ppw < 1 ? 1 : ppw > msim::kCentMaxPpw ? msim::kCentMaxPpw : ppw;
    p.ppw = (int)ppw;
    const long long per_wg = ppw * msim::kCentWaves;
    p.n_pr = (int)((n_d + per_wg - 1) / per_wg);
    p.wgs = (long long)p.n_pr * n_q;
    return p;
}

}  // namespace

extern "C" {

int msim_cent_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows,
                          const void *C, int K, uint16_t *codes, int32_t *status, void *stream) {
    const char *who = "msim_cent_encode_docs";
    if (n_d < 0 || n_rows < 0 || max_doc_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_d=%d rows=%lld max_doc_rows=%d)", who, n_d, (long long)n_rows, max_doc_rows);
    if (int rc = cent_check_format(who, dtype, dim, K)) return rc;
    if (n_d == 0 || max_doc_rows == 0) return MSIM_OK;
    if ((!D && n_rows > 0) || !d_off || !C || (!codes && n_rows > 0)) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(C, 16) || misaligned(codes, 16) || misaligned(d_off, 4) || misaligned(status, 4))
        return fail(MSIM_EINVAL, "%s: rows, centroids and codes must be 16-byte aligned, offsets and status 4-byte aligned", who);
    const long long gy = ((long long)max_doc_rows + msim::kCentEncRows - 1) / msim::kCentEncRows;
    if (gy > 65535) return fail(MSIM_EUNSUPPORTED, "%s: max_doc_rows=%d above %d", who, max_doc_rows, 65535 * msim::kCentEncRows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::cent_encode_kernel<true> : msim::cent_encode_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_d, (unsigned)gy), dim3(256), 0, st, static_cast<const uint16_t *>(D), d_off, n_d,
                       (long long)n_rows, max_doc_rows, static_cast<const uint16_t *>(C), K, codes, status);
    return launch_failed("cent_encode_kernel");
}

size_t msim_cent_table_bytes(int n_q, int max_q_tokens, int K) {
    if (n_q <= 0 || K <= 0 || max_q_tokens < 0) return 0;
    return (size_t)n_q * cent_blocks(max_q_tokens) * K * msim::kCentTableRow;
}

int msim_cent_table(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int dim,
                    const void *C, int K, void *table, void *stream) {
    const char *who = "msim_cent_table";
    if (n_q < 0 || q_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d q_rows=%lld max_q_tokens=%d)", who, n_q, (long long)q_rows, max_q_tokens);
    if (int rc = cent_check_format(who, dtype, dim, K)) return rc;
    if (max_q_tokens > msim::kCentMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, msim::kCentMaxTokens);
    if (n_q == 0) return MSIM_OK;
    if ((!Qt && q_rows > 0) || !q_off || !C || !table) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(table, 16) || misaligned(q_off, 4))
        return fail(MSIM_EINVAL, "%s: tokens, centroids and table must be 16-byte aligned, offsets 4-byte aligned", who);
    const int nb = cent_blocks(max_q_tokens);
    if ((long long)n_q * nb > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld blocks exceed one launch", who, (long long)n_q * nb);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto kern = dtype == MSIM_DTYPE_F16 ? msim::cent_table_kernel<true> : msim::cent_table_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)(n_q * nb), (unsigned)(K / 256)), dim3(256), 0, st, static_cast<const uint16_t *>(Qt), q_off,
                       n_q, (long long)q_rows, nb, static_cast<const uint16_t *>(C), K, static_cast<_Float16 *>(table));
    return launch_failed("cent_table_kernel");
}

int msim_cent_scores_plan(int n_q, int max_q_tokens, int K, int n_d, int64_t d_rows, int32_t *plan) {
    const char *who = "msim_cent_scores_plan";
    if (n_q < 0 || n_d < 0 || d_rows < 0 || max_q_tokens < 0 || !plan) return fail(MSIM_EINVAL, "%s: bad argument", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const CentPlan p = cent_plan(n_q, max_q_tokens, K, n_d, d_rows, di->cus);
    plan[0] = p.nb;
    plan[1] = p.ppw;
    plan[2] = msim::kCentWaves;
    plan[3] = (int32_t)(p.wgs > 0x7fffffffLL ? 0x7fffffffLL : p.wgs);
    return MSIM_OK;
}

int msim_cent_scores(const void *table, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int K, const uint16_t *codes,
                     const int32_t *d_off, const uint8_t *clamp0, int n_d, int64_t d_rows, float *scores, int64_t ld_scores,
                     void *stream) {
    const char *who = "msim_cent_scores";
    if (n_q < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, n_q, n_d,
                    (long long)q_rows, (long long)d_rows, max_q_tokens);
    if (int rc = cent_check_format(who, MSIM_DTYPE_BF16, msim::kDim, K)) return rc;
    if (max_q_tokens > msim::kCentMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, msim::kCentMaxTokens);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!table || !q_off || (!codes && d_rows > 0) || !d_off || !scores) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(table, 16) || misaligned(codes, 16) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(scores, 4))
        return fail(MSIM_EINVAL, "%s: table and codes must be 16-byte aligned; offsets and scores 4-byte aligned", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (d_rows > 0x7fffffffLL - 1024) return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld exceeds 32-bit row indices", who, (long long)d_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const CentPlan p = cent_plan(n_q, max_q_tokens, K, n_d, d_rows, di->cus);
    if (p.wgs > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld workgroups exceed one launch", who, p.wgs);
    constexpr int park = msim::kCentWaves * msim::kCentBatch * msim::kCentTableRow;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(msim::cent_scores_kernel, msim::kCentMaxK * msim::kCentTableRow + park, configured)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(msim::cent_scores_kernel, dim3((unsigned)p.wgs), dim3(msim::kCentWaves * 64), K * msim::kCentTableRow + park, st,
                       static_cast<const _Float16 *>(table), q_off, n_q, (long long)q_rows, p.nb, K, codes, d_off, clamp0, n_d,
                       (long long)d_rows, p.ppw, p.n_pr, scores, (long long)ld_scores);
    return launch_failed("cent_scores_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- the residual-compressed corpus (residual_codec.hip)
namespace {

int res_check_format(const char *who, int dtype, int dim, int K, int bits) {
    if (int rc = cent_check_format(who, dtype, dim, K)) return rc;
    if (!(bits == 2 || bits == 4)) return fail(MSIM_EUNSUPPORTED, "%s: %d residual bits; the codec stores 2 or 4 per dimension", who, bits);
    return MSIM_OK;
}

// rows out of the compressed shard (residual_align.hip): K outside the centroid index's range is a format the kernels do not have
int res_rows_check_format(const char *who, int dtype, int dim, int K, int bits) {
    if (K < msim::kCentMinK || K > msim::kCentMaxK || K % 256 != 0)
        return fail(MSIM_EUNSUPPORTED, "%s: %d centroids; the count is a multiple of 256 from %d to %d", who, K, msim::kCentMinK,
                    msim::kCentMaxK);
    return res_check_format(who, dtype, dim, K, bits);
}

}  // namespace

extern "C" {

int msim_res_encode_docs(int dtype, const void *D, int64_t n_rows, int dim, const uint16_t *codes, const void *C, int K,
                         const float *cutoffs, int bits, uint8_t *residuals, void *stream) {
    const char *who = "msim_res_encode_docs";
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (int rc = res_check_format(who, dtype, dim, K, bits)) return rc;
    if (n_rows == 0) return MSIM_OK;
    if (!D || !codes || !C || !cutoffs || !residuals) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(codes, 2) || misaligned(cutoffs, 4))
        return fail(MSIM_EINVAL, "%s: rows, centroids and residuals must be 16-byte aligned, codes 2-byte and cutoffs 4-byte aligned", who);
    const long long blocks = (n_rows * msim::kResChunks + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_encode_kernel<true, 2> : msim::res_encode_kernel<false, 2>)
                          : (f16 ? msim::res_encode_kernel<true, 4> : msim::res_encode_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const uint16_t *>(D), codes,
                       (long long)n_rows, static_cast<const uint16_t *>(C), K, cutoffs, residuals);
    return launch_failed("res_encode_kernel");
}

int msim_res_decode_rows(int dtype, const uint16_t *codes, const uint8_t *residuals, int64_t n_rows, int64_t row0, int64_t row1,
                         const void *C, int K, const float *weights, int bits, int dim, void *out, void *stream) {
    const char *who = "msim_res_decode_rows";
    if (n_rows < 0 || row0 < 0 || row1 < row0 || row1 > n_rows)
        return fail(MSIM_EINVAL, "%s: rows %lld .. %lld of %lld", who, (long long)row0, (long long)row1, (long long)n_rows);
    if (int rc = res_check_format(who, dtype, dim, K, bits)) return rc;
    if (row1 == row0) return MSIM_OK;
    if (!codes || !residuals || !C || !weights || !out) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(out, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(codes, 2) || misaligned(weights, 4))
        return fail(MSIM_EINVAL, "%s: out, centroids and residuals must be 16-byte aligned, codes 2-byte and weights 4-byte aligned", who);
    const long long blocks = ((row1 - row0) * msim::kResChunks + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)(row1 - row0));
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_decode_kernel<true, 2> : msim::res_decode_kernel<false, 2>)
                          : (f16 ? msim::res_decode_kernel<true, 4> : msim::res_decode_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), codes, residuals, (long long)row0,
                       (long long)row1, static_cast<const uint16_t *>(C), K, weights, static_cast<uint16_t *>(out));
    return launch_failed("res_decode_kernel");
}

// one wave scores one entry from the page's own rows: nothing is inverted, so the workspace is the status word alone
size_t msim_res_candidates_workspace_bytes(int n_q, int m, int n_d) {
    if (n_q <= 0 || m <= 0 || n_d < 0) return 0;
    return 16;
}

int msim_res_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                        const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                        const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand,
                        int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids, void *workspace, void *stream) {
    const char *who = "msim_res_candidates";
    if (n_q < 0 || m < 0 || n_d < 0 || d_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d n_d=%d d_rows=%lld)", who, n_q, m, n_d, (long long)d_rows);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (int rc = res_check_format(who, dtype, dim, K, bits)) return rc;
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
    hipLaunchKernelGGL(msim::res_zero_status_kernel, dim3(1), dim3(64), 0, st, status);
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_candidates_kernel<true, 2> : msim::res_candidates_kernel<false, 2>)
                          : (f16 ? msim::res_candidates_kernel<true, 4> : msim::res_candidates_kernel<false, 4>);
    // a persistent grid: one entry per wave at a time, as many workgroups per CU as the launch bounds keep resident (two)
    const long long wg_needed = (E + 3) / 4;
    const long long wg_cap = (long long)di->cus * 2;
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), msim::kResLdsBytes, st,
                       static_cast<const uint16_t *>(Qt), q_off, n_q, (long long)q_off_host[n_q], codes, residuals,
                       static_cast<const uint16_t *>(C), K, weights, d_off, d_clamp0, n_d, (long long)d_rows, cand, (long long)ld_cand, m,
                       (long long)id_base, out_scores, (long long)ld_scores, out_ids, status);
    hipLaunchKernelGGL(msim::res_poison_kernel, dim3(eblocks), dim3(256), 0, st, status, n_q, m, out_scores, (long long)ld_scores);
    return launch_failed("res_candidates_kernel");
}

// K1a's contract over the compressed rows: every wave decodes the chunks it multiplies, nothing is staged or allocated
int msim_res_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                              const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights, int bits,
                              const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, const int64_t *cand, int m,
                              int64_t ld_cand, int64_t id_base, float *best_sim, int32_t *best_row, float *sims, int max_rows,
                              void *stream) {
    const char *who = "msim_res_align_candidates";
    if (n_q < 0 || m < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0 || max_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d max_rows=%d)", who, n_q,
                    m, n_d, (long long)q_rows, (long long)d_rows, max_q_tokens, max_rows);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (int rc = res_rows_check_format(who, dtype, dim, K, bits)) return rc;
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
    auto kern = bits == 2 ? (f16 ? msim::res_align_kernel<true, 2> : msim::res_align_kernel<false, 2>)
                          : (f16 ? msim::res_align_kernel<true, 4> : msim::res_align_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)n_q * m)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(Qt), q_off, codes, residuals, static_cast<const uint16_t *>(C), K, weights, d_off,
                       d_clamp0, cand, best_sim, best_row, sims, a);
    return launch_failed("res_align_kernel");
}

// msim_gather_pages' contract over the compressed rows: the box is decoded into, never copied from a decoded page
int msim_res_gather_pages(int dtype, const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights,
                          int bits, int dim, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base, const int64_t *ids,
                          int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream) {
    const char *who = "msim_res_gather_pages";
    if (n_slots < 0 || n_d < 0 || d_rows < 0 || pad_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_slots=%lld n_d=%d d_rows=%lld pad_rows=%lld)", who, (long long)n_slots, n_d,
                    (long long)d_rows, (long long)pad_rows);
    if (n_slots == 0) return MSIM_OK;
    if (int rc = res_rows_check_format(who, dtype, dim, K, bits)) return rc;
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
    auto kern = bits == 2 ? (f16 ? msim::res_gather_pages_kernel<true, 2> : msim::res_gather_pages_kernel<false, 2>)
                          : (f16 ? msim::res_gather_pages_kernel<true, 4> : msim::res_gather_pages_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_slots), dim3(256), 0, static_cast<hipStream_t>(stream), codes, residuals,
                       static_cast<const uint16_t *>(C), K, weights, (long long)d_rows, d_off, n_d, (long long)id_base, ids,
                       (long long)pad_rows, static_cast<uint16_t *>(out), lengths);
    return launch_failed("res_gather_pages_kernel");
}

// the full scan: the status words plus one 16-byte group per query at most -- a function of n_q alone, never of the row count
size_t msim_res_scores_workspace_bytes(int n_q, int n_d) {
    if (n_q <= 0 || n_d <= 0) return 0;
    return align16(msim::kResScanStatusBytes + (size_t)n_q * sizeof(msim::ResScanGroup));
}

int msim_res_scores(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                    const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                    const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, float *out_scores, int64_t ld_scores, void *workspace,
                    void *stream) {
    const char *who = "msim_res_scores";
    if (n_q < 0 || n_d < 0 || d_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d d_rows=%lld)", who, n_q, n_d, (long long)d_rows);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (int rc = res_check_format(who, dtype, dim, K, bits)) return rc;
    if (!Qt || !q_off || !q_off_host || ((!codes || !residuals) && d_rows > 0) || !C || !weights || !d_off || !out_scores || !workspace)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(C, 16) || misaligned(residuals, 16) || misaligned(workspace, 16) || misaligned(codes, 2) ||
        misaligned(weights, 4) || misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(out_scores, 4))
        return fail(MSIM_EINVAL, "%s: Qt, centroids, residuals and workspace must be 16-byte aligned; the rest by their element size", who);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, n_d);
    if (d_rows > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld exceeds 32-bit page offsets", who, (long long)d_rows);
    if (q_off_host[0] != 0) return fail(MSIM_EINVAL, "%s: q_off[0] must be 0", who);
    // the checks of the offsets and, by the rule the device applies to its own copy (residual_scan.hip), the number of query groups
    const int cap_units = std::min(std::max(ab_env("MSIM_RES_SCAN_UNITS", msim::kResScanGroupUnits), 1), msim::kStreamMaxUnits);
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
    hipLaunchKernelGGL(msim::res_scan_groups_kernel, dim3(1), dim3(64), 0, st, q_off, n_q, q_rows, cap_units, n_groups, groups, status);
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_scan_kernel<true, 2> : msim::res_scan_kernel<false, 2>)
                          : (f16 ? msim::res_scan_kernel<true, 4> : msim::res_scan_kernel<false, 4>);
    // a persistent grid: every wave walks pages of its own, as many workgroups per CU as the launch bounds keep resident (two)
    const long long wg_needed = ((long long)n_d + 3) / 4;
    const long long wg_cap = (long long)di->cus * 2;
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), msim::kResLdsBytes, st,
                       static_cast<const uint16_t *>(Qt), q_off, n_q, q_rows, codes, residuals, static_cast<const uint16_t *>(C), K, weights,
                       d_off, d_clamp0, n_d, (long long)d_rows, out_scores, (long long)ld_scores, groups, n_groups, status);
    const long long pblocks = ((long long)n_q * n_d + 255) / 256;
    hipLaunchKernelGGL(msim::res_scan_poison_kernel, dim3((unsigned)(pblocks < wg_cap * 4 ? pblocks : wg_cap * 4)), dim3(256), 0, st, status,
                       n_q, n_d, out_scores, (long long)ld_scores);
    return launch_failed("res_scan_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- the live compressed shard: fused append-encode (residual_live.hip)
extern "C" {

int msim_res_append(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows, const void *C,
                    int K, const float *cutoffs, int bits, uint16_t *codes, uint8_t *residuals, int64_t dst_row0, int64_t dst_rows,
                    int32_t *status, void *stream) {
    const char *who = "msim_res_append";
    if (n_d < 0 || n_rows < 0 || max_doc_rows < 0 || dst_row0 < 0 || dst_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_d=%d rows=%lld max_doc_rows=%d dst_row0=%lld dst_rows=%lld)", who, n_d,
                    (long long)n_rows, max_doc_rows, (long long)dst_row0, (long long)dst_rows);
    if (dim != msim::kDim) return fail(MSIM_EINVAL, "%s: rows of width %d; the residual codec takes width %d", who, dim, msim::kDim);
    if (int rc = res_check_format(who, dtype, dim, K, bits)) return rc;
    if (n_rows > dst_rows - dst_row0)
        return fail(MSIM_EINVAL, "%s: rows %lld .. %lld do not fit the %lld destination rows", who, (long long)dst_row0,
                    (long long)(dst_row0 + n_rows), (long long)dst_rows);
    if (n_d == 0 || max_doc_rows == 0) return MSIM_OK;
    if ((!D && n_rows > 0) || !d_off || !C || !cutoffs || ((!codes || !residuals) && n_rows > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(D, 16) || misaligned(C, 16) || misaligned(codes, 16) || misaligned(residuals, 16) || misaligned(d_off, 4) ||
        misaligned(status, 4) || misaligned(cutoffs, 4))
        return fail(MSIM_EINVAL, "%s: rows, centroids, codes and residuals must be 16-byte aligned; offsets, status and cutoffs 4-byte aligned",
                    who);
    const long long gy = ((long long)max_doc_rows + msim::kCentEncRows - 1) / msim::kCentEncRows;
    if (gy > 65535) return fail(MSIM_EUNSUPPORTED, "%s: max_doc_rows=%d above %d", who, max_doc_rows, 65535 * msim::kCentEncRows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    auto kern = bits == 2 ? (f16 ? msim::res_append_kernel<true, 2> : msim::res_append_kernel<false, 2>)
                          : (f16 ? msim::res_append_kernel<true, 4> : msim::res_append_kernel<false, 4>);
    hipLaunchKernelGGL(kern, dim3((unsigned)n_d, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(D), d_off, n_d, (long long)n_rows, max_doc_rows, static_cast<const uint16_t *>(C), K,
                       cutoffs, codes, residuals, (long long)dst_row0, (long long)dst_rows, status);
    return launch_failed("res_append_kernel");
}

}  // extern "C"
