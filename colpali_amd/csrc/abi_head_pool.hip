// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the embedding head, hierarchical token pooling and the host gather helpers.
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates,
// frees or synchronises, so every entry point is hipGraph-capturable.  The kernels included below are defined and launched in
// this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "abi_shapes.hpp"
#include "embed_head.hip"
#include "token_pooling.hip"

using namespace msim_abi;

extern "C" {

// ---------------------------------------------------------------- embedding head (the producer of the corpus format)
int msim_embed_head_row_map(const void *mask, int mask_kind, const void *extra, int extra_kind, int64_t M, int32_t *row_map, void *stream) {
    if (M < 0) return fail(MSIM_EINVAL, "bad size (M=%lld)", (long long)M);
    if (M == 0) return MSIM_OK;
    if (!mask || !row_map) return fail(MSIM_EINVAL, "null pointer argument");
    if (mask_kind < 0 || mask_kind > 6 || (extra && (extra_kind < 0 || extra_kind > 6))) return fail(MSIM_EINVAL, "unknown mask kind");
    if (M > 0x7ffffffdLL) return fail(MSIM_EUNSUPPORTED, "too many rows for an int32 row map");
    const long long padded = (M + msim::kHeadBM - 1) / msim::kHeadBM * msim::kHeadBM;
    hipLaunchKernelGGL(msim::head_row_map_kernel, dim3((unsigned)((padded + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), mask,
                       mask_kind, extra, extra_kind, (long long)M, padded, row_map);
    return launch_failed("head_row_map_kernel");
}

int msim_embed_head_writer_map(const void *mask, int mask_kind, const void *extra, int extra_kind, int B, int S, const int64_t *rows_before,
                               int64_t *counts, int32_t *row_map, int64_t *rows_after, void *stream) {
    if (B < 0 || S <= 0) return fail(MSIM_EINVAL, "bad size (B=%d S=%d)", B, S);
    if (B == 0) return MSIM_OK;
    if (!mask || !rows_before || !counts || !row_map || !rows_after) return fail(MSIM_EINVAL, "null pointer argument");
    if (mask_kind < 0 || mask_kind > 6 || (extra && (extra_kind < 0 || extra_kind > 6))) return fail(MSIM_EINVAL, "unknown mask kind");
    const long long M = (long long)B * S;
    const long long padded = (M + msim::kHeadBM - 1) / msim::kHeadBM * msim::kHeadBM;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(msim::head_page_count_kernel, dim3(B), dim3(256), 0, st, mask, mask_kind, extra, extra_kind, S,
                       reinterpret_cast<long long *>(counts));
    hipLaunchKernelGGL(msim::head_writer_map_kernel, dim3(B + 1), dim3(256), 0, st, mask, mask_kind, extra, extra_kind, B, S,
                       reinterpret_cast<const long long *>(rows_before), reinterpret_cast<const long long *>(counts), padded, row_map,
                       reinterpret_cast<long long *>(rows_after));
    return launch_failed("head_writer_map_kernel");
}

int msim_embed_head_bwd(int dtype, const void *proj, const void *grad_out, const int32_t *row_map, int64_t M, int n_out,
                        void *dproj, void *stream) {
    if (M < 0) return fail(MSIM_EINVAL, "bad size (M=%lld)", (long long)M);
    if (M == 0) return MSIM_OK;
    if (!proj || !grad_out || !row_map || !dproj) return fail(MSIM_EINVAL, "null pointer argument");
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16)
        return fail(MSIM_EUNSUPPORTED, "dtype code %d: the embedding head takes bfloat16 (0) or float16 (1)", dtype);
    if (n_out != msim::kHeadN) return fail(MSIM_EUNSUPPORTED, "n_out=%d: the embedding head is built for 128 output columns", n_out);
    if ((reinterpret_cast<uintptr_t>(proj) | reinterpret_cast<uintptr_t>(grad_out) | reinterpret_cast<uintptr_t>(dproj)) & 15)
        return fail(MSIM_EINVAL, "proj, grad_out and dproj must be 16-byte aligned");
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const long long blocks = (M + 15) / 16;
    const int grid = (int)(blocks < (long long)di->cus * 16 ? blocks : (long long)di->cus * 16);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *p = static_cast<const uint16_t *>(proj), *g = static_cast<const uint16_t *>(grad_out);
    uint16_t *o = static_cast<uint16_t *>(dproj);
    if (dtype == MSIM_DTYPE_F16)
        hipLaunchKernelGGL(msim::embed_head_bwd_rows_kernel<true>, dim3(grid), dim3(256), 0, st, p, g, row_map, (long long)M, o);
    else
        hipLaunchKernelGGL(msim::embed_head_bwd_rows_kernel<false>, dim3(grid), dim3(256), 0, st, p, g, row_map, (long long)M, o);
    return launch_failed("embed_head_bwd_rows_kernel");
}

int msim_embed_head(int dtype, const void *X, int64_t M, int H, const void *W, const void *bias, int n_out,
                    const int32_t *row_map, void *out, int64_t ld_out, void *stream) {
    if (M < 0 || H <= 0) return fail(MSIM_EINVAL, "bad size (M=%lld H=%d)", (long long)M, H);
    if (M == 0) return MSIM_OK;
    if (!X || !W || !row_map || !out) return fail(MSIM_EINVAL, "null pointer argument");
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16)
        return fail(MSIM_EUNSUPPORTED, "dtype code %d: the embedding head takes bfloat16 (0) or float16 (1) hidden states", dtype);
    if (n_out != msim::kHeadN) return fail(MSIM_EUNSUPPORTED, "n_out=%d: the embedding head is built for 128 output columns", n_out);
    if (H % msim::kHeadBK != 0 || H > 16384) return fail(MSIM_EUNSUPPORTED, "H=%d: hidden size must be a multiple of 64, <= 16384", H);
    if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(W)) & 15) return fail(MSIM_EINVAL, "X and W must be 16-byte aligned");
    if (ld_out < msim::kHeadN) return fail(MSIM_EINVAL, "ld_out=%lld < 128", (long long)ld_out);
    if (M > (int64_t)0x7fffffff * 128) return fail(MSIM_EUNSUPPORTED, "too many rows");
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::HeadArgs a;
    a.M = M;
    a.H = H;
    a.ld_out = ld_out;
    a.trace = nullptr;
    a.stagger = ab_env("MSIM_HEAD_STAGGER", 0);
    a.stagger_sleep = ab_env("MSIM_HEAD_STAGGER_SLEEP", 1);
#ifdef MSIM_TRACE                                            // `make trace` only: device address of 9 x 8 uint64 (tools/trace_head.py)
    if (const char *tp = getenv("MSIM_HEAD_TRACE_PTR")) a.trace = reinterpret_cast<unsigned long long *>(strtoull(tp, nullptr, 0));
#endif
    const long long tiles = (M + msim::kHeadBM - 1) / msim::kHeadBM;
    const int grid = tiles < di->cus ? (int)tiles : di->cus;
    const long long tiles_h = (M + 127) / 128;                               // HALF variant: 128-row tiles, two workgroups per CU
    const int grid_h = tiles_h < 2 * di->cus ? (int)tiles_h : 2 * di->cus;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *x = static_cast<const uint16_t *>(X), *w = static_cast<const uint16_t *>(W), *b = static_cast<const uint16_t *>(bias);
    uint16_t *o = static_cast<uint16_t *>(out);
    auto go = [&](auto kern, std::atomic<int> *configured, int lds) -> int {
        if (int rc = allow_lds(kern, lds, configured)) return rc;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(msim::kHeadThreads), lds, st, x, w, b, row_map, o, a);
        return MSIM_OK;
    };
    auto go_half = [&](auto kern, std::atomic<int> *configured) -> int {
        constexpr int lds = 3 * 128 * 128 + 2 * msim::kHeadWBytes;             // 48 + 32 KiB
        if (int rc = allow_lds(kern, lds, configured)) return rc;
        hipLaunchKernelGGL(kern, dim3(grid_h), dim3(320), lds, st, x, w, b, row_map, o, a);
        return MSIM_OK;
    };
    int rc;
    const bool f16 = dtype == MSIM_DTYPE_F16;
    // Shipped: loader two weight chunks ahead (rings 3 + 3), output rows staged through LDS and stored as whole rows with the
    // streaming policy (needs 16-byte aligned output rows; the 2-byte-store form of the same kernel otherwise).  Every other
    // variant of embed_head_kernel was measured and not kept; they are compiled into measurement builds only
    // (preprocessor, not `if constexpr`: in a non-template function a discarded branch is still instantiated and code-generated).
#if !defined(MSIM_AB) && !defined(MSIM_TRACE)
    {
        const bool whole_rows = ld_out % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        static std::atomic<int> cfg[8][kMaxDevices];
        // hidden sizes above 4096: the same two forms with the accumulator folded every 1024 K (WIDE, embed_head.hip)
        if (H > 4096 && whole_rows)
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true, false, false, true, false, true>, cfg[4], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true, false, false, true, false, true>, cfg[5], msim::kHeadFLds);
        else if (H > 4096)
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true, false, false, false, false, true>, cfg[6], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true, false, false, false, false, true>, cfg[7], msim::kHeadFLds);
        else if (whole_rows)
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true, false, false, true>, cfg[0], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true, false, false, true>, cfg[1], msim::kHeadFLds);
        else
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true>, cfg[2], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true>, cfg[3], msim::kHeadFLds);
        (void)go_half;
    }
#else
    {
        static std::atomic<int> configured[12][kMaxDevices];
        // MSIM_HEAD_VARIANT = bit 0: flag-synchronised weight ring instead of one s_barrier per K chunk; bit 1: hand-pipelined operand
        // fetch; bit 2: swapped MFMA roles + per-row epilogue; bit 3 (default): loader two weight chunks ahead, rings 3 + 3; bit 4: two half-size workgroups per CU; bit 5: DMA pieces between the
        // MFMAs; bit 6 (default): whole-row output stores through LDS
        // (tuning knob for A/B measurements, not part of the ABI; profiles/r02_logs/ab_head_variants.log)
        static const int variant = ab_env("MSIM_HEAD_VARIANT", 72) & 127;
        const bool epi2 = (variant & 4) && ld_out % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0 &&
                          (bias == nullptr || (reinterpret_cast<uintptr_t>(bias) & 3) == 0);   // 8-byte stores, 4-byte bias loads
        // bit 3: loader two weight chunks ahead (rings 3 + 3)
        // bit 6 (default): output rows staged through LDS and stored as whole rows; needs 16-byte aligned rows, else the 2-byte form
        const bool epi3 = (variant & 64) && ld_out % 8 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
        static const int pair_env = ab_env("MSIM_HEAD_PAIR", 0);       // round 3: chunks requested two at a time (rings 4 + 2, whole-row stores)
        if (pair_env && epi3) {
            static std::atomic<int> configured6[2][kMaxDevices];
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, false, false, false, true, true>, configured6[0], msim::kHeadLds)
                     : go(msim::embed_head_kernel<false, false, false, false, false, false, false, true, true>, configured6[1], msim::kHeadLds);
        } else if (epi3) {
            static std::atomic<int> configured5[2][kMaxDevices];
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true, false, false, true>, configured5[0], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true, false, false, true>, configured5[1], msim::kHeadFLds);
        } else if (variant & 32) {           // bit 5: hidden-state DMA pieces issued between the k-steps' MFMAs (+ bit 3 rings, + bit 2 epilogue)
            static std::atomic<int> configured4[6][kMaxDevices];
            if ((variant & 8) && (variant & 4) && epi2)
                rc = f16 ? go(msim::embed_head_kernel<true, false, false, true, true, false, true>, configured4[0], msim::kHeadFLds)
                         : go(msim::embed_head_kernel<false, false, false, true, true, false, true>, configured4[1], msim::kHeadFLds);
            else if (variant & 8)
                rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true, false, true>, configured4[2], msim::kHeadFLds)
                         : go(msim::embed_head_kernel<false, false, false, false, true, false, true>, configured4[3], msim::kHeadFLds);
            else
                rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, false, false, true>, configured4[4], msim::kHeadLds)
                         : go(msim::embed_head_kernel<false, false, false, false, false, false, true>, configured4[5], msim::kHeadLds);
        } else if (variant & 16) {           // bit 4: two half-size workgroups per CU
            static std::atomic<int> configured3[2][kMaxDevices];
            rc = f16 ? go_half(msim::embed_head_kernel<true, false, false, false, false, true>, configured3[0])
                     : go_half(msim::embed_head_kernel<false, false, false, false, false, true>, configured3[1]);
        } else if ((variant & 8) && (variant & 4) && epi2) {
            static std::atomic<int> configured2[2][kMaxDevices];
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, true, true>, configured2[0], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, true, true>, configured2[1], msim::kHeadFLds);
        } else if (variant & 8) {
            rc = f16 ? go(msim::embed_head_kernel<true, false, false, false, true>, configured[10], msim::kHeadFLds)
                     : go(msim::embed_head_kernel<false, false, false, false, true>, configured[11], msim::kHeadFLds);
        } else
        switch (epi2 ? 4 : (variant & 3)) {
            case 1: rc = f16 ? go(msim::embed_head_kernel<true, true, false>, configured[0], msim::kHeadFLds)
                             : go(msim::embed_head_kernel<false, true, false>, configured[1], msim::kHeadFLds); break;
            case 2: rc = f16 ? go(msim::embed_head_kernel<true, false, true>, configured[2], msim::kHeadLds)
                             : go(msim::embed_head_kernel<false, false, true>, configured[3], msim::kHeadLds); break;
            case 3: rc = f16 ? go(msim::embed_head_kernel<true, true, true>, configured[4], msim::kHeadFLds)
                             : go(msim::embed_head_kernel<false, true, true>, configured[5], msim::kHeadFLds); break;
            case 4: rc = f16 ? go(msim::embed_head_kernel<true, false, false, true>, configured[8], msim::kHeadLds)
                             : go(msim::embed_head_kernel<false, false, false, true>, configured[9], msim::kHeadLds); break;
            default: rc = f16 ? go(msim::embed_head_kernel<true, false, false>, configured[6], msim::kHeadLds)
                              : go(msim::embed_head_kernel<false, false, false>, configured[7], msim::kHeadLds); break;
        }
    }
#endif
    if (rc) return rc;
    return launch_failed("embed_head_kernel");
}

// ---------------------------------------------------------------- hierarchical token pooling
int msim_pool_cluster(int dtype, const void *E, const int32_t *d_off, int n_pages, int dim, int max_rows,
                      const int64_t *ws_off, int pool_factor, float *X_ws, double *D_ws, int32_t *labels,
                      int32_t *n_clusters, void *stream) {
    if (n_pages < 0 || max_rows < 0) return fail(MSIM_EINVAL, "negative size");
    if (n_pages == 0) return MSIM_OK;
    if (!E || !d_off || !ws_off || !X_ws || !D_ws || !labels || !n_clusters) return fail(MSIM_EINVAL, "null pointer argument");
    if (pool_factor < 1) return fail(MSIM_EINVAL, "pool_factor must be >= 1");
    static const int32_t dummy_off[2] = {0, 0};
    if (int rc = check_smooth(E, E, dummy_off, dtype, dim, 1, 1.0f)) return rc;      // row layout contract of the generic kernels
    if (max_rows > msim::kPoolMaxRows) return fail(MSIM_EUNSUPPORTED, "a page of %d rows: at most %d are supported", max_rows, msim::kPoolMaxRows);
    if (n_pages > 65535) return fail(MSIM_EUNSUPPORTED, "at most 65535 pages per call");
    hipStream_t st = static_cast<hipStream_t>(stream);
    msim::PoolArgs a{n_pages, dim, dim * elem_bytes(dtype), pool_factor};
    const char *e = static_cast<const char *>(E);
    if (max_rows > 0) {
        const dim3 ggrid((max_rows + 127) / 128, (max_rows + 31) / 32, n_pages);
        switch (dtype) {
            case MSIM_DTYPE_F32: hipLaunchKernelGGL(msim::pool_gram_kernel<msim::kDtypeF32>, ggrid, dim3(256), 0, st, e, d_off, ws_off, X_ws, a); break;
            case MSIM_DTYPE_F16: hipLaunchKernelGGL(msim::pool_gram_kernel<msim::kDtypeF16>, ggrid, dim3(256), 0, st, e, d_off, ws_off, X_ws, a); break;
            default: hipLaunchKernelGGL(msim::pool_gram_kernel<msim::kDtypeBf16>, ggrid, dim3(256), 0, st, e, d_off, ws_off, X_ws, a); break;
        }
        const int tiles = (max_rows + 15) / 16;
        hipLaunchKernelGGL(msim::pool_pdist_kernel, dim3(tiles, tiles, n_pages), dim3(256), 0, st, d_off, ws_off, X_ws, D_ws);
    }
    // pages of at most kPoolMaxN rows keep the clustering state in LDS; a call with a longer page runs the variant whose long pages
    // keep it in their (by then dead) region of X_ws
    if (max_rows > msim::kPoolMaxN) {
        static std::atomic<int> configured_big[kMaxDevices];
        if (int rc = allow_lds(msim::pool_cluster_kernel<true>, (int)sizeof(msim::PoolLds), configured_big)) return rc;
        hipLaunchKernelGGL(msim::pool_cluster_kernel<true>, dim3(n_pages), dim3(msim::kPoolThreads), sizeof(msim::PoolLds), st, d_off, ws_off,
                           X_ws, D_ws, labels, n_clusters, pool_factor);
    } else {
        static std::atomic<int> configured[kMaxDevices];
        if (int rc = allow_lds(msim::pool_cluster_kernel<false>, (int)sizeof(msim::PoolLds), configured)) return rc;
        hipLaunchKernelGGL(msim::pool_cluster_kernel<false>, dim3(n_pages), dim3(msim::kPoolThreads), sizeof(msim::PoolLds), st, d_off, ws_off,
                           X_ws, D_ws, labels, n_clusters, pool_factor);
    }
    return launch_failed("token pooling");
}

int msim_pool_reduce(int dtype, const void *E, const int32_t *d_off, int n_pages, int dim, int ld_in, const int32_t *labels,
                     const int32_t *out_off, void *out, int ld_out, void *stream) {
    if (n_pages < 0) return fail(MSIM_EINVAL, "negative size");
    if (n_pages == 0) return MSIM_OK;
    if (!E || !d_off || !labels || !out_off || !out) return fail(MSIM_EINVAL, "null pointer argument");
    if (dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16 && dtype != MSIM_DTYPE_F32) return fail(MSIM_EUNSUPPORTED, "dtype code %d", dtype);
    if (dim <= 0 || dim > 2048 || ld_in < dim || ld_out < dim) return fail(MSIM_EUNSUPPORTED, "dim=%d (ld_in=%d ld_out=%d)", dim, ld_in, ld_out);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char *e = static_cast<const char *>(E);
    char *o = static_cast<char *>(out);
    const int es = elem_bytes(dtype);
    switch (dtype) {
        case MSIM_DTYPE_F32: hipLaunchKernelGGL(msim::pool_reduce_kernel<msim::kDtypeF32>, dim3(n_pages), dim3(256), 0, st, e, d_off, labels, out_off, o, dim, ld_in * es, ld_out * es); break;
        case MSIM_DTYPE_F16: hipLaunchKernelGGL(msim::pool_reduce_kernel<msim::kDtypeF16>, dim3(n_pages), dim3(256), 0, st, e, d_off, labels, out_off, o, dim, ld_in * es, ld_out * es); break;
        default: hipLaunchKernelGGL(msim::pool_reduce_kernel<msim::kDtypeBf16>, dim3(n_pages), dim3(256), 0, st, e, d_off, labels, out_off, o, dim, ld_in * es, ld_out * es); break;
    }
    return launch_failed("pool_reduce_kernel");
}

int msim_host_gather(void *dst, const void *const *src, const int64_t *dst_off, const int64_t *nbytes, int64_t n, int n_threads) {
    if (n < 0) return fail(MSIM_EINVAL, "negative count");
    if (n == 0) return MSIM_OK;
    if (!dst || !src || !dst_off || !nbytes) return fail(MSIM_EINVAL, "null pointer argument");
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (nbytes[i] < 0 || dst_off[i] < 0 || (nbytes[i] > 0 && !src[i])) return fail(MSIM_EINVAL, "bad buffer %lld", (long long)i);
        total += nbytes[i];
    }
    char *d = static_cast<char *>(dst);
    auto run = [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i)
            if (nbytes[i]) memcpy(d + dst_off[i], src[i], (size_t)nbytes[i]);
    };
    int nt = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
    if (total < (int64_t)(4 << 20) * nt) nt = (int)(total >> 22) < 1 ? 1 : (int)(total >> 22);   // below ~4 MiB per thread: fewer
    if (nt <= 1 || n < 2) {
        run(0, n);
        return MSIM_OK;
    }
    std::vector<std::thread> pool;
    pool.reserve(nt);
    const int64_t per = (total + nt - 1) / nt;
    int64_t lo = 0, acc = 0;
    for (int64_t i = 0; i < n; ++i) {
        acc += nbytes[i];
        if (acc >= per || i + 1 == n) {
            pool.emplace_back(run, lo, i + 1);
            lo = i + 1;
            acc = 0;
        }
    }
    for (auto &t : pool) t.join();
    return MSIM_OK;
}

}  // extern "C"

namespace {
inline bool row_is_zero(const char *p, int64_t row_bytes) {
    int64_t i = 0;
    uint64_t acc = 0;
    for (; i + 8 <= row_bytes; i += 8) {
        uint64_t v;
        memcpy(&v, p + i, 8);
        acc |= v;
    }
    for (; i < row_bytes; ++i) acc |= (unsigned char)p[i];
    return acc == 0;
}

template <class F>
void host_parallel(int64_t n, int n_threads, int64_t work_bytes, F &&body) {
    int nt = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : n_threads);
    if (work_bytes < (int64_t)(4 << 20) * nt) nt = (int)(work_bytes >> 22) < 1 ? 1 : (int)(work_bytes >> 22);
    if (nt <= 1 || n < 2) {
        body(0, n);
        return;
    }
    std::vector<std::thread> pool;
    pool.reserve(nt);
    const int64_t per = (n + nt - 1) / nt;
    for (int64_t lo = 0; lo < n; lo += per) pool.emplace_back(body, lo, lo + per < n ? lo + per : n);
    for (auto &t : pool) t.join();
}
}  // namespace

extern "C" {

int msim_host_count_nonzero_rows(const void *const *src, const int64_t *rows, int64_t row_bytes, int64_t n, int32_t *counts,
                                 int n_threads) {
    if (n < 0 || row_bytes <= 0) return fail(MSIM_EINVAL, "bad size");
    if (n == 0) return MSIM_OK;
    if (!src || !rows || !counts) return fail(MSIM_EINVAL, "null pointer argument");
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] > 0x7fffffff || (rows[i] > 0 && !src[i])) return fail(MSIM_EINVAL, "bad buffer %lld", (long long)i);
        total += rows[i] * row_bytes;
    }
    host_parallel(n, n_threads, total, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const char *p = static_cast<const char *>(src[i]);
            int32_t c = 0;
            for (int64_t r = 0; r < rows[i]; ++r) c += row_is_zero(p + r * row_bytes, row_bytes) ? 0 : 1;
            counts[i] = c;
        }
    });
    return MSIM_OK;
}

int msim_host_gather_nonzero_rows(void *dst, const void *const *src, const int64_t *rows, int64_t row_bytes, const int64_t *dst_row,
                                  int64_t n, int n_threads) {
    if (n < 0 || row_bytes <= 0) return fail(MSIM_EINVAL, "bad size");
    if (n == 0) return MSIM_OK;
    if (!dst || !src || !rows || !dst_row) return fail(MSIM_EINVAL, "null pointer argument");
    int64_t total = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (rows[i] < 0 || dst_row[i] < 0 || (rows[i] > 0 && !src[i])) return fail(MSIM_EINVAL, "bad buffer %lld", (long long)i);
        total += rows[i] * row_bytes;
    }
    char *d = static_cast<char *>(dst);
    host_parallel(n, n_threads, total, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; ++i) {
            const char *p = static_cast<const char *>(src[i]);
            char *o = d + dst_row[i] * row_bytes;
            for (int64_t r = 0; r < rows[i]; ++r) {
                if (row_is_zero(p + r * row_bytes, row_bytes)) continue;
                memcpy(o, p + r * row_bytes, (size_t)row_bytes);
                o += row_bytes;
            }
        }
    });
    return MSIM_OK;
}

}  // extern "C"
