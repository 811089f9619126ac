// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the training path -- pair lists and their backward, K1t and the dense
// backward, the loss epilogue and the smooth-max kernels.
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates,
// frees or synchronises, so every entry point is hipGraph-capturable.  The kernels included below are defined and launched in
// this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "abi_shapes.hpp"
#include "maxsim_batch_t.hip"
#include "maxsim_dense_t.hip"
#include "maxsim_pairs.hip"
#include "maxsim_generic.hip"
#include "maxsim_bwd.hip"
#include "maxsim_smooth.hip"
#include "loss_epilogue.hip"

using namespace msim_abi;

namespace {

template <int TPQ, bool F16, int WPP, int RING = msim::kPairsRing>
int launch_pairs_argmax(const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0,
                        const int32_t *pairs, float *out_scores, int32_t *out_argmax, const msim::PairsArgs &a,
                        const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::maxsim_pairs_argmax_kernel<TPQ, F16, WPP, RING>;
    constexpr int lds = 4 * RING * msim::kSlabBytes + (WPP > 1 ? 4 * TPQ * msim::kTokTile * 8 : 0);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    const int wg_needed = WPP > 1 ? a.n_pairs : (a.n_pairs + 3) / 4;
    const int wg_cap = di.cus * (di.lds_per_cu / lds);
    hipLaunchKernelGGL(kern, dim3(wg_needed < wg_cap ? wg_needed : wg_cap), dim3(256), lds, st, Q, D, d_off, clamp0, pairs,
                       out_scores, out_argmax, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_pairs_argmax_kernel<%d,%d> launch: %s", TPQ, WPP, hipGetErrorString(e));
    return MSIM_OK;
}

template <int TPQ1, int GQ, bool F16>
int launch_allpairs_argmax(const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0, float *out_scores,
                           long long ld, int32_t *out_argmax, const msim::PairsArgs &a, const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::maxsim_allpairs_argmax_kernel<TPQ1, GQ, F16>;
    constexpr int lds = 4 * msim::kPairsRing * msim::kSlabBytes;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    const long long work = (long long)((a.n_q + GQ - 1) / GQ) * a.n_d;
    const long long wg_needed = (work + 3) / 4;
    const int wg_cap = di.cus * (di.lds_per_cu / lds);
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), lds, st, Q, D, d_off, clamp0, out_scores, ld,
                       out_argmax, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_allpairs_argmax_kernel<%d,%d> launch: %s", TPQ1, GQ, hipGetErrorString(e));
    return MSIM_OK;
}

template <bool F16>
int allpairs_argmax_dispatch(int tpq, const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0, float *out_scores,
                             long long ld, int32_t *out_argmax, const msim::PairsArgs &a, const DeviceInfo &di, hipStream_t st) {
    switch (tpq) {
        case 1: return launch_allpairs_argmax<1, 4, F16>(Q, D, d_off, clamp0, out_scores, ld, out_argmax, a, di, st);
        case 2: return launch_allpairs_argmax<2, 2, F16>(Q, D, d_off, clamp0, out_scores, ld, out_argmax, a, di, st);
        case 3: return launch_allpairs_argmax<3, 1, F16>(Q, D, d_off, clamp0, out_scores, ld, out_argmax, a, di, st);
        default: return launch_allpairs_argmax<4, 1, F16>(Q, D, d_off, clamp0, out_scores, ld, out_argmax, a, di, st);
    }
}

// short pair lists (the 2B pairs of the pairwise loss): one workgroup per pair, four waves sharing the document (latency);
// long lists: one wave per pair (throughput)
constexpr int kPairsSplitMax = 1024;

template <bool F16>
int pairs_argmax_dispatch(int tpq, const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0,
                          const int32_t *pairs, float *out_scores, int32_t *out_argmax, const msim::PairsArgs &a,
                          const DeviceInfo &di, hipStream_t st) {
    if (a.n_pairs <= di.cus) {       // every pair's workgroup is resident at once: a deep ring (three slabs in flight per wave) costs nothing
        switch (tpq) {
            case 1: return launch_pairs_argmax<1, F16, 4, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            case 2: return launch_pairs_argmax<2, F16, 4, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            case 3: return launch_pairs_argmax<3, F16, 4, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            default: return launch_pairs_argmax<4, F16, 4, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        }
    }
    if (a.n_pairs <= kPairsSplitMax) {
        switch (tpq) {
            case 1: return launch_pairs_argmax<1, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            case 2: return launch_pairs_argmax<2, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            case 3: return launch_pairs_argmax<3, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            default: return launch_pairs_argmax<4, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        }
    }
    switch (tpq) {
        case 1: return launch_pairs_argmax<1, F16, 1>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        case 2: return launch_pairs_argmax<2, F16, 1>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        case 3: return launch_pairs_argmax<3, F16, 1>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        default: return launch_pairs_argmax<4, F16, 1>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
    }
}

// long queries against short documents (the trainer's symmetric direction): the transposed pair kernel, one workgroup per pair
template <int TPD, bool F16, int RING>
int launch_pairs_argmax_t(const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0,
                          const int32_t *pairs, float *out_scores, int32_t *out_argmax, const msim::PairsArgs &a,
                          const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::maxsim_pairs_argmax_t_kernel<TPD, F16, RING>;
    constexpr int lds = 4 * RING * msim::kSlabBytes + 16;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    const int wg_cap = 4 * di.cus * (di.lds_per_cu / lds);        // a few rounds of resident workgroups; the kernel strides beyond
    hipLaunchKernelGGL(kern, dim3(a.n_pairs < wg_cap ? a.n_pairs : wg_cap), dim3(256), lds, st, Q, D, d_off, clamp0, pairs,
                       out_scores, out_argmax, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_pairs_argmax_t_kernel<%d> launch: %s", TPD, hipGetErrorString(e));
    return MSIM_OK;
}

template <bool F16>
int pairs_argmax_t_dispatch(int tpd, const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const uint8_t *clamp0,
                            const int32_t *pairs, float *out_scores, int32_t *out_argmax, const msim::PairsArgs &a,
                            const DeviceInfo &di, hipStream_t st) {
    // few pairs (the pairwise loss' 2B): every workgroup resident at once, a 4-slab ring per wave hides the LDS-DMA round trips;
    // many (dense upstream gradients: B x C pairs): the 2-slab ring keeps two workgroups on a CU
    if (a.n_pairs <= di.cus) {
        switch (tpd) {
            case 1: return launch_pairs_argmax_t<1, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            case 2: return launch_pairs_argmax_t<2, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
            default: return launch_pairs_argmax_t<4, F16, 4>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        }
    }
    switch (tpd) {
        case 1: return launch_pairs_argmax_t<1, F16, 2>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        case 2: return launch_pairs_argmax_t<2, F16, 2>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
        default: return launch_pairs_argmax_t<4, F16, 2>(Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, di, st);
    }
}

// dD for SHORT documents with LONG entry lists (the trainer's symmetric direction: maxsim_bwd.hip, dense form): number of splits of
// every document's pair list, 0 = use the row-range kernel.  A function of the sizes alone (host side, no device read).
struct DdPlan {
    int mode = 0;          // 0: the row-range kernel; 1: dense, per (document, split); 2: dense, per (pair, split)
    int splits = 0;
    size_t bytes = 0;      // scratch
};

DdPlan dd_plan(int n_pairs, int Lq, int n_d, int dim, int max_doc_rows, int cus) {
    DdPlan pl;
    if (n_d <= 0 || n_pairs <= 0 || max_doc_rows <= 0 || max_doc_rows > msim::kBwdRows || dim <= 0) return pl;
    const long long entries_per_doc = (long long)n_pairs * Lq / n_d;
    if (entries_per_doc >= 1024) {                                // long lists on average: the dense upstream gradient of ColbertLoss
        int splits = (4 * cus + n_d - 1) / n_d;                   // ~4 workgroups per CU (16-32 KiB of LDS each)
        const long long by_work = entries_per_doc / 256;          // at least 256 (pair, token) entries per split
        if (splits > by_work) splits = (int)by_work;
        if (splits > 64) splits = 64;
        pl.mode = 1;
        pl.splits = splits < 1 ? 1 : splits;
        pl.bytes = (size_t)pl.splits * n_d * max_doc_rows * dim * sizeof(float);
    } else if (Lq >= 256) {
        // few pairs, but each brings a long list to ITS document (the pairwise loss in the symmetric direction: 2B pairs of 780 tokens
        // over 256 documents -- 195 entries per document on average, 780 or more for the <= 2B documents that have any): the row-range
        // kernel walked those 780 entries as three rounds of dependent gathers on ONE workgroup per document, 159 us of a 370 us step.
        // One workgroup per (pair, split of ~64 tokens): every step of the walk is a dependent gather, so few of them per workgroup
        pl.mode = 2;
        pl.splits = Lq / 64 > 16 ? 16 : Lq / 64;
        pl.bytes = (size_t)pl.splits * n_pairs * max_doc_rows * dim * sizeof(float);
    }
    if (pl.bytes > ((size_t)256 << 20)) pl = DdPlan{};            // scratch stays bounded: the row-range kernel serves the rest
    return pl;
}

// A side stream and a few events per device, created on first use (round 6).  The two GEMM kernels of msim_dense_t_bwd (dP, dR) are
// independent of each other and each alone keeps the matrix cores ~27 % busy (latency chains, one workgroup per CU): the call forks
// them onto two streams and joins before it returns to the caller's stream, so they share the CUs (LDS 67 + 70 KiB, 4 waves per
// SIMD) and cover each other's stalls (ColbertLoss, both directions at config 5's shape: 0.468 -> 0.390 ms).  Fork / join with
// events is the capturable pattern: a hipGraph of the step gets two parallel branches.
struct SideStream {
    hipStream_t st = nullptr;
    hipEvent_t ev[8] = {};
    std::atomic<int> ready{0};
    std::atomic<unsigned> next{0};
};
SideStream g_side[kMaxDevices];

int side_stream(SideStream **out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= kMaxDevices) return fail(MSIM_ELAUNCH, "device ordinal %d out of range", dev);
    SideStream &s = g_side[dev];
    if (!s.ready.load(std::memory_order_acquire)) {
        static std::mutex mu;
        std::lock_guard<std::mutex> lock(mu);
        if (!s.ready.load(std::memory_order_relaxed)) {
            hipError_t e = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking);
            if (e != hipSuccess) return fail(MSIM_ELAUNCH, "hipStreamCreateWithFlags: %s", hipGetErrorString(e));
            for (auto &ev : s.ev) {
                e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
                if (e != hipSuccess) return fail(MSIM_ELAUNCH, "hipEventCreateWithFlags: %s", hipGetErrorString(e));
            }
            s.ready.store(1, std::memory_order_release);
        }
    }
    *out = &s;
    return MSIM_OK;
}

// every gradient kernel of one msim_pairs_bwd call; OUT16: dQ / dD in the embeddings' own 16-bit dtype
template <int DT, bool OUT16>
void launch_bwd_kernels(const char *Q, const char *D, const int32_t *d_off, int max_doc_rows, const int32_t *pairs,
                        const int32_t *order_by_doc, const float *g, const int32_t *argmax, void *dQ, void *dD,
                        const msim::PairsArgs &a, int dim, int cus, hipStream_t st, float *partial, const DdPlan &pl, msim::GScale gs) {
    const int row_bytes = dim * msim::elem_size<DT>();
    // (round 6, measured and NOT kept: dQ on a second stream beside dD, as msim_dense_t_bwd does with its two GEMM kernels -- the
    // fork / join edges cost more than the 5-20 us of overlap they buy here: pairwise loss 0.102 -> 0.123 ms, ColbertLoss 0.188 -> 0.209)
    if (a.n_q > 0 && a.Lq > 0) {
        // tokens per wave: the pair-range lookup is per wave, so few waves per query once there are more tokens than the chip has waves
        const long long tokens = (long long)a.n_q * a.Lq;
        int tpw = (int)((tokens + 4095) / 4096);
        tpw = tpw < 1 ? 1 : (tpw > 16 ? 16 : tpw);
        // few tokens with long pair lists (a dense gradient: 1024 tokens x 256 pairs at config 5's shape): the four waves of a workgroup
        // share the tokens and split the pairs (maxsim_bwd.hip: psplit)
        const int psplit = (tokens <= 2048 && (long long)a.n_pairs >= 64LL * a.n_q) ? 1 : 0;
        if (psplit) tpw = 1;
        const int chunks = psplit ? a.Lq : (a.Lq + 4 * tpw - 1) / (4 * tpw);
        hipLaunchKernelGGL((msim::maxsim_bwd_dq_kernel<DT, OUT16>), dim3((unsigned)a.n_q * chunks), dim3(256), 0, st, D, d_off, pairs, g,
                           argmax, dQ, a, row_bytes, tpw, gs, psplit);
    }
    const int ry = (max_doc_rows + msim::kBwdRows - 1) / msim::kBwdRows;
    const int zc = (dim + 127) / 128;
    if (a.n_d <= 0 || ry <= 0) return;
    const int splits = pl.splits;
    if (pl.mode == 2 && partial) {
        const int lds = 2 * max_doc_rows * 128 * (int)sizeof(float);  // <= 64 KiB
        hipLaunchKernelGGL(msim::maxsim_bwd_dd_pairs_kernel<DT>, dim3(a.n_pairs, splits, zc), dim3(256), lds, st, Q, d_off, pairs, order_by_doc,
                           g, argmax, partial, a, dim, max_doc_rows, splits, gs);
        const int per_wg = 256 * (OUT16 ? 2 : 1);                     // one step per thread
        hipLaunchKernelGGL((msim::maxsim_bwd_dd_pairsum_kernel<DT, OUT16>), dim3(a.n_d, (max_doc_rows * dim + per_wg - 1) / per_wg), dim3(256), 0,
                           st, partial, d_off, pairs, order_by_doc, dD, a.n_pairs, dim, max_doc_rows, splits);
        return;
    }
    if (pl.mode == 1 && partial) {
        const int lds = 2 * max_doc_rows * 128 * (int)sizeof(float);  // <= 64 KiB
        hipLaunchKernelGGL(msim::maxsim_bwd_dd_dense_kernel<DT>, dim3(a.n_d, splits, zc), dim3(256), lds, st, Q, d_off, pairs, order_by_doc,
                           g, argmax, partial, a, dim, max_doc_rows, splits, gs);
        const int per_thread = OUT16 ? 2 : 1;
        hipLaunchKernelGGL((msim::maxsim_bwd_dd_sum_kernel<DT, OUT16>), dim3(a.n_d, (max_doc_rows * dim + 256 * per_thread - 1) / (256 * per_thread)),
                           dim3(256), 0, st, partial, d_off, pairs, order_by_doc, dD, a.n_d, a.n_pairs, dim, max_doc_rows, splits);
        return;
    }
    // round 6: documents whose entry lists fit the LDS lists of the row-list kernel (a bound the host can know: a document meets every
    // query at most twice in the lists the losses make) are bucketed by row once instead of re-scanned per 64-row range
    static const bool rows_off = ab_env("MSIM_DD_ROWS", 1) == 0;          // tuning knob (A/B), not part of the ABI
    const long long pairs_per_doc = std::min<long long>(a.n_pairs, 2LL * a.n_q);
    // (a list with a handful of entries per document -- the pairwise loss: 2B pairs over C documents -- stays with the kernel below,
    // whose eight small workgroups per CU zero-fill the untouched documents faster: 13.5 against 18 us at config 5's shape)
    const bool dense_enough = (long long)a.n_pairs * a.Lq >= 64LL * a.n_d;
    if (!rows_off && dense_enough && pairs_per_doc <= msim::kRowsMaxPairs && pairs_per_doc * a.Lq <= msim::kRowsMaxEnt) {
        int sy = (2 * cus + a.n_d - 1) / a.n_d;                            // about two 512-thread workgroups per CU
        const int by_rows = (max_doc_rows + 63) / 64, need = (max_doc_rows + msim::kRowsMaxRows - 1) / msim::kRowsMaxRows;
        sy = sy > by_rows ? by_rows : sy;
        sy = sy < need ? need : (sy < 1 ? 1 : sy);
        hipLaunchKernelGGL((msim::maxsim_bwd_dd_rows_kernel<DT, OUT16>), dim3(a.n_d, sy, zc), dim3(msim::kRowsThreads), 0, st, Q, d_off, pairs,
                           order_by_doc, g, argmax, dD, a, dim, gs);
        return;
    }
    // row ranges per workgroup: about eight workgroups per CU in total (each looks its document's pair range up once)
    int gy = (8 * cus + a.n_d - 1) / a.n_d;
    gy = gy < 1 ? 1 : (gy > ry ? ry : gy);
    hipLaunchKernelGGL((msim::maxsim_bwd_dd_kernel<DT, OUT16>), dim3(a.n_d, gy, zc), dim3(256), 0, st, Q, d_off, pairs, order_by_doc, g,
                       argmax, dD, a, dim, gs);
}

template <int DT>
int generic_pairs_argmax(const char *Q, const char *D, const int32_t *d_off, const uint8_t *clamp0, const int32_t *pairs,
                         float *out_scores, int32_t *out_argmax, const msim::PairsArgs &a, int row_bytes, const DeviceInfo &di,
                         hipStream_t st) {
    const int wg_needed = (a.n_pairs + 3) / 4;
    const int wg_cap = di.cus * 8;
    hipLaunchKernelGGL(msim::maxsim_generic_pairs_argmax_kernel<DT>, dim3(wg_needed < wg_cap ? wg_needed : wg_cap), dim3(256), 0,
                       st, Q, D, d_off, clamp0, pairs, out_scores, out_argmax, a, row_bytes);
    return launch_failed("maxsim_generic_pairs_argmax_kernel");
}

// ---------------------------------------------------------------- smooth-max (tau * logsumexp) kernels
template <int DT, int T>
int launch_smooth(const GenericCall &c, float tau) {
    auto kern = msim::maxsim_smooth_kernel<DT, T>;
    const int lds = T * msim::kTokTile * (c.row_bytes + 16);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, 160 * 1024, configured)) return rc;
    msim::SmoothArgs a;
    a.ld = c.ld;
    a.n_q = c.n_q;
    a.Lq = c.Lq;
    a.n_d = c.n_d;
    a.row_bytes = c.row_bytes;
    a.tau = tau;
    const int tpq = (c.Lq + msim::kTokTile - 1) / msim::kTokTile;
    const int groups = tpq <= T ? (c.n_q + (T / tpq) - 1) / (T / tpq) : c.n_q;
    if (groups > 65535) return fail(MSIM_EUNSUPPORTED, "too many query groups (%d) for one launch", groups);
    const int wg_needed = (c.n_d + msim::kGenericWaves - 1) / msim::kGenericWaves;
    int per_cu = c.di->lds_per_cu / lds;
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int wg_cap = c.di->cus * per_cu;
    hipLaunchKernelGGL(kern, dim3(wg_needed < wg_cap ? wg_needed : wg_cap, groups), dim3(msim::kGenericWaves * 64), lds, c.st,
                       c.Q, c.D, c.d_off, c.scores, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_smooth_kernel<%d,%d> launch: %s", DT, T, hipGetErrorString(e));
    return MSIM_OK;
}

template <int DT>
int smooth_dispatch(const GenericCall &c, float tau) {
    const int tpq = (c.Lq + msim::kTokTile - 1) / msim::kTokTile;
    const long long tiles = (long long)c.n_q * tpq;
    const int tile_lds = msim::kTokTile * (c.row_bytes + 16);
    int T = 2;                                   // (max, sum) state per tile on top of the accumulators: two tiles per wave
    while (T > 1 && (T * tile_lds > 80 * 1024 || T / 2 >= tiles)) T >>= 1;
    return T == 2 ? launch_smooth<DT, 2>(c, tau) : launch_smooth<DT, 1>(c, tau);
}

template <int DT>
int smooth_pairs(const char *Q, const char *D, const int32_t *d_off, const int32_t *pairs, float *out_scores, float *out_lse,
                 const msim::PairsArgs &a, int row_bytes, float tau, const DeviceInfo &di, hipStream_t st) {
    const int wg_needed = (a.n_pairs + 3) / 4;
    const int wg_cap = di.cus * 8;
    hipLaunchKernelGGL(msim::maxsim_smooth_pairs_kernel<DT>, dim3(wg_needed < wg_cap ? wg_needed : wg_cap), dim3(256), 0, st, Q, D,
                       d_off, pairs, out_scores, out_lse, a, row_bytes, tau);
    return launch_failed("maxsim_smooth_pairs_kernel");
}

template <int DT>
int smooth_bwd(const char *Q, const char *D, const int32_t *d_off, int max_doc_rows, const int32_t *pairs,
               const int32_t *order_by_doc, const float *g, const float *lse, float *dQ, float *dD, float *workspace,
               msim::SmoothBwdArgs a, int n_split, hipStream_t st) {
    const int tpq = (a.Lq + msim::kTokTile - 1) / msim::kTokTile;
    const int cg = (a.dim + 32 * msim::kSmoothCB - 1) / (32 * msim::kSmoothCB);
    const bool hoist = a.row_bytes <= 256;                       // the owner tile's fragments fit 8 registers quads
    static const bool no_stage = ab_env("MSIM_SMOOTH_NO_STAGE", 0) != 0;   // A/B knob (measurement builds)
    const int slabs = (max_doc_rows + 31) / 32;
    if constexpr (DT != msim::kDtypeF32) {
        if (a.row_bytes == msim::kRowBytes && a.dim == msim::kDim && !no_stage) {   // 128 x 16-bit rows: staged "other" tiles
            constexpr bool F16 = DT == msim::kDtypeF16;
            if (a.n_q > 0) {
                a.n_split = n_split;
                auto kern = msim::maxsim_smooth_bwd_staged_kernel<F16, true>;
                constexpr int lds = msim::kSmoothWavesDQ * msim::kSmoothStageBytes;
                static std::atomic<int> configured[kMaxDevices];
                if (int rc = allow_lds(kern, lds, configured)) return rc;
                hipLaunchKernelGGL(kern, dim3(a.n_q * n_split, tpq, 1), dim3(msim::kSmoothWavesDQ * 64), lds, st, Q, D, d_off, pairs,
                                   order_by_doc, g, lse, n_split > 1 ? workspace : dQ, a);
                if (n_split > 1) {
                    const long long n = (long long)a.n_q * a.Lq * a.dim;
                    hipLaunchKernelGGL(msim::smooth_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, workspace, dQ, n,
                                       n_split);
                }
            }
            if (a.n_d > 0 && slabs > 0) {
                a.n_split = 1;
                auto kern = msim::maxsim_smooth_bwd_staged_kernel<F16, false>;
                constexpr int lds = msim::kSmoothWavesDD * msim::kSmoothStageBytes;
                static std::atomic<int> configured[kMaxDevices];
                if (int rc = allow_lds(kern, lds, configured)) return rc;
                hipLaunchKernelGGL(kern, dim3(a.n_d, slabs, 1), dim3(msim::kSmoothWavesDD * 64), lds, st, Q, D, d_off, pairs, order_by_doc, g,
                                   lse, dD, a);
            }
            hipError_t es = hipGetLastError();
            if (es != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_smooth_bwd_staged_kernel launch: %s", hipGetErrorString(es));
            return MSIM_OK;
        }
    }
    if (a.n_q > 0) {
        a.n_split = n_split;
        const dim3 grid(a.n_q * n_split, tpq, cg), block(msim::kSmoothWavesDQ * 64);
        float *dst = n_split > 1 ? workspace : dQ;
        if (hoist)
            hipLaunchKernelGGL((msim::maxsim_smooth_bwd_kernel<DT, true, true>), grid, block, 0, st, Q, D, d_off, pairs, order_by_doc, g, lse, dst, a);
        else
            hipLaunchKernelGGL((msim::maxsim_smooth_bwd_kernel<DT, true, false>), grid, block, 0, st, Q, D, d_off, pairs, order_by_doc, g, lse, dst, a);
        if (n_split > 1) {
            const long long n = (long long)a.n_q * a.Lq * a.dim;
            hipLaunchKernelGGL(msim::smooth_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, workspace, dQ, n, n_split);
        }
    }
    if (a.n_d > 0 && slabs > 0) {
        a.n_split = 1;
        const dim3 grid(a.n_d, slabs, cg), block(msim::kSmoothWavesDD * 64);
        if (hoist)
            hipLaunchKernelGGL((msim::maxsim_smooth_bwd_kernel<DT, false, true>), grid, block, 0, st, Q, D, d_off, pairs, order_by_doc, g, lse, dD, a);
        else
            hipLaunchKernelGGL((msim::maxsim_smooth_bwd_kernel<DT, false, false>), grid, block, 0, st, Q, D, d_off, pairs, order_by_doc, g, lse, dD, a);
    }
    return launch_failed("maxsim_smooth_bwd_kernel");
}

// number of workgroups that share one owner tile's pair list in the dQ pass (enough to fill the chip twice)
int smooth_dq_split(int n_q, int Lq, const DeviceInfo &di) {
    const int tiles = n_q * ((Lq + msim::kTokTile - 1) / msim::kTokTile);
    int s = (2 * di.cus + tiles - 1) / (tiles > 0 ? tiles : 1);
    return s < 1 ? 1 : (s > 32 ? 32 : s);
}

// ---------------------------------------------------------------- K1t: long queries x short documents, all pairs
template <bool F16, int U, int DPW, bool ROUTE>
int launch_batch_t(const uint16_t *Q, const uint16_t *D, float *scores, int32_t *q_lengths, uint8_t *route, msim::BatchTArgs a,
                   const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::maxsim_batch_t_kernel<F16, U, DPW, ROUTE>;
    constexpr int lds = 3 * 4 * msim::kSlabBytes;                  // 96 KiB ring
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    a.n_blocks = (a.n_d + 8 * DPW - 1) / (8 * DPW);
    // page slots per XCD: every page its own slot until the launch holds ~4 workgroups per CU, then the workgroups walk pages
    int slots_p = (a.n_q + 7) / 8;
    const int cap = (4 * di.cus / 8 + a.n_blocks - 1) / a.n_blocks;
    if (slots_p > cap) slots_p = cap < 1 ? 1 : cap;
    a.slots_p = slots_p;
    a.n_slots = slots_p * a.n_blocks;
    hipLaunchKernelGGL(kern, dim3(8 * a.n_slots), dim3(512), lds, st, Q, D, scores, q_lengths, route, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_batch_t_kernel<%d,%d> launch: %s", U, DPW, hipGetErrorString(e));
    return MSIM_OK;
}

template <bool F16>
int batch_t_dispatch(int units, const uint16_t *Q, const uint16_t *D, float *scores, int32_t *ql, uint8_t *route,
                     const msim::BatchTArgs &a, const DeviceInfo &di, hipStream_t st) {
    if (route) {        // with the routing bytes of the dense backward (documents of at most 64 rows)
        if (units <= 1) return launch_batch_t<F16, 1, 8, true>(Q, D, scores, ql, route, a, di, st);
        if (units == 2) return launch_batch_t<F16, 2, 4, true>(Q, D, scores, ql, route, a, di, st);
        if (units == 3) return launch_batch_t<F16, 3, 2, true>(Q, D, scores, ql, route, a, di, st);
        return launch_batch_t<F16, 4, 2, true>(Q, D, scores, ql, route, a, di, st);
    }
    if (units <= 1) return launch_batch_t<F16, 1, 8, false>(Q, D, scores, ql, nullptr, a, di, st);
    if (units == 2) return launch_batch_t<F16, 2, 4, false>(Q, D, scores, ql, nullptr, a, di, st);
    if (units == 3) return launch_batch_t<F16, 3, 2, false>(Q, D, scores, ql, nullptr, a, di, st);
    if (units == 4) return launch_batch_t<F16, 4, 2, false>(Q, D, scores, ql, nullptr, a, di, st);
    return launch_batch_t<F16, 8, 1, false>(Q, D, scores, ql, nullptr, a, di, st);
}

int fwd_transposed(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim, float *scores,
                   int64_t ld_scores, int32_t *q_lengths, uint8_t *route, void *stream) {
    if (n_q < 0 || n_d < 0 || Lq <= 0 || Ld <= 0) return fail(MSIM_EINVAL, "negative or empty size");
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!Q || !D || !scores) return fail(MSIM_EINVAL, "null pointer argument");
    if ((dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16) || dim != msim::kDim)
        return fail(MSIM_EUNSUPPORTED, "msim_fwd_transposed takes bf16 / f16 embeddings of width %d", msim::kDim);
    if (Ld > 8 * msim::kUnitTok) return fail(MSIM_EUNSUPPORTED, "resident documents of at most %d rows (got %d)", 8 * msim::kUnitTok, Ld);
    if (route && Ld > msim::kDenseTMaxLd)
        return fail(MSIM_EUNSUPPORTED, "the routing is kept for resident documents of at most %d rows (got %d)", msim::kDenseTMaxLd, Ld);
    if ((long long)Lq * msim::kRowBytes >= (1ll << 31)) return fail(MSIM_EUNSUPPORTED, "queries of %d rows", Lq);
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "ld_scores < n_d");
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D)) & 15) return fail(MSIM_EINVAL, "embeddings must be 16-byte aligned");
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::BatchTArgs a{};
    a.ld = ld_scores;
    a.n_q = n_q;
    a.Lq = Lq;
    a.n_d = n_d;
    a.Ld = Ld;
    a.Lq_pad = msim::dense_t_lq_pad(Lq);
    const int units = (Ld + msim::kUnitTok - 1) / msim::kUnitTok;
    const uint16_t *q = static_cast<const uint16_t *>(Q), *d = static_cast<const uint16_t *>(D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == MSIM_DTYPE_F16 ? batch_t_dispatch<true>(units, q, d, scores, q_lengths, route, a, *di, st)
                                   : batch_t_dispatch<false>(units, q, d, scores, q_lengths, route, a, *di, st);
}

// ---- the dense hard-max backward of the transposed shape (maxsim_dense_t.hip)
constexpr int kDenseTMaxDocs = 4096;        // dP keeps one weight pair per document of the page in LDS
constexpr int kDenseTMaxPagesPer = 256;     // dR keeps one weight pair per (page of its split, document of the workgroup) in LDS
struct DenseTPlan {
    size_t rimg, pimg, partial, bytes;   // byte offsets of the two operand images and the page-split partials; total
    int ks, nsb, nc, n_split, pages_per, doc_groups;
};
DenseTPlan dense_t_plan(int n_q, int Lq, int n_d, int Ld, int cus) {
    DenseTPlan p{};
    p.ks = (Ld + 31) / 32;
    p.nsb = Ld <= 16 ? 1 : Ld <= 32 ? 2 : 4;     // 16-row blocks per document: NSB * NC = 4 combinations per wave pair
    p.nc = 4 / p.nsb;
    p.doc_groups = (n_d + 4 * p.nc - 1) / (4 * p.nc);
    int split = (cus + p.doc_groups - 1) / (p.doc_groups > 0 ? p.doc_groups : 1);
    const int min_split = (n_q + kDenseTMaxPagesPer - 1) / kDenseTMaxPagesPer;
    split = split < min_split ? min_split : split;
    split = split < 1 ? 1 : split > n_q ? n_q : split;
    p.pages_per = split > 0 ? (n_q + split - 1) / split : 1;
    p.n_split = p.pages_per > 0 ? (n_q + p.pages_per - 1) / p.pages_per : 0;
    const size_t ksp = msim::dense_t_lq_pad(Lq) / 32;
    p.rimg = 0;
    p.pimg = align16((size_t)n_d * p.ks * msim::kKStepBytes);
    p.partial = p.pimg + align16((size_t)n_q * ksp * msim::kKStepBytes);
    p.bytes = p.partial + align16((size_t)p.n_split * n_d * Ld * msim::kDim * sizeof(float));
    return p;
}
bool dense_t_supported(int dtype, int n_q, int Lq, int n_d, int Ld, int dim) {
    if ((dtype != MSIM_DTYPE_BF16 && dtype != MSIM_DTYPE_F16) || dim != msim::kDim) return false;
    if (Ld <= 0 || Ld > msim::kDenseTMaxLd || Lq <= 0 || n_q <= 0 || n_d <= 0 || n_d > kDenseTMaxDocs) return false;
    const long long lq_pad = msim::dense_t_lq_pad(Lq);
    return (long long)n_q * lq_pad * msim::kRowBytes < (1ll << 31) && (long long)n_q * n_d * lq_pad < (1ll << 31) &&
           (long long)n_d * 64 * msim::kRowBytes < (1ll << 31);
}

template <bool F16>
int dense_t_bwd_launch(const uint16_t *Q, const uint16_t *D, const float *G, msim::GScale gs, const uint8_t *route, uint16_t *dQ,
                       uint16_t *dD, char *ws, const DenseTPlan &pl, msim::DenseTArgs a, hipStream_t st) {
    uint16_t *rimg = reinterpret_cast<uint16_t *>(ws + pl.rimg), *pimg = reinterpret_cast<uint16_t *>(ws + pl.pimg);
    float *partial = reinterpret_cast<float *>(ws + pl.partial);
    SideStream *side = nullptr;
    if (int rc = side_stream(&side)) return rc;
    const unsigned e0 = side->next.fetch_add(2) % 8;      // two events of the pool per call (fork, join)
    hipEvent_t fork = side->ev[e0], join = side->ev[(e0 + 1) % 8];
    // fork: the side stream takes the page image and dR (+ its split sum), the caller's stream the document image and dP
    hipError_t e = hipEventRecord(fork, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(side->st, fork, 0);
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "msim_dense_t_bwd fork: %s", hipGetErrorString(e));
    hipLaunchKernelGGL(msim::dense_t_image_kernel, dim3(a.n_d * pl.ks), dim3(256), 0, st, D, rimg, a.n_d, a.Ld, pl.ks);
    hipLaunchKernelGGL(msim::dense_t_image_kernel, dim3(a.n_q * a.ksp), dim3(256), 0, side->st, Q, pimg, a.n_q, a.Lq, a.ksp);
    static std::atomic<int> conf_long[2][kMaxDevices], conf_short[4][kMaxDevices];
    // LDS: the operand ring + the routing bytes + the W patterns / weight pairs (dP: one per document of the page, padded to whole
    // stages; dR: one per (page of the split, document of the workgroup)); the attribute is raised once to what dense_t_supported admits
    constexpr int kLongRing = msim::kDenseTLongRing, kShortRing = msim::kDenseTShortRing;
    constexpr int kLongStage = msim::kDenseTLongSteps * (8192 + 128 + 144);      // image + routing bytes + W patterns (KS = 1: one document per step)
    constexpr int lds_long_max = kLongRing * kLongStage + 4 * (kDenseTMaxDocs + 4), lds_short_max = kShortRing * (16384 + 1024) + 4 * 16 * kDenseTMaxPagesPer;
    const int lds_long = kLongRing * kLongStage + 4 * ((a.n_d + 3) / 4 * 4 + 4);
    const int lds_short = kShortRing * (16384 + 1024) + 4 * 16 * pl.pages_per;
    const dim3 grid_long((a.Lq + 127) / 128, a.n_q);
    if (pl.ks == 1) {
        auto k = msim::dense_t_bwd_long_kernel<F16, 1>;
        if (int rc = allow_lds(k, lds_long_max, conf_long[0])) return rc;
        hipLaunchKernelGGL(k, grid_long, dim3(512), lds_long, st, rimg, route, G, gs, dQ, a);
    } else {
        auto k = msim::dense_t_bwd_long_kernel<F16, 2>;
        if (int rc = allow_lds(k, lds_long_max, conf_long[1])) return rc;
        hipLaunchKernelGGL(k, grid_long, dim3(512), lds_long, st, rimg, route, G, gs, dQ, a);
    }
    const dim3 grid_short(pl.doc_groups, pl.n_split);
#define MSIM_SHORT(NSB, NC, SLOT)                                                                         \
    {                                                                                                     \
        auto k = msim::dense_t_bwd_short_kernel<F16, NSB, NC>;                                            \
        if (int rc = allow_lds(k, lds_short_max, conf_short[SLOT])) return rc;                            \
        hipLaunchKernelGGL(k, grid_short, dim3(512), lds_short, side->st, pimg, route, G, gs, partial, a); \
    }
    if (pl.nsb <= 1) MSIM_SHORT(1, 4, 0)
    else if (pl.nsb == 2) MSIM_SHORT(2, 2, 1)
    else MSIM_SHORT(4, 1, 2)
#undef MSIM_SHORT
    const long long n_elems = (long long)a.n_d * a.Ld * msim::kDim;
    hipLaunchKernelGGL(msim::dense_t_bwd_short_sum_kernel<F16>, dim3((unsigned)((n_elems / 4 + 255) / 256)), dim3(256), 0, side->st, partial, dD,
                       n_elems, pl.n_split);
    // join: the caller's stream continues when both halves are done
    e = hipEventRecord(join, side->st);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, join, 0);
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "msim_dense_t_bwd join: %s", hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "msim_dense_t_bwd launch: %s", hipGetErrorString(e));
    return MSIM_OK;
}
}  // namespace

extern "C" {

#ifdef MSIM_AB
int msim_ab_rows_trace(unsigned long long *out16) {      // measurement builds only
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(msim::g_rows_trace), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

int msim_fwd_transposed(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim, float *scores,
                        int64_t ld_scores, int32_t *q_lengths, void *stream) {
    return fwd_transposed(dtype, Q, n_q, Lq, D, n_d, Ld, dim, scores, ld_scores, q_lengths, nullptr, stream);
}

size_t msim_dense_t_route_bytes(int n_q, int Lq, int n_d) {
    if (n_q <= 0 || Lq <= 0 || n_d <= 0) return 0;
    return (size_t)n_q * n_d * msim::dense_t_lq_pad(Lq);
}

int msim_dense_t_supported(int dtype, int n_q, int Lq, int n_d, int Ld, int dim) {
    return dense_t_supported(dtype, n_q, Lq, n_d, Ld, dim) ? 1 : 0;
}

int msim_fwd_transposed_route(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim, float *scores,
                              int64_t ld_scores, int32_t *q_lengths, uint8_t *route, void *stream) {
    if (!route) return fail(MSIM_EINVAL, "null routing buffer");
    if (n_q > 0 && n_d > 0 && !dense_t_supported(dtype, n_q, Lq, n_d, Ld, dim))
        return fail(MSIM_EUNSUPPORTED, "msim_fwd_transposed_route: bf16 / f16, width %d, documents of at most %d rows, sizes below 2^31 bytes",
                    msim::kDim, msim::kDenseTMaxLd);
    return fwd_transposed(dtype, Q, n_q, Lq, D, n_d, Ld, dim, scores, ld_scores, q_lengths, route, stream);
}

size_t msim_dense_t_bwd_workspace_bytes(int n_q, int Lq, int n_d, int Ld, int dim) {
    (void)dim;
    if (n_q <= 0 || n_d <= 0 || Lq <= 0 || Ld <= 0) return 0;
    const DeviceInfo *di = nullptr;
    const int cus = device_info(&di) == MSIM_OK ? di->cus : 256;            // the plan only has to be the same in both calls
    return dense_t_plan(n_q, Lq, n_d, Ld, cus).bytes;
}

int msim_dense_t_bwd(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim, const float *G, int64_t ldg,
                     const void *g_scale, int g_scale_dtype, const uint8_t *route, void *dQ, void *dD, void *workspace, void *stream) {
    if (n_q < 0 || n_d < 0 || Lq <= 0 || Ld <= 0) return fail(MSIM_EINVAL, "negative or empty size");
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!Q || !D || !G || !route || !dQ || !dD || !workspace) return fail(MSIM_EINVAL, "null pointer argument");
    if (!dense_t_supported(dtype, n_q, Lq, n_d, Ld, dim))
        return fail(MSIM_EUNSUPPORTED, "msim_dense_t_bwd: bf16 / f16, width %d, documents of at most %d rows, sizes below 2^31 bytes",
                    msim::kDim, msim::kDenseTMaxLd);
    if (ldg < n_d) return fail(MSIM_EINVAL, "ldg < n_d");
    if (g_scale && g_scale_dtype != MSIM_DTYPE_BF16 && g_scale_dtype != MSIM_DTYPE_F16 && g_scale_dtype != MSIM_DTYPE_F32)
        return fail(MSIM_EINVAL, "g_scale dtype code %d", g_scale_dtype);
    if ((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D) | reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dD) |
         reinterpret_cast<uintptr_t>(workspace)) & 15)
        return fail(MSIM_EINVAL, "embeddings, gradients and workspace must be 16-byte aligned");
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const DenseTPlan pl = dense_t_plan(n_q, Lq, n_d, Ld, di->cus);
    msim::DenseTArgs a{};
    a.ldg = ldg;
    a.n_q = n_q;
    a.Lq = Lq;
    a.n_d = n_d;
    a.Ld = Ld;
    a.Lq_pad = msim::dense_t_lq_pad(Lq);
    a.ksp = a.Lq_pad / 32;
    a.n_split = pl.n_split;
    a.pages_per = pl.pages_per;
    if (msim::kAbBuild) {
        const char *e = getenv("MSIM_DENSE_T_DBG");
        a.dbg = e ? atoi(e) : 0;
        const char *o = getenv("MSIM_DENSE_T_DBG_OUT");
        a.dbg_out = o ? reinterpret_cast<unsigned long long *>(strtoull(o, nullptr, 0)) : nullptr;
    }
    const msim::GScale gs{g_scale, g_scale_dtype};
    const uint16_t *q = static_cast<const uint16_t *>(Q), *d = static_cast<const uint16_t *>(D);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == MSIM_DTYPE_F16
               ? dense_t_bwd_launch<true>(q, d, G, gs, route, static_cast<uint16_t *>(dQ), static_cast<uint16_t *>(dD),
                                          static_cast<char *>(workspace), pl, a, st)
               : dense_t_bwd_launch<false>(q, d, G, gs, route, static_cast<uint16_t *>(dQ), static_cast<uint16_t *>(dD),
                                           static_cast<char *>(workspace), pl, a, st);
}

// ---------------------------------------------------------------- pair lists (training losses)
int msim_pairs_argmax(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off,
                      const uint8_t *d_clamp0, int n_d, int dim, int max_doc_rows, const int32_t *pairs, int n_pairs,
                      float *out_scores, int32_t *out_argmax, void *stream) {
    if (n_q < 0 || n_d < 0 || Lq <= 0 || n_pairs < 0 || max_doc_rows < 0) return fail(MSIM_EINVAL, "negative size");
    if (n_pairs == 0) return MSIM_OK;
    if (!pairs) return fail(MSIM_EINVAL, "null pointer argument");
    if (int rc = check_common(Q, D, d_off, dtype, dim, Lq)) return rc;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const int tpq = (Lq + msim::kTokTile - 1) / msim::kTokTile;
    msim::PairsArgs a{n_q, Lq, n_d, n_pairs};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *q = static_cast<const uint16_t *>(Q), *d = static_cast<const uint16_t *>(D);
    // long queries x short documents in the tuned dtype / width (pages as queries, the trainer's symmetric direction): transposed form
    if (dtype != MSIM_DTYPE_F32 && dim == msim::kDim && Lq > kLongSegRows && max_doc_rows > 0 && max_doc_rows <= 4 * msim::kTokTile &&
        (long long)Lq * msim::kRowBytes < (1ll << 31)) {
        const int tpd = (max_doc_rows + msim::kTokTile - 1) / msim::kTokTile;
        return dtype == MSIM_DTYPE_F16
                   ? pairs_argmax_t_dispatch<true>(tpd, q, d, d_off, d_clamp0, pairs, out_scores, out_argmax, a, *di, st)
                   : pairs_argmax_t_dispatch<false>(tpd, q, d, d_off, d_clamp0, pairs, out_scores, out_argmax, a, *di, st);
    }
    if (!is_tuned(dtype, dim, Lq)) {
        const char *qc = static_cast<const char *>(Q), *dc = static_cast<const char *>(D);
        const int rb = dim * elem_bytes(dtype);
        switch (dtype) {
            case MSIM_DTYPE_F32:
                return generic_pairs_argmax<msim::kDtypeF32>(qc, dc, d_off, d_clamp0, pairs, out_scores, out_argmax, a, rb, *di, st);
            case MSIM_DTYPE_F16:
                return generic_pairs_argmax<msim::kDtypeF16>(qc, dc, d_off, d_clamp0, pairs, out_scores, out_argmax, a, rb, *di, st);
            default:
                return generic_pairs_argmax<msim::kDtypeBf16>(qc, dc, d_off, d_clamp0, pairs, out_scores, out_argmax, a, rb, *di, st);
        }
    }
    return dtype == MSIM_DTYPE_F16
               ? pairs_argmax_dispatch<true>(tpq, q, d, d_off, d_clamp0, pairs, out_scores, out_argmax, a, *di, st)
               : pairs_argmax_dispatch<false>(tpq, q, d, d_off, d_clamp0, pairs, out_scores, out_argmax, a, *di, st);
}

int msim_allpairs_argmax(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                         int n_d, int dim, float *out_scores, int64_t ld_scores, int32_t *out_argmax, void *stream) {
    if (n_q < 0 || n_d < 0 || Lq <= 0) return fail(MSIM_EINVAL, "negative size");
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!out_scores && !out_argmax) return fail(MSIM_EINVAL, "nothing to compute");
    if (out_scores && ld_scores < n_d) return fail(MSIM_EINVAL, "ld_scores < n_d");
    if (int rc = check_common(Q, D, d_off, dtype, dim, Lq)) return rc;
    if (!is_tuned(dtype, dim, Lq))
        return fail(MSIM_EUNSUPPORTED, "msim_allpairs_argmax takes bf16 / f16 embeddings of width %d and queries of at most %d tokens "
                    "(list the pairs and call msim_pairs_argmax otherwise)", msim::kDim, 4 * msim::kTokTile);
    if ((long long)n_q * n_d > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "more than 2^31 pairs");
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const int tpq = (Lq + msim::kTokTile - 1) / msim::kTokTile;
    msim::PairsArgs a{n_q, Lq, n_d, n_q * n_d};
    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint16_t *q = static_cast<const uint16_t *>(Q), *d = static_cast<const uint16_t *>(D);
    return dtype == MSIM_DTYPE_F16 ? allpairs_argmax_dispatch<true>(tpq, q, d, d_off, d_clamp0, out_scores, ld_scores, out_argmax, a, *di, st)
                                   : allpairs_argmax_dispatch<false>(tpq, q, d, d_off, d_clamp0, out_scores, ld_scores, out_argmax, a, *di, st);
}

size_t msim_pairs_bwd_workspace_bytes(int n_q, int Lq, int n_d, int dim, int max_doc_rows, int n_pairs) {
    (void)n_q;
    const DeviceInfo *di = nullptr;
    const int cus = device_info(&di) == MSIM_OK ? di->cus : 256;            // the plan only has to be the same in both calls
    return dd_plan(n_pairs, Lq, n_d, dim, max_doc_rows, cus).bytes;
}

int msim_pairs_bwd(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, int n_d, int dim,
                   int max_doc_rows, const int32_t *pairs, const int32_t *order_by_doc, const float *g,
                   const void *g_scale, int g_scale_dtype, const int32_t *argmax, int n_pairs, int out_dtype, void *dQ, void *dD,
                   void *workspace, void *stream) {
    if (n_q < 0 || n_d < 0 || Lq <= 0 || n_pairs < 0 || max_doc_rows < 0) return fail(MSIM_EINVAL, "negative size");
    if (!dQ || !dD) return fail(MSIM_EINVAL, "null pointer argument");
    if (n_pairs > 0 && (!pairs || !order_by_doc || !g || !argmax)) return fail(MSIM_EINVAL, "null pair-list argument");
    if (int rc = check_common(Q, D, d_off, dtype, dim, Lq)) return rc;
    if ((max_doc_rows + msim::kBwdRows - 1) / msim::kBwdRows > 65535)
        return fail(MSIM_EUNSUPPORTED, "max_doc_rows=%d too large", max_doc_rows);
    if (n_d > 0x7fffffff / 2) return fail(MSIM_EUNSUPPORTED, "too many documents");
    if (out_dtype != MSIM_DTYPE_F32 && out_dtype != dtype)
        return fail(MSIM_EINVAL, "gradients come out as fp32 or in the embeddings' own dtype (out_dtype %d, dtype %d)", out_dtype, dtype);
    if (g_scale && g_scale_dtype != MSIM_DTYPE_BF16 && g_scale_dtype != MSIM_DTYPE_F16 && g_scale_dtype != MSIM_DTYPE_F32)
        return fail(MSIM_EINVAL, "g_scale dtype code %d", g_scale_dtype);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::PairsArgs a{n_q, Lq, n_d, n_pairs};
    hipStream_t st = static_cast<hipStream_t>(stream);
    // short documents with long entry lists (the trainer's symmetric direction): the dense dD form, through the caller's scratch
    DdPlan pl;
    float *partial = static_cast<float *>(workspace);
    if (partial) {
        pl = dd_plan(n_pairs, Lq, n_d, dim, max_doc_rows, di->cus);
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(MSIM_EINVAL, "workspace must be 16-byte aligned");
    }
    const msim::GScale gs{g_scale, g_scale_dtype};
    const char *qc = static_cast<const char *>(Q), *dc = static_cast<const char *>(D);
    const bool out16 = out_dtype != MSIM_DTYPE_F32;
#define MSIM_BWD(DT, O16) \
    launch_bwd_kernels<DT, O16>(qc, dc, d_off, max_doc_rows, pairs, order_by_doc, g, argmax, dQ, dD, a, dim, di->cus, st, partial, pl, gs)
    if (dtype == MSIM_DTYPE_F32) MSIM_BWD(msim::kDtypeF32, false);
    else if (dtype == MSIM_DTYPE_F16) { if (out16) MSIM_BWD(msim::kDtypeF16, true); else MSIM_BWD(msim::kDtypeF16, false); }
    else { if (out16) MSIM_BWD(msim::kDtypeBf16, true); else MSIM_BWD(msim::kDtypeBf16, false); }
#undef MSIM_BWD
    return launch_failed("maxsim_pairs_bwd");
}

// ---------------------------------------------------------------- loss epilogue
// one workgroup reads the whole score matrix when it is small (loss_epilogue_small_kernel): no scratch, no ticket
static bool epilogue_is_small(int B, int C) { return B > 0 && B <= msim::kEpiSmallRows && (long long)B * C <= (1 << 18); }

size_t msim_loss_epilogue_workspace_bytes(int B, int C) {
    if (epilogue_is_small(B, C)) return 0;
    return B > 0 ? 16 + (size_t)3 * B * sizeof(float) : 16;
}

int msim_loss_epilogue(int mode, const float *scores, int64_t ld, int B, int C, const void *Q, int q_dtype, int Lq, int width,
                       int offset, float temperature, int normalize, int filter, float filter_threshold, float filter_factor,
                       float *G, int32_t *pairs, float *coef, int32_t *order, void *workspace, float *out, void *loss_out,
                       const int32_t *q_lengths, void *stream) {
    if (B < 0 || C < 0 || Lq < 0 || width <= 0) return fail(MSIM_EINVAL, "negative size");
    if (mode != MSIM_LOSS_PAIRWISE && mode != MSIM_LOSS_INFONCE && mode != MSIM_LOSS_SIGMOID) return fail(MSIM_EINVAL, "unknown loss mode %d", mode);
    if (mode == MSIM_LOSS_SIGMOID && C != B)
        return fail(MSIM_EINVAL, "the sigmoid loss is defined on the in-batch square: %d queries, %d documents", B, C);
    if (!scores || !Q || !out) return fail(MSIM_EINVAL, "null pointer argument");
    if (q_dtype != MSIM_DTYPE_BF16 && q_dtype != MSIM_DTYPE_F16 && q_dtype != MSIM_DTYPE_F32)
        return fail(MSIM_EUNSUPPORTED, "dtype code %d", q_dtype);
    if (B == 0) return fail(MSIM_EINVAL, "empty batch");
    if (offset < 0 || (long long)offset + B > C) return fail(MSIM_EINVAL, "offset %d + batch %d exceeds the %d documents", offset, B, C);
    if (ld < C) return fail(MSIM_EINVAL, "ld=%lld < C=%d", (long long)ld, C);
    if (temperature == 0.0f) return fail(MSIM_EINVAL, "temperature must be non-zero");
    if (mode == MSIM_LOSS_PAIRWISE) {
        if (C < 2) return fail(MSIM_EINVAL, "the pairwise loss needs at least 2 documents (topk(2))");
        if (!pairs || !coef || !order) return fail(MSIM_EINVAL, "null pair-list output");
    }
    const bool small = epilogue_is_small(B, C);
    if (!small && !workspace) return fail(MSIM_EINVAL, "this batch needs msim_loss_epilogue_workspace_bytes(B, C) bytes of zero-filled scratch");
    if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15)) return fail(MSIM_EINVAL, "workspace must be 16-byte aligned");
    msim::EpiArgs a;
    a.ld = ld;
    a.B = B;
    a.C = C;
    a.Lq = Lq;
    a.q_elem_bytes = elem_bytes(q_dtype);
    a.q_is_f16 = q_dtype == MSIM_DTYPE_F16;
    a.q_row_bytes = width * a.q_elem_bytes;
    a.offset = offset;
    a.mode = mode == MSIM_LOSS_PAIRWISE ? msim::kEpiPairwise : mode == MSIM_LOSS_SIGMOID ? msim::kEpiSigmoid : msim::kEpiInfoNCE;
    a.normalize = normalize != 0;
    a.filter = filter != 0;
    a.inv_T = 1.0f / temperature;
    a.filter_threshold = filter_threshold;
    a.filter_factor = filter_factor;
    if (small) {
        const int staged = (long long)B * C <= msim::kEpiStageFloats;
        const int lds = staged ? B * C * (int)sizeof(float) : 0;
        static std::atomic<int> configured[kMaxDevices];
        if (int rc = allow_lds(msim::loss_epilogue_small_kernel, msim::kEpiStageFloats * (int)sizeof(float), configured)) return rc;
        hipLaunchKernelGGL(msim::loss_epilogue_small_kernel, dim3(1), dim3(msim::kEpiSmallThreads), lds, static_cast<hipStream_t>(stream),
                           scores, static_cast<const char *>(Q), q_lengths, G, pairs, coef, order, out, loss_out, a, staged);
    } else {
        char *ws = static_cast<char *>(workspace);
        hipLaunchKernelGGL(msim::loss_epilogue_kernel, dim3(B), dim3(msim::kEpiThreads), 0, static_cast<hipStream_t>(stream), scores,
                           static_cast<const char *>(Q), G, pairs, coef, order, reinterpret_cast<float *>(ws + 16),
                           reinterpret_cast<unsigned int *>(ws), out, loss_out, q_lengths, a);
    }
    return launch_failed("loss_epilogue_kernel");
}

// ---------------------------------------------------------------- smooth-max entry points
int msim_smooth_fwd(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, int n_d, int dim, float tau,
                    float *scores, int64_t ld_scores, void *stream) {
    if (n_q < 0 || n_d < 0) return fail(MSIM_EINVAL, "negative size (n_q=%d n_d=%d)", n_q, n_d);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!scores) return fail(MSIM_EINVAL, "null pointer argument");
    if (int rc = check_smooth(Q, D, d_off, dtype, dim, Lq, tau)) return rc;
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "ld_scores=%lld < n_d=%d", (long long)ld_scores, n_d);
    GenericCall c;
    if (int rc = device_info(&c.di)) return rc;
    c.Q = static_cast<const char *>(Q);
    c.D = static_cast<const char *>(D);
    c.d_off = d_off;
    c.clamp0 = nullptr;
    c.scores = scores;
    c.ld = ld_scores;
    c.n_q = n_q;
    c.Lq = Lq;
    c.n_d = n_d;
    c.row_bytes = dim * elem_bytes(dtype);
    c.flags = 0;
    c.st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case MSIM_DTYPE_F32: return smooth_dispatch<msim::kDtypeF32>(c, tau);
        case MSIM_DTYPE_F16: return smooth_dispatch<msim::kDtypeF16>(c, tau);
        default: return smooth_dispatch<msim::kDtypeBf16>(c, tau);
    }
}

}  // extern "C"

namespace {
template <int TPQ, bool F16>
int launch_smooth_pairs_stream(const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const int32_t *pairs, float *out_scores,
                               float *out_lse, const msim::PairsArgs &a, float tau, const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::maxsim_smooth_pairs_stream_kernel<TPQ, F16>;
    constexpr int lds = 4 * msim::kPairsRing * msim::kSlabBytes;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    const int wg_needed = (a.n_pairs + 3) / 4;
    const int wg_cap = di.cus * (di.lds_per_cu / lds);
    hipLaunchKernelGGL(kern, dim3(wg_needed < wg_cap ? wg_needed : wg_cap), dim3(256), lds, st, Q, D, d_off, pairs, out_scores, out_lse,
                       a, tau);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_smooth_pairs_stream_kernel<%d> launch: %s", TPQ, hipGetErrorString(e));
    return MSIM_OK;
}
template <bool F16>
int smooth_pairs_stream_dispatch(int tpq, const uint16_t *Q, const uint16_t *D, const int32_t *d_off, const int32_t *pairs,
                                 float *out_scores, float *out_lse, const msim::PairsArgs &a, float tau, const DeviceInfo &di,
                                 hipStream_t st) {
    switch (tpq) {
        case 1: return launch_smooth_pairs_stream<1, F16>(Q, D, d_off, pairs, out_scores, out_lse, a, tau, di, st);
        case 2: return launch_smooth_pairs_stream<2, F16>(Q, D, d_off, pairs, out_scores, out_lse, a, tau, di, st);
        case 3: return launch_smooth_pairs_stream<3, F16>(Q, D, d_off, pairs, out_scores, out_lse, a, tau, di, st);
        default: return launch_smooth_pairs_stream<4, F16>(Q, D, d_off, pairs, out_scores, out_lse, a, tau, di, st);
    }
}
}  // namespace

extern "C" {

int msim_smooth_pairs(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, int n_d, int dim,
                      const int32_t *pairs, int n_pairs, float tau, float *out_scores, float *out_lse, void *stream) {
    if (n_q < 0 || n_d < 0 || n_pairs < 0) return fail(MSIM_EINVAL, "negative size");
    if (n_pairs == 0) return MSIM_OK;
    if (!pairs) return fail(MSIM_EINVAL, "null pointer argument");
    if (int rc = check_smooth(Q, D, d_off, dtype, dim, Lq, tau)) return rc;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::PairsArgs a{n_q, Lq, n_d, n_pairs};
    const char *qc = static_cast<const char *>(Q), *dc = static_cast<const char *>(D);
    const int rb = dim * elem_bytes(dtype);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int tpq = (Lq + msim::kTokTile - 1) / msim::kTokTile;
    if (dim == msim::kDim && dtype != MSIM_DTYPE_F32 && tpq <= 4) {   // 128 x 16-bit rows: the LDS-DMA pipeline
        const uint16_t *q16 = static_cast<const uint16_t *>(Q), *d16 = static_cast<const uint16_t *>(D);
        return dtype == MSIM_DTYPE_F16 ? smooth_pairs_stream_dispatch<true>(tpq, q16, d16, d_off, pairs, out_scores, out_lse, a, tau, *di, st)
                                       : smooth_pairs_stream_dispatch<false>(tpq, q16, d16, d_off, pairs, out_scores, out_lse, a, tau, *di, st);
    }
    switch (dtype) {
        case MSIM_DTYPE_F32: return smooth_pairs<msim::kDtypeF32>(qc, dc, d_off, pairs, out_scores, out_lse, a, rb, tau, *di, st);
        case MSIM_DTYPE_F16: return smooth_pairs<msim::kDtypeF16>(qc, dc, d_off, pairs, out_scores, out_lse, a, rb, tau, *di, st);
        default: return smooth_pairs<msim::kDtypeBf16>(qc, dc, d_off, pairs, out_scores, out_lse, a, rb, tau, *di, st);
    }
}

size_t msim_smooth_bwd_workspace_bytes(int n_q, int Lq, int dim) {
    const DeviceInfo *di = nullptr;
    if (n_q <= 0 || Lq <= 0 || dim <= 0 || device_info(&di)) return 0;
    const int ns = smooth_dq_split(n_q, Lq, *di);
    return ns > 1 ? (size_t)ns * n_q * Lq * dim * sizeof(float) : 0;
}

int msim_smooth_pairs_bwd(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, int n_d, int dim,
                          int max_doc_rows, const int32_t *pairs, const int32_t *order_by_doc, const float *g, const float *lse,
                          int n_pairs, float tau, float *dQ, float *dD, void *workspace, void *stream) {
    if (n_q < 0 || n_d < 0 || n_pairs < 0 || max_doc_rows < 0) return fail(MSIM_EINVAL, "negative size");
    if (!dQ || !dD) return fail(MSIM_EINVAL, "null pointer argument");
    if (n_pairs > 0 && (!pairs || !order_by_doc || !g || !lse)) return fail(MSIM_EINVAL, "null pair-list argument");
    if (int rc = check_smooth(Q, D, d_off, dtype, dim, Lq, tau)) return rc;
    if ((max_doc_rows + 31) / 32 > 65535) return fail(MSIM_EUNSUPPORTED, "max_doc_rows=%d too large", max_doc_rows);
    if ((Lq + 31) / 32 > 65535) return fail(MSIM_EUNSUPPORTED, "Lq=%d too large", Lq);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const int ns = smooth_dq_split(n_q, Lq, *di);
    if (ns > 1 && !workspace) return fail(MSIM_EINVAL, "workspace required (msim_smooth_bwd_workspace_bytes)");
    if ((reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dD) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return fail(MSIM_EINVAL, "dQ, dD and the workspace must be 16-byte aligned");
    msim::SmoothBwdArgs a{n_q, Lq, n_d, n_pairs, dim * elem_bytes(dtype), dim, tau, 1};
    const char *qc = static_cast<const char *>(Q), *dc = static_cast<const char *>(D);
    float *ws = static_cast<float *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case MSIM_DTYPE_F32: return smooth_bwd<msim::kDtypeF32>(qc, dc, d_off, max_doc_rows, pairs, order_by_doc, g, lse, dQ, dD, ws, a, ns, st);
        case MSIM_DTYPE_F16: return smooth_bwd<msim::kDtypeF16>(qc, dc, d_off, max_doc_rows, pairs, order_by_doc, g, lse, dQ, dD, ws, a, ns, st);
        default: return smooth_bwd<msim::kDtypeBf16>(qc, dc, d_off, max_doc_rows, pairs, order_by_doc, g, lse, dQ, dD, ws, a, ns, st);
    }
}

}  // extern "C"
