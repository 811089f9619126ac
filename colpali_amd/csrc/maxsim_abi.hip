// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): the forward scorers -- msim_fwd, msim_fwd_ragged and their plans and
// workspace sizes (and their forms over the 13-bit image of a bf16 corpus: msim_fwd_pack13, msim_fwd_ragged_pack13), the plain similarity matrix, msim_query_compact and candidate reranking (msim_fwd_candidates, both widths).
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates,
// frees or synchronises, so every entry point is hipGraph-capturable.  The other families of entry points live in abi_train.hip,
// abi_head_pool.hip, abi_search.hip and abi_index.hip, the state they share in abi_core.cpp; the kernels included below are
// defined and launched in this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "abi_shapes.hpp"
#include "maxsim_stream.hip"
#include "maxsim_stream13.hip"
#include "maxsim_batch.hip"
#if defined(MSIM_AB) || defined(MSIM_TRACE)
#include "maxsim_batch_packed.hip"     // K1bK: several short documents per chunk -- measured, slower than K1b, measurement builds only
#endif
#include "maxsim_generic.hip"
#include "maxsim_panels.hip"
#include "maxsim_candidates.hip"
#include "maxsim_candidates_panels.hip"
#include "query_compact.hip"

using namespace msim_abi;

namespace {

// the 13-bit image of the corpus (pack13.hip) beside the blob: K1s plans of bf16 calls scan it instead
struct Pack13View {
    const uint8_t *image;
    const int32_t *slab_off;
    const uint8_t *flagged;
    const int32_t *list;         // the flagged ids, n_list of them: scored from the blob
    int n_list;
};

struct FwdCall {
    const uint16_t *Q, *D;       // Q: the [n_q, Lq, 128] box (uniform queries: also a flat token matrix) or the flat token matrix (q_off)
    const int32_t *d_off;
    const uint8_t *clamp0;
    float *scores;
    long long ld;
    int n_q, Lq, n_d;
    unsigned flags;
    const DeviceInfo *di;
    hipStream_t st;
    void *workspace = nullptr;   // msim_fwd_workspace_bytes() bytes or null
    // the flat token layout (maxsim_common.hpp)
    const int32_t *q_off = nullptr;        // device: token offsets [n_q + 1]; null = uniform queries of Lq tokens
    const int32_t *q_off_host = nullptr;   // the same numbers on the host: the plan below is made from them
    int seg = 0, n_seg = 1;                // uniform long queries: n_q counts PIECES of `seg` tokens (FlatQ::n_seg)
    int avg_rows = 0;                      // the caller's hint: average rows per document (MSIM_FLAG_AVG_ROWS), 0 = unknown
    const Pack13View *p13 = nullptr;       // bf16 only
};

constexpr size_t kFwdWorkspaceBytes = 4096;   // K1b's convoy counters: n_ranges * n_qblocks <= 8 * 64 ints

constexpr int kStreamRing = 4;  // default slabs per wave-private ring: 4 waves x 4 x 8 KiB = 128 KiB per workgroup (launch_stream picks 2 for 5-8 units)

// host mirror of msim::flat_qoff
struct HostQ {
    const int32_t *off;
    int Lq, seg, n_seg;
    int at(int i) const {
        if (off) return off[i];
        if (n_seg <= 1) return i * Lq;
        const int r = i / n_seg, s = i - r * n_seg;
        const int o = s * seg;
        return r * Lq + (o < Lq ? o : Lq);
    }
};
HostQ host_q(const FwdCall &c) { return HostQ{c.q_off_host, c.Lq, c.seg, c.n_seg}; }
msim::FlatQ flat_q(const FwdCall &c) { return msim::FlatQ{c.q_off, c.Lq, c.seg, c.n_seg}; }

// Cache policy of K1s's document stream: every byte is read once by one CU, so the LDS-DMA loads carry `nt`
// (do not allocate in L2 / MALL).  Measured on MI355X, 16 GiB shard: 6.31 -> 7.02 TB/s at 1 query, 6.08 -> 6.45 TB/s
// at 4 queries.  MSIM_STREAM_NT=0 switches it off (AUX = 0) for A/B measurements (tuning knob, not part of the ABI).
int stream_nt() {
    static const int v = ab_env("MSIM_STREAM_NT", 1) != 0;
    return v;
}

// what the launches of the K1s family share: the kernel arguments taken from the call, and the grid -- one wave per document, four
// waves per workgroup, never more workgroups than are resident at once (the waves walk the documents grid-stride)
msim::StreamArgs stream_args(const FwdCall &c) {
    msim::StreamArgs a;
    a.ld = c.ld;
    a.fq = flat_q(c);
    a.n_q = c.n_q;
    a.n_d = c.n_d;
    a.flags = c.flags;
#ifdef MSIM_TRACE
    a.trace = nullptr;
    if (const char *tp = getenv("MSIM_STREAM_TRACE_PTR")) a.trace = reinterpret_cast<unsigned long long *>(strtoull(tp, nullptr, 0));
#endif
    return a;
}
dim3 stream_grid(const FwdCall &c, int lds) {
    const int wg_needed = (c.n_d + 3) / 4;
    const int wg_cap = c.di->cus * (c.di->lds_per_cu / lds);
    return dim3(wg_needed < wg_cap ? wg_needed : wg_cap);
}

// MSIM_STREAM_ORDER=0..4 / MSIM_STREAM_ORDER_RAW=0..4 (measurement builds): the slab body's request order of the 2-slot forms
// (maxsim_stream.hip: hook, early, paced, split, paced half) in K1s13 / in raw K1s; the shipped library has DEFAULT and nothing else
template <int RING, int DEFAULT, class Launch>
int dispatch_order(int forced, Launch &&launch) {
#if defined(MSIM_AB) || defined(MSIM_TRACE)
    if constexpr (RING == 2) {
        switch (forced) {
            case msim::kOrderHook: return launch(std::integral_constant<int, msim::kOrderHook>{});
            case msim::kOrderEarly: return launch(std::integral_constant<int, msim::kOrderEarly>{});
            case msim::kOrderPaced: return launch(std::integral_constant<int, msim::kOrderPaced>{});
            case msim::kOrderSplit: return launch(std::integral_constant<int, msim::kOrderSplit>{});
            case msim::kOrderPacedHalf: return launch(std::integral_constant<int, msim::kOrderPacedHalf>{});
            default: break;
        }
    }
#endif
    (void)forced;
    return launch(std::integral_constant<int, DEFAULT>{});
}

// LIST: the documents doc_list[0 .. c.n_d) instead of 0 .. c.n_d-1
template <int NU, bool F16, int AUX, int RING, bool LIST, int ORDER>
int launch_stream_order(const FwdCall &c, const int32_t *doc_list) {
    auto kern = msim::maxsim_stream_kernel<NU, RING, F16, AUX, LIST, ORDER>;
    constexpr int lds = 4 * (RING * msim::kSlabBytes + msim::kStreamTokBytes);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    hipLaunchKernelGGL(kern, stream_grid(c, lds), dim3(256), lds, c.st, c.Q, c.D, c.d_off, c.clamp0, c.scores, stream_args(c),
                       doc_list);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_stream_kernel<%d> launch: %s", NU, hipGetErrorString(e));
    return MSIM_OK;
}
template <int NU, bool F16, int AUX, int RING = kStreamRing, bool LIST = false>
int launch_stream_aux(const FwdCall &c, const int32_t *doc_list = nullptr) {
    static const int forced = ab_env("MSIM_STREAM_ORDER_RAW", -1);
    return dispatch_order<RING, msim::stream_order(RING)>(
        forced, [&](auto order) { return launch_stream_order<NU, F16, AUX, RING, LIST, decltype(order)::value>(c, doc_list); });
}

template <int NU, bool F16>
int launch_stream(const FwdCall &c) {
    // 5-8 units (3-4 token tiles of 32): a 2-slab ring (72 KiB per workgroup) lets TWO workgroups share a CU -- two waves per SIMD,
    // one covering the other's DMA issue / operand reads / max folds: 4 queries 6.51-6.55 -> 6.82 TB/s (85 % of spec); up to 4 units
    // are at the stream ceiling either way and keep the deeper ring.  In the compiled body the eight requests of the next slab stand
    // in one block behind the last operand read (maxsim_stream.hip: ORDER, hook), not one per NU MFMAs; pinning them there is a tie.
    // MSIM_STREAM_RING=2|4 forces one of them (tuning knob, not part of the ABI).
    constexpr int ring_default = NU >= 5 ? 2 : kStreamRing;
#ifdef MSIM_AB
    {
        static const int ring_env = ab_env("MSIM_STREAM_RING", 0);
        const int ring = ring_env ? ring_env : ring_default;
        if (ring == 2) return launch_stream_aux<NU, F16, 2, 2>(c);
        return stream_nt() ? launch_stream_aux<NU, F16, 2>(c) : launch_stream_aux<NU, F16, 0>(c);
    }
#endif
    return launch_stream_aux<NU, F16, 2, ring_default>(c);     // nt stream
}

// K1s over the 13-bit image (maxsim_stream13.hip): the same ring depths and grid rule as launch_stream -- 2 slabs of 6.5 KiB for 5-8
// units (60.25 KiB per workgroup: two per CU; the next slab's requests pinned one per NU / 2 MFMAs: maxsim_stream.hip, ORDER, paced
// half; the two waves of a SIMD swap s_setprio every 32 slabs: maxsim_stream13.hip, PRIO), 4 slabs below.  The documents the encoder flagged are skipped there and scored
// from the blob by the raw K1s over their id list, into the same score columns; that launch exists only when the list is not empty.
template <int NU, int RING, int ORDER, int DECODE = msim::stream13_decode(), int PRIO = msim::stream13_prio(RING)>
int launch_stream13_order(const FwdCall &c) {
    auto kern = msim::maxsim_stream13_kernel<NU, RING, 2, ORDER, DECODE, PRIO>;
    constexpr int lds = 4 * (RING * msim::kSlab13Bytes + msim::kStreamTokBytes);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    hipLaunchKernelGGL(kern, stream_grid(c, lds), dim3(256), lds, c.st, c.Q, c.d_off, c.clamp0, c.scores, stream_args(c),
                       c.p13->image, c.p13->slab_off, c.p13->flagged);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_stream13_kernel<%d> launch: %s", NU, hipGetErrorString(e));
    if (c.p13->n_list > 0) {
        FwdCall l = c;
        l.n_d = c.p13->n_list;
        return launch_stream_aux<NU, false, 2, RING, true>(l, c.p13->list);
    }
    return MSIM_OK;
}
// MSIM_STREAM13_DECODE=0|1 / MSIM_STREAM13_PRIO=0..3 (measurement builds): how the high bytes are decoded (maxsim_stream13.hip: or3, bfi)
// and how the two waves of a SIMD share its vector issue (none, doc, slabs, static; 2-slot forms only), at the shipped request order
template <int NU, int RING, int ORDER>
int launch_stream13_issue(const FwdCall &c) {
#if defined(MSIM_AB) || defined(MSIM_TRACE)
    static const int decode = ab_env("MSIM_STREAM13_DECODE", msim::stream13_decode());
    static const int prio = RING == 2 ? ab_env("MSIM_STREAM13_PRIO", msim::stream13_prio(RING)) : msim::kPrioNone;
    if constexpr (ORDER == msim::stream13_order(RING)) {
        auto with_prio = [&](auto dec) {
            constexpr int D = decltype(dec)::value;
            if constexpr (RING == 2) {
                switch (prio) {
                    case msim::kPrioDoc: return launch_stream13_order<NU, RING, ORDER, D, msim::kPrioDoc>(c);
                    case msim::kPrioSlabs: return launch_stream13_order<NU, RING, ORDER, D, msim::kPrioSlabs>(c);
                    case msim::kPrioStatic: return launch_stream13_order<NU, RING, ORDER, D, msim::kPrioStatic>(c);
                    default: break;
                }
            }
            return launch_stream13_order<NU, RING, ORDER, D, msim::kPrioNone>(c);
        };
        return decode == msim::kDecodeOr3 ? with_prio(std::integral_constant<int, msim::kDecodeOr3>{})
                                          : with_prio(std::integral_constant<int, msim::kDecodeBfi>{});
    }
#endif
    return launch_stream13_order<NU, RING, ORDER>(c);
}
template <int NU>
int launch_stream13(const FwdCall &c) {
    constexpr int RING = NU >= 5 ? 2 : kStreamRing;
    static const int forced = ab_env("MSIM_STREAM_ORDER", -1);
    return dispatch_order<RING, msim::stream13_order(RING)>(forced, [&](auto order) { return launch_stream13_issue<NU, RING, decltype(order)::value>(c); });
}

// K1s holds 1..8 units: launch(std::integral_constant<int, NU>) for the plan's count
template <class Launch>
int dispatch_units(int nu, Launch &&launch) {
    switch (nu) {
        case 1: return launch(std::integral_constant<int, 1>{});
        case 2: return launch(std::integral_constant<int, 2>{});
        case 3: return launch(std::integral_constant<int, 3>{});
        case 4: return launch(std::integral_constant<int, 4>{});
        case 5: return launch(std::integral_constant<int, 5>{});
        case 6: return launch(std::integral_constant<int, 6>{});
        case 7: return launch(std::integral_constant<int, 7>{});
        default: return launch(std::integral_constant<int, 8>{});
    }
}

// ---- the plan of one tuned forward call, made on the host from the queries' lengths -- ONE definition, shared by the dispatch and
// by msim_fwd_workspace_bytes (which must report scratch exactly when the launch would use it: round-2 advisor finding).
//   * up to 8 queries / 8 units (128 tokens) in total: K1s, every wave holds all units (HBM-bound regime, one pass over the corpus,
//     no barriers at all);
//   * more: K1b, whose query blocks hold WHOLE queries -- at most nw * maxu units of tokens and nw * 8 queries (one 8-lane group of the
//     workgroup per query in the reduction).  One block if the batch fits one of the six shapes
//         units <= 16: pair (2 waves) | <= 20: 4 waves x 5 units, three workgroups per CU | <= 32: 4 waves | <= 40: 4 waves x 10 | <= 64: 8 waves | <= 80: 8 x 10
//     (the measured ladder of rounds 2-3 in 16-token units: profiles/r02_logs/ab_ridge.log, r03_logs/ab_batch_t5.log,
//     ab_batch8_final.log), else several blocks on the 8-wave form, filled greedily in query order and then re-cut evenly; eight or
//     ten units per wave by cost: a block's pace is set by its heaviest wave, so a plan costs (blocks) x (units of the heaviest
//     wave), and the ten-unit bodies run ~10 % behind the eight-unit ones per step.
struct FlatPlan {
    bool stream = false;
    int nu = 0;                   // K1s: units per wave
    int nw = 0, maxu = 0;         // K1b
    std::vector<int> blk_q0;      // K1b: first query of every block, + n_q
    int n_blocks() const { return (int)blk_q0.size() - 1; }
};

// greedy fill in query order under (token, query) capacities; false if one query alone exceeds a block
bool fill_blocks(const HostQ &hq, int n_q, int nw, int maxu, std::vector<int> &blk) {
    const int cap_tok = nw * maxu * msim::kUnitTok, cap_q = nw * 8;
    blk.clear();
    blk.push_back(0);
    int cur_tok = 0, cur_q = 0;
    for (int i = 0; i < n_q; ++i) {
        const int len = hq.at(i + 1) - hq.at(i);
        if (len > cap_tok) return false;
        if (cur_q == cap_q || cur_tok + len > cap_tok) {
            blk.push_back(i);
            cur_tok = 0;
            cur_q = 0;
        }
        cur_tok += len;
        ++cur_q;
    }
    blk.push_back(n_q);
    return true;
}

// the same number of blocks, cut evenly by tokens (a block's pace is its heaviest wave: 31 + 32 + 31 + ... beats 32 + 32 + ... + 8);
// kept only if every block still fits
void balance_blocks(const HostQ &hq, int n_q, int nw, int maxu, std::vector<int> &blk) {
    const int nb = (int)blk.size() - 1;
    if (nb <= 1) return;
    const int cap_tok = nw * maxu * msim::kUnitTok, cap_q = nw * 8;
    const long long base = hq.at(0), total = (long long)hq.at(n_q) - base;
    std::vector<int> cut(1, 0);
    int q = 0;
    for (int b = 1; b < nb; ++b) {
        const long long want = (total * b + nb - 1) / nb;         // tokens in front of block b
        while (q < n_q && (long long)hq.at(q) - base < want) ++q;
        if (q <= cut.back()) q = cut.back() + 1;
        if (q >= n_q) return;
        cut.push_back(q);
    }
    cut.push_back(n_q);
    for (int b = 0; b < nb; ++b)
        if (hq.at(cut[b + 1]) - hq.at(cut[b]) > cap_tok || cut[b + 1] - cut[b] > cap_q) return;
    blk.swap(cut);
}

int heaviest_wave_units(const HostQ &hq, const std::vector<int> &blk, int nw) {
    int worst = 0;
    for (size_t b = 0; b + 1 < blk.size(); ++b) {
        const int units = (hq.at(blk[b + 1]) - hq.at(blk[b]) + msim::kUnitTok - 1) / msim::kUnitTok;
        const int w = (units + nw - 1) / nw;
        if (w > worst) worst = w;
    }
    return worst;
}

// MSIM_BATCH_NW=2|4|8 forces the number of waves that share a document stream in K1b (tuning knob for A/B measurements, not
// part of the ABI)
int batch_nw_override() {
    static const int v = [] {
        const int x = ab_env("MSIM_BATCH_NW", 0);
        return (x == 2 || x == 4 || x == 8) ? x : 0;
    }();
    return v;
}

int flat_plan(const HostQ &hq, int n_q, FlatPlan &p) {
    const long long tokens = (long long)hq.at(n_q) - hq.at(0);
    if (tokens < 0) return fail(MSIM_EINVAL, "query token offsets are not non-decreasing");
    const long long units = (tokens + msim::kUnitTok - 1) / msim::kUnitTok;
    p = FlatPlan{};
    if (n_q <= 8 && units <= 8) {
        p.stream = true;
        p.nu = units > 0 ? (int)units : 1;
        return MSIM_OK;
    }
    static const int shapes[7][2] = {{2, 8}, {4, 5}, {2, 10}, {4, 8}, {4, 10}, {8, 8}, {8, 10}};
    // round 4 re-measured the ladder in units (profiles/r04_logs/ab_plan_ladder.log, 16 GiB shard, random rows / zero-filled shard):
    // 18 units: pair x 10 (9 + 9) 4.12 ms / 2.97 vs 4 waves (5/5/4/4) 4.23 / 2.99; 20 units: 4 waves x 5 units 4.38 / 3.04 vs the
    // pair 4.42-4.45 / 3.19 -- four evenly loaded waves beat two ten-unit ones once the units divide by four.  Then the FIVE-unit
    // form of the 4-wave shape: a kernel that never holds more than five units needs 168 registers, so THREE workgroups share a CU
    // (three waves per SIMD; 2-chunk ring, 37.5 KiB of LDS each) -- 17..20 units: 9 queries 4.02 -> 3.98 ms, 10 queries 4.25 -> 4.13
    // (zero shard 0.726 -> 0.747, 0.731 -> 0.740), bit-identical (profiles/r04_logs/ab_five_units_3wg.log; with the 3-chunk ring the
    // third workgroup does not fit the LDS and it is slower than the two-workgroup form).  The pair x 10 shape is a measurement-build
    // shape since
    const int forced = batch_nw_override();
    static const int forced_maxu = ab_env("MSIM_BATCH_MAXU", 0);      // 8 | 10 (measurement builds)
#ifdef MSIM_AB
    // measurement builds only (next lead): the five-unit instantiation of the PAIR form -- six pairs per CU
    if (forced == 2 && forced_maxu == 5 && units <= 10 && n_q <= 16 && fill_blocks(hq, n_q, 2, 5, p.blk_q0) && p.n_blocks() == 1) {
        p.nw = 2;
        p.maxu = 5;
        return MSIM_OK;
    }
#endif
    for (const auto &sh : shapes) {
        if (forced && sh[0] != forced) continue;
        if (forced_maxu && sh[1] != forced_maxu) continue;
        if (units > sh[0] * sh[1] || n_q > sh[0] * 8) continue;
        if (sh[0] == 2 && sh[1] == 10 && !(forced == 2 || forced_maxu == 10)) continue;       // superseded by {4, 5}: measurement builds only
        if (!fill_blocks(hq, n_q, sh[0], sh[1], p.blk_q0) || p.n_blocks() != 1) continue;
        p.nw = sh[0];
        p.maxu = sh[1];
        return MSIM_OK;
    }
#ifdef MSIM_AB
    // measurement builds only (round 5, short documents): several blocks on the FOUR-wave form -- two workgroups per CU, 64-row chunks,
    // one covering the other's per-document barriers -- instead of the eight-wave form (MSIM_BATCH_NW=4 with more than 40 units)
    if (forced == 4) {
        std::vector<int> b4;
        if (fill_blocks(hq, n_q, 4, 8, b4)) {
            balance_blocks(hq, n_q, 4, 8, b4);
            p.nw = 4;
            p.maxu = 8;
            p.blk_q0.swap(b4);
            return MSIM_OK;
        }
    }
#endif
    std::vector<int> b8, b10;
    if (!fill_blocks(hq, n_q, 8, 8, b8)) {
        if (!fill_blocks(hq, n_q, 8, 10, b10))
            return fail(MSIM_EUNSUPPORTED, "a query of more than %d tokens does not fit one query block", 8 * 10 * msim::kUnitTok);
        balance_blocks(hq, n_q, 8, 10, b10);
        p.nw = 8;
        p.maxu = 10;
        p.blk_q0.swap(b10);
        return MSIM_OK;
    }
    balance_blocks(hq, n_q, 8, 8, b8);
    p.nw = 8;
    p.maxu = 8;
    if (fill_blocks(hq, n_q, 8, 10, b10)) {
        balance_blocks(hq, n_q, 8, 10, b10);
        const long long c8 = (long long)(b8.size() - 1) * heaviest_wave_units(hq, b8, 8);
        const long long c10 = (long long)(b10.size() - 1) * heaviest_wave_units(hq, b10, 8);
        // ... or no slower AND the only one whose blocks are all resident at once (32 CUs per XCD on MI355X: one document range per
        // XCD, held together by the convoy, every corpus byte read from HBM once).  1000 queries x 40 tokens: 40 blocks of 64 units
        // run as four ranges x five rounds and read the corpus TWICE (PMC: 66.5 GB for 33.3 GB); 32 blocks of 80 units read it once
        // in the same time (99.3 vs 99.4-99.8 ms, profiles/r06_logs/ab_short_docs_packed.log section 7)
        // (a one-round plan takes as long as its heaviest wave whatever the number of blocks: only when the round is full, 31 or 32
        // blocks -- with 28 ten-unit blocks four CUs per XCD idle and the eight-unit plan's sub-ranges win by 13 %)
        const bool single_round10 = b10.size() - 1 <= 32 && b10.size() - 1 >= 31 && b8.size() - 1 > 32;
        if (11 * c10 < 10 * c8 || (c10 <= c8 && single_round10)) {
            p.maxu = 10;
            p.blk_q0.swap(b10);
            return MSIM_OK;
        }
    }
    p.blk_q0.swap(b8);
    return MSIM_OK;
}

// document ranges per XCD of a K1b / K1bPF launch (the rule is explained where launch_batch calls it): one block -> one range per
// resident workgroup; several blocks -> the smallest number of ranges whose last round of resident workgroups is >= 97 % full, else the
// fullest; never ranges of fewer than `min_docs` documents (~2000 rows by the caller's MSIM_FLAG_AVG_ROWS hint, 64 documents without it)
int ranges_per_xcd(int n_qblocks, int cus_per_xcd, int n_d, int avg_rows) {
    int min_docs = 64;
    if (avg_rows > 0) {
        min_docs = (2048 + avg_rows - 1) / avg_rows;
        min_docs = min_docs < 2 ? 2 : (min_docs > 64 ? 64 : min_docs);
    }
    int sub = n_qblocks >= cus_per_xcd ? 1 : cus_per_xcd / n_qblocks;
    if (n_qblocks > 1) {
        double best = 0.0;
        int best_sub = 1;
        for (int s = 1; s <= 32; ++s) {
            if (s > 1 && (long long)8 * s * min_docs > n_d) break;
            const long long slots_x = (long long)n_qblocks * s;
            const long long rounds = (slots_x + cus_per_xcd - 1) / cus_per_xcd;
            const double eff = (double)slots_x / (double)(rounds * cus_per_xcd);
            if (eff > best + 1e-9) {
                best = eff;
                best_sub = s;
            }
            if (eff >= (s == 1 ? 0.93 : 0.97)) break;    // one range per XCD keeps every block of a range resident at once: the convoy
                                                        // holds them together and the range is fetched from HBM once (30 blocks on 32
                                                        // CUs: 33 GB per launch instead of 354 GB in sixteen ranges, for the same time)
        }
        sub = best_sub;
    }
    return sub;
}

// PACKED (measurement builds): K1bK (maxsim_batch_packed.hip), the eight-wave form whose chunks hold several short documents
template <bool F16, int NW, int RING, int AUX, int MAXU, bool PACKED>
auto batch_kernel_ptr() {
#if defined(MSIM_AB) || defined(MSIM_TRACE)
    if constexpr (PACKED) return msim::maxsim_batch_packed_kernel<F16, AUX, MAXU>;
    else
#endif
    return msim::maxsim_batch_kernel<F16, NW, RING, AUX, MAXU>;
}

template <bool F16, int NW, int RING = 3, int AUX = 0, int MAXU = 8, bool PACKED = false>
int launch_batch(const FwdCall &c, const FlatPlan &plan) {
    static_assert(!PACKED || (NW == 8 && RING == 3), "K1bK is the eight-wave form");
    auto kern = batch_kernel_ptr<F16, NW, RING, AUX, MAXU, PACKED>();
    // ring + the per-token max table(s) + the queries' token ranges
    constexpr int lds = RING * (NW / 2) * msim::kSlabBytes +
                        (PACKED ? 2 * (NW / 2) * NW * MAXU * msim::kUnitTok * 4 : (NW > 2 ? 2 : 1) * NW * MAXU * msim::kUnitTok * 16) +
                        NW * 8 * 8;
    constexpr int wg_per_cu = MAXU == 5 ? 12 / NW : 8 / NW;  // the five-unit form: 168 registers, three waves per SIMD (three 4-wave workgroups per CU)
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    // blockIdx -> (XCD = b % 8, slot = b / 8): the CUs of one XCD share a document range through its L2
    const int cus_per_xcd = (c.di->cus / 8 > 0 ? c.di->cus / 8 : 1) * wg_per_cu;   // resident workgroups per XCD
    static const int over_env = ab_env("MSIM_BATCH_OVER", NW == 4 ? 8 : 1);
    static const bool convoy_off = ab_env("MSIM_BATCH_CONVOY", 1) == 0;
    const int total_blocks = plan.n_blocks();
    for (int b0 = 0; b0 < total_blocks; b0 += msim::kMaxQBlocks) {       // the block table travels in the kernel arguments
        msim::BatchArgs a{};
        a.ld = c.ld;
        a.fq = flat_q(c);
        a.n_d = c.n_d;
        a.flags = c.flags;
        a.n_qblocks = total_blocks - b0 < msim::kMaxQBlocks ? total_blocks - b0 : msim::kMaxQBlocks;
        for (int b = 0; b <= a.n_qblocks; ++b) a.blk_q0[b] = plan.blk_q0[b0 + b];
        // Ranges per XCD.  An XCD's workgroups are handed out in blockIdx order, range-major: (range 0, all query blocks), (range 1, ...),
        // so the slots of one XCD are a queue its CUs drain.  One block: one range per resident workgroup.  Several blocks: the number
        // of slots (blocks x ranges) should fill whole rounds of the XCD's resident workgroups -- 40 blocks on 32 CUs in ONE range each
        // are two rounds, the second a quarter full (round 4, 1000 queries x 40 tokens: 1125 ms; four ranges = 160 slots = five full
        // rounds); 20 blocks in one range leave 12 of 32 CUs idle.  Smallest number of ranges whose last round is >= 97 % full, else
        // the fullest; never ranges of fewer than two documents.
        // a range costs its workgroup a prologue (the block's 64 units: 256 KiB out of L2) whatever its size, so it should hold ~2000
        // rows.  The host does not see the row offsets: without the caller's hint (MSIM_FLAG_AVG_ROWS) that is taken as 64 documents.
        // (Round 5: with that floor alone a 1000-page corpus of 1030-row pages -- the drop-in call of BASELINE config 2 -- got ONE range
        // per XCD: 4 query blocks x 8 ranges = 32 workgroups on 256 CUs.)
        int sub = ranges_per_xcd(a.n_qblocks, cus_per_xcd, c.n_d, c.avg_rows);
        // Two workgroups share a CU in the 4-wave form, and the matrix pipe serves the OLDER wave first: of two workgroups that start
        // together one finishes after ~2/3 of the launch and the other runs its last third alone, one wave per SIMD, which cannot fill
        // the pipe (tools/trace_batch.py: workgroup 0 busy for 68 % of the launch; SQ_WAVE_CYCLES: 83 % occupancy).  With 8 x more, smaller
        // ranges than resident workgroups a finished workgroup is replaced at once and the lone phase shrinks to the last range: +3-5 %
        // at 9..16 queries (profiles/r02_logs/ab_batch_over.log; the pair form does not gain and keeps one range per resident
        // workgroup).  Only when one query block streams the corpus (no L2 sharing between blocks to preserve), and never down
        // to ranges of fewer than ~16 documents.
        if (NW < 8 && a.n_qblocks == 1 && over_env > 1) {
            int over = over_env;
            while (over > 1 && (long long)8 * sub * over * 16 > c.n_d) over >>= 1;
            sub *= over;
        }
        a.n_ranges = 8 * sub;
        const int slots = sub > 1 ? a.n_qblocks * sub : a.n_qblocks;
        // convoy (maxsim_batch.hip): only when several query blocks share a range AND all of them are resident at once
        a.convoy = nullptr;
        if (c.workspace && !convoy_off && a.n_qblocks > 1 && (long long)a.n_qblocks * sub <= cus_per_xcd && a.n_qblocks <= 64 &&
            (size_t)a.n_ranges * a.n_qblocks * sizeof(int) <= kFwdWorkspaceBytes) {
            a.convoy = static_cast<int *>(c.workspace);
            if (hipMemsetAsync(a.convoy, 0, (size_t)a.n_ranges * a.n_qblocks * sizeof(int), c.st) != hipSuccess)
                return fail(MSIM_ELAUNCH, "hipMemsetAsync(convoy counters) failed");
        }
        a.trace = nullptr;
#ifdef MSIM_TRACE
        if (const char *tp = getenv("MSIM_BATCH_TRACE_PTR")) a.trace = reinterpret_cast<unsigned long long *>(strtoull(tp, nullptr, 0));
#endif
        hipLaunchKernelGGL(kern, dim3(8 * slots), dim3(NW * 64), lds, c.st, c.Q, c.D, c.d_off, c.clamp0, c.scores, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_batch%s_kernel<%d,%d> launch: %s", PACKED ? "_packed" : "", NW, MAXU, hipGetErrorString(e));
    }
    return MSIM_OK;
}

template <bool F16>
int fwd_dispatch(const FwdCall &c) {
    thread_local FlatPlan plan;
    if (int rc = flat_plan(host_q(c), c.n_q, plan)) return rc;
    if (plan.stream) {
        if constexpr (!F16) {
            if (c.p13 != nullptr)
                return dispatch_units(plan.nu, [&](auto nu) { return launch_stream13<decltype(nu)::value>(c); });
        }
        return dispatch_units(plan.nu, [&](auto nu) { return launch_stream<decltype(nu)::value, F16>(c); });
    }
    // one query block = every corpus byte is read once by one workgroup: stream it past L2 / MALL (nt), like K1s does.
    // MSIM_BATCH_NT=0 switches that off for A/B measurements (tuning knob, not part of the ABI).
    static const bool nt_off = ab_env("MSIM_BATCH_NT", 1) == 0;
    const bool single = plan.n_blocks() == 1 && !nt_off;
    if (plan.nw == 4 && plan.maxu == 5) {
#ifdef MSIM_AB
        static const int ring5 = ab_env("MSIM_BATCH_RING5", 2);
        if (ring5 == 3) return launch_batch<F16, 4, 3, 2, 5>(c, plan);
#endif
        return launch_batch<F16, 4, 2, 2, 5>(c, plan);
    }
#ifdef MSIM_AB
    if (plan.nw == 2 && plan.maxu == 10) return launch_batch<F16, 2, 4, 2, 10>(c, plan);
    if (plan.nw == 2 && plan.maxu == 5) {
        static const int ring5p = ab_env("MSIM_BATCH_RING5", 2);
        return ring5p == 3 ? launch_batch<F16, 2, 3, 2, 5>(c, plan) : launch_batch<F16, 2, 2, 2, 5>(c, plan);
    }
#endif
    if (plan.nw == 2) return launch_batch<F16, 2, 4, 2, 8>(c, plan);
#ifdef MSIM_AB
    if (plan.nw == 4 && plan.maxu == 8 && !single) return launch_batch<F16, 4, 3, 0, 8>(c, plan);
#endif
    if (plan.nw == 4) return plan.maxu == 10 ? launch_batch<F16, 4, 3, 2, 10>(c, plan) : launch_batch<F16, 4, 3, 2, 8>(c, plan);
#if defined(MSIM_AB) || defined(MSIM_TRACE)
    // measurement builds only (round 6, short documents): MSIM_BATCH_PACKED=1 -- chunks that hold several documents (K1bK); the same
    // bits, 4-9 % slower than K1b at 64 / 343 rows (profiles/r06_logs/ab_short_docs_packed.log)
    static const int packed_env = ab_env("MSIM_BATCH_PACKED", 0);
    if (packed_env != 0) {
        if (plan.maxu == 10) return single ? launch_batch<F16, 8, 3, 2, 10, true>(c, plan) : launch_batch<F16, 8, 3, 0, 10, true>(c, plan);
        return single ? launch_batch<F16, 8, 3, 2, 8, true>(c, plan) : launch_batch<F16, 8, 3, 0, 8, true>(c, plan);
    }
#endif
    if (plan.maxu == 10) return single ? launch_batch<F16, 8, 3, 2, 10>(c, plan) : launch_batch<F16, 8, 3, 0, 10>(c, plan);
    return single ? launch_batch<F16, 8, 3, 2, 8>(c, plan) : launch_batch<F16, 8, 3, 0, 8>(c, plan);
}

// scratch of a tuned forward call: K1b's convoy counters, needed once several query blocks stream a document range
size_t flat_workspace_bytes(const HostQ &hq, int n_q) {
    thread_local FlatPlan plan;
    if (flat_plan(hq, n_q, plan) != MSIM_OK) return 0;
    return (!plan.stream && plan.n_blocks() > 1) ? kFwdWorkspaceBytes : 0;
}

// ---------------------------------------------------------------- generic kernels (K1g)
template <int DT, int T>
int launch_generic(const GenericCall &c) {
    auto kern = msim::maxsim_generic_kernel<DT, T>;
    const int lds = T * msim::kTokTile * (c.row_bytes + 16);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, 160 * 1024, configured)) return rc;
    msim::GenericArgs a;
    a.ld = c.ld;
    a.n_q = c.n_q;
    a.Lq = c.Lq;
    a.n_d = c.n_d;
    a.row_bytes = c.row_bytes;
    a.flags = c.flags;
    const int tpq = (c.Lq + msim::kTokTile - 1) / msim::kTokTile;
    const int groups = tpq <= T ? (c.n_q + (T / tpq) - 1) / (T / tpq) : c.n_q;
    if (groups > 65535) return fail(MSIM_EUNSUPPORTED, "too many query groups (%d) for one launch", groups);
    const int wg_needed = (c.n_d + msim::kGenericWaves - 1) / msim::kGenericWaves;
    int per_cu = c.di->lds_per_cu / lds;
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int wg_cap = c.di->cus * per_cu;
    hipLaunchKernelGGL(kern, dim3(wg_needed < wg_cap ? wg_needed : wg_cap, groups), dim3(msim::kGenericWaves * 64), lds, c.st,
                       c.Q, c.D, c.d_off, c.clamp0, c.scores, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_generic_kernel<%d,%d> launch: %s", DT, T, hipGetErrorString(e));
    return MSIM_OK;
}

template <int DT>
int generic_dispatch(const GenericCall &c) {
    const int tpq = (c.Lq + msim::kTokTile - 1) / msim::kTokTile;
    const long long tiles = (long long)c.n_q * tpq;
    const int tile_lds = msim::kTokTile * (c.row_bytes + 16);
    int T = 4;                                   // resident token tiles: as many as fit 96 KiB of LDS
    while (T > 1 && (T * tile_lds > 96 * 1024 || T / 2 >= tiles)) T >>= 1;
    switch (T) {
        case 4: return launch_generic<DT, 4>(c);
        case 2: return launch_generic<DT, 2>(c);
        default: return launch_generic<DT, 1>(c);
    }
}

int generic_fwd(int dtype, const GenericCall &c) {
    switch (dtype) {
        case MSIM_DTYPE_F32: return generic_dispatch<msim::kDtypeF32>(c);
        case MSIM_DTYPE_F16: return generic_dispatch<msim::kDtypeF16>(c);
        default: return generic_dispatch<msim::kDtypeBf16>(c);
    }
}


// ---------------------------------------------------------------- plain similarity matrix
template <int DT, int T>
int launch_sim(const char *A, const char *B, float *out, const msim::SimArgs &a, const DeviceInfo &di, hipStream_t st) {
    auto kern = msim::sim_matrix_kernel<DT, T>;
    const int lds = T * msim::kTokTile * (a.row_bytes + 16);
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, 160 * 1024, configured)) return rc;
    const int groups = (a.n_a + T * msim::kTokTile - 1) / (T * msim::kTokTile);
    if (groups > 65535) return fail(MSIM_EUNSUPPORTED, "too many row groups (%d) for one launch", groups);
    const int slabs = (a.n_b + msim::kSlabRows - 1) / msim::kSlabRows;
    const int wg_needed = (slabs + msim::kGenericWaves - 1) / msim::kGenericWaves;
    int per_cu = di.lds_per_cu / lds;
    per_cu = per_cu < 1 ? 1 : (per_cu > 4 ? 4 : per_cu);
    const int wg_cap = di.cus * per_cu;
    hipLaunchKernelGGL(kern, dim3(wg_needed < wg_cap ? wg_needed : wg_cap, groups), dim3(msim::kGenericWaves * 64), lds, st, A, B,
                       out, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "sim_matrix_kernel<%d,%d> launch: %s", DT, T, hipGetErrorString(e));
    return MSIM_OK;
}

template <int DT>
int sim_dispatch(const char *A, const char *B, float *out, const msim::SimArgs &a, const DeviceInfo &di, hipStream_t st) {
    const int tile_lds = msim::kTokTile * (a.row_bytes + 16);
    int T = 4;
    while (T > 1 && (T * tile_lds > 80 * 1024 || (T / 2) * msim::kTokTile >= a.n_a)) T >>= 1;
    switch (T) {
        case 4: return launch_sim<DT, 4>(A, B, out, a, di, st);
        case 2: return launch_sim<DT, 2>(A, B, out, a, di, st);
        default: return launch_sim<DT, 1>(A, B, out, a, di, st);
    }
}

// ---------------------------------------------------------------- panel kernels (K1sP / K1bP): 16-bit, dim 320
constexpr int kPanels320 = 3, kLast320 = 4;     // 320 = (2 * 8 + 4) * 16

bool is_panels(int dtype, int dim, long long tiles, int tpq) {
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != 320 || tpq > 4) return false;
    return tiles <= 4 || tpq <= 2;               // K1sP holds <= 4 token tiles, K1bP whole queries of <= 2 tiles per wave
}

template <int QT, int TPQ, bool F16>
int launch_stream_panels(const FwdCall &c) {
    auto kern = msim::maxsim_stream_panels_kernel<QT, TPQ, kPanels320, kLast320, F16, 2>;
    constexpr int lds = 4 * msim::kPanelRing * msim::kSlabBytes;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    msim::PanelStreamArgs a;
    a.ld = c.ld;
    a.n_q = c.n_q;
    a.Lq = c.Lq;
    a.n_d = c.n_d;
    a.flags = c.flags;
    hipLaunchKernelGGL(kern, stream_grid(c, lds), dim3(256), lds, c.st, c.Q, c.D, c.d_off, c.clamp0, c.scores, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_stream_panels_kernel<%d,%d> launch: %s", QT, TPQ, hipGetErrorString(e));
    return MSIM_OK;
}

template <int NT, int TPQ, bool F16>
int launch_batch_panels(const FwdCall &c) {
    auto kern = msim::maxsim_batch_panels_kernel<NT, TPQ, kPanels320, kLast320, F16>;
    constexpr int lds = msim::kPanelStages * kPanels320 * msim::kSlabBytes;
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    msim::PanelBatchArgs a{};
    a.ld = c.ld;
    a.n_q = c.n_q;
    a.Lq = c.Lq;
    a.n_d = c.n_d;
    a.flags = c.flags;
    const int q_per_block = msim::kBatchWaves * NT / TPQ;
    a.n_qblocks = (c.n_q + q_per_block - 1) / q_per_block;
    const int cus_per_xcd = c.di->cus / 8 > 0 ? c.di->cus / 8 : 1;
    const int sub = a.n_qblocks >= cus_per_xcd ? 1 : cus_per_xcd / a.n_qblocks;
    a.n_ranges = 8 * sub;
    const int slots = sub > 1 ? a.n_qblocks * sub : a.n_qblocks;
    hipLaunchKernelGGL(kern, dim3(8 * slots), dim3(512), lds, c.st, c.Q, c.D, c.d_off, c.clamp0, c.scores, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_batch_panels_kernel<%d,%d> launch: %s", NT, TPQ, hipGetErrorString(e));
    return MSIM_OK;
}

template <bool F16>
int panels_dispatch(const FwdCall &c) {
    const int tpq = (c.Lq + msim::kTokTile - 1) / msim::kTokTile;
    if ((long long)c.n_q * tpq <= 4) {
        switch (c.n_q * 10 + tpq) {
            case 11: return launch_stream_panels<1, 1, F16>(c);
            case 21: return launch_stream_panels<2, 1, F16>(c);
            case 31: return launch_stream_panels<3, 1, F16>(c);
            case 41: return launch_stream_panels<4, 1, F16>(c);
            case 12: return launch_stream_panels<2, 2, F16>(c);
            case 22: return launch_stream_panels<4, 2, F16>(c);
            case 13: return launch_stream_panels<3, 3, F16>(c);
            default: return launch_stream_panels<4, 4, F16>(c);
        }
    }
    if (tpq == 2) return launch_batch_panels<2, 2, F16>(c);
    return c.n_q <= 8 ? launch_batch_panels<1, 1, F16>(c) : launch_batch_panels<2, 1, F16>(c);
}


// ---- K1bPF: the flat token layout at width 320 (maxsim_panels.hip).  8 waves x <= 4 units (round 6: or ONE block of 2 / 4 waves for small batches), query blocks of whole queries
// (<= 512 tokens, <= 64 queries), filled greedily in query order and re-cut evenly like K1b's.
constexpr int kPanelsFlatMaxU = 4;
constexpr int kPanelsFlatMaxTokens = msim::kBatchWaves * kPanelsFlatMaxU * msim::kUnitTok;      // 512

int panels_flat_plan(const HostQ &hq, int n_q, FlatPlan &p) {
    if ((long long)hq.at(n_q) - hq.at(0) < 0) return fail(MSIM_EINVAL, "query token offsets are not non-decreasing");
    p = FlatPlan{};
    // the ladder (round 6): a batch that fits ONE block of two waves (<= 8 units, <= 16 queries) or four waves (<= 16 units, <= 32
    // queries) takes that shape -- up to four units per wave behind a narrower barrier, two workgroups per CU; everything else the
    // 8-wave shape (one or several blocks)
    const long long tokens = (long long)hq.at(n_q) - hq.at(0);
    const long long units = (tokens + msim::kUnitTok - 1) / msim::kUnitTok;
    p.nw = (units <= 2 * kPanelsFlatMaxU && n_q <= 16) ? 2 : (units <= 4 * kPanelsFlatMaxU && n_q <= 32) ? 4 : msim::kBatchWaves;
    p.maxu = kPanelsFlatMaxU;
    if (!fill_blocks(hq, n_q, p.nw, p.maxu, p.blk_q0) || (p.nw != msim::kBatchWaves && p.n_blocks() != 1)) {
        p.nw = msim::kBatchWaves;                     // (unit padding at query borders cannot overflow: units counts whole tokens)
        p.blk_q0.clear();
    }
    if (p.blk_q0.empty() && !fill_blocks(hq, n_q, p.nw, p.maxu, p.blk_q0))
        return fail(MSIM_EUNSUPPORTED, "a query of more than %d tokens does not fit one query block of the width-320 kernels: pad the "
                    "queries to one length and call msim_fwd", kPanelsFlatMaxTokens);
    balance_blocks(hq, n_q, p.nw, p.maxu, p.blk_q0);
    return MSIM_OK;
}

template <bool F16, int NW, int STAGES>
int launch_batch_panels_flat_nw(const FwdCall &c, const FlatPlan &plan) {
    auto kern = msim::maxsim_batch_panels_flat_kernel<F16, kPanels320, kLast320, kPanelsFlatMaxU, NW, STAGES>;
    constexpr int lds = STAGES * kPanels320 * msim::kSlabBytes + NW * kPanelsFlatMaxU * msim::kUnitTok * 16 +
                        NW * 8 * 8;                      // stage ring + the per-token max table + the queries' token ranges
    static std::atomic<int> configured[kMaxDevices];
    if (int rc = allow_lds(kern, lds, configured)) return rc;
    const int cus_per_xcd = (c.di->cus / 8 > 0 ? c.di->cus / 8 : 1) * (NW == msim::kBatchWaves ? 1 : 2);   // workgroups resident per XCD
    const int total_blocks = plan.n_blocks();
    for (int b0 = 0; b0 < total_blocks; b0 += msim::kMaxQBlocks) {
        msim::BatchArgs a{};
        a.ld = c.ld;
        a.fq = flat_q(c);
        a.n_d = c.n_d;
        a.flags = c.flags;
        a.n_qblocks = total_blocks - b0 < msim::kMaxQBlocks ? total_blocks - b0 : msim::kMaxQBlocks;
        for (int b = 0; b <= a.n_qblocks; ++b) a.blk_q0[b] = plan.blk_q0[b0 + b];
        const int sub = ranges_per_xcd(a.n_qblocks, cus_per_xcd, c.n_d, c.avg_rows);
        a.n_ranges = 8 * sub;
        const int slots = sub > 1 ? a.n_qblocks * sub : a.n_qblocks;
        a.convoy = nullptr;
        a.trace = nullptr;
        hipLaunchKernelGGL(kern, dim3(8 * slots), dim3(NW * 64), lds, c.st, c.Q, c.D, c.d_off, c.clamp0, c.scores, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_batch_panels_flat_kernel<%d> launch: %s", NW, hipGetErrorString(e));
    }
    return MSIM_OK;
}

template <bool F16>
int launch_batch_panels_flat(const FwdCall &c) {
    thread_local FlatPlan plan;
    if (int rc = panels_flat_plan(host_q(c), c.n_q, plan)) return rc;
    if (plan.nw == 2) return launch_batch_panels_flat_nw<F16, 2, 3>(c, plan);
    if (plan.nw == 4) return launch_batch_panels_flat_nw<F16, 4, 3>(c, plan);
    return launch_batch_panels_flat_nw<F16, msim::kBatchWaves, msim::kPanelStages>(c, plan);
}

// a uniform box [n_q, Lq, 320] on the flat kernel?  K1sP keeps the calls of <= 4 token tiles (HBM-bound, no barriers); K1bP keeps whole
// queries of 32 or 64 tokens (no padding to win back); everything else up to 512 tokens is scored as 16-token units of the token matrix,
// which cross query borders (1000 x Lq 40: 2500 units of 16 instead of 2000 tiles of 32) -- and three and more tiles per query, which
// K1bP does not take, are just more units.  MSIM_PANELS_FLAT=0|1 forces the choice (A/B knob of the measurement builds, not ABI).
bool box_on_panels_flat(int dtype, int dim, int n_q, int Lq) {
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != 320 || Lq > kPanelsFlatMaxTokens) return false;
    const int tpq = (Lq + msim::kTokTile - 1) / msim::kTokTile;
    if ((long long)n_q * tpq <= 4) return false;
    static const int forced = ab_env("MSIM_PANELS_FLAT", -1);
    if (forced == 0) return tpq > 2;
    if (forced == 1) return true;
    return tpq > 2 || (Lq % msim::kTokTile) != 0;
}

int fwd_ragged_impl(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                    const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, float *scores, int64_t ld_scores,
                    uint32_t flags, void *workspace, void *stream, const Pack13View *p13);
int fwd_impl(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
             int n_d, int dim, float *scores, int64_t ld_scores, uint32_t flags, void *workspace, void *stream, const Pack13View *p13);

// the image arguments of the *_pack13 entries
int check_pack13(const char *who, const void *image, const int32_t *slab_off, const uint8_t *flagged, const int32_t *list, int n_list,
                 Pack13View *v) {
    if (!image || !slab_off || !flagged || n_list < 0 || (n_list > 0 && !list)) return fail(MSIM_EINVAL, "%s: bad image arguments", who);
    if (reinterpret_cast<uintptr_t>(image) & 15) return fail(MSIM_EINVAL, "%s: the image must be 16-byte aligned", who);
    *v = Pack13View{static_cast<const uint8_t *>(image), slab_off, flagged, list, n_list};
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_fwd_pack13(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d,
                    int dim, const void *image, const int32_t *slab_off, const uint8_t *flagged, const int32_t *list, int n_list,
                    float *scores, int64_t ld_scores, uint32_t flags, void *workspace, void *stream) {
    Pack13View v;
    if (int rc = check_pack13("msim_fwd_pack13", image, slab_off, flagged, list, n_list, &v)) return rc;
    return fwd_impl(dtype, Q, n_q, Lq, D, d_off, d_clamp0, n_d, dim, scores, ld_scores, flags, workspace, stream, &v);
}

int msim_fwd_ragged_pack13(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                           const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, const void *image, const int32_t *slab_off,
                           const uint8_t *flagged, const int32_t *list, int n_list, float *scores, int64_t ld_scores, uint32_t flags,
                           void *workspace, void *stream) {
    Pack13View v;
    if (int rc = check_pack13("msim_fwd_ragged_pack13", image, slab_off, flagged, list, n_list, &v)) return rc;
    return fwd_ragged_impl(dtype, Qt, q_off, q_off_host, n_q, D, d_off, d_clamp0, n_d, dim, scores, ld_scores, flags, workspace, stream, &v);
}

int msim_fwd_ragged(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                    const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, float *scores, int64_t ld_scores,
                    uint32_t flags, void *workspace, void *stream) {
    return fwd_ragged_impl(dtype, Qt, q_off, q_off_host, n_q, D, d_off, d_clamp0, n_d, dim, scores, ld_scores, flags, workspace, stream, nullptr);
}

int msim_fwd(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
             int n_d, int dim, float *scores, int64_t ld_scores, uint32_t flags, void *workspace, void *stream) {
    return fwd_impl(dtype, Q, n_q, Lq, D, d_off, d_clamp0, n_d, dim, scores, ld_scores, flags, workspace, stream, nullptr);
}

size_t msim_fwd_workspace_bytes(int dtype, int n_q, int Lq, int n_d, int dim) {
    // the only scratch msim_fwd uses: the progress counters of K1b's convoy, needed once more than one query block streams a
    // document range (bf16 / fp16, width 128).  Passing NULL instead only switches the convoy off; a non-null workspace must hold
    // at least the bytes reported here (4096 whenever it is non-zero).
    if (n_q <= 0 || n_d <= 0 || Lq <= 0) return 0;
    if (is_long_tuned(dtype, dim, Lq))                                              // pieces on K1b: counters + the partial sums
        return kFwdWorkspaceBytes + (size_t)n_q * long_segments(Lq) * n_d * sizeof(float);
    if (!is_tuned(dtype, dim, Lq)) return 0;
    return flat_workspace_bytes(HostQ{nullptr, Lq, 0, 1}, n_q);                     // exactly launch_batch's condition
}

int msim_fwd_plan(const int32_t *q_off_host, int n_q, int Lq, int32_t *out5) {
    if (!out5 || n_q <= 0 || (!q_off_host && Lq <= 0)) return fail(MSIM_EINVAL, "bad arguments");
    thread_local FlatPlan plan;
    const HostQ hq = q_off_host ? HostQ{q_off_host, 0, 0, 1}
                                : (Lq > kLongSegRows ? HostQ{nullptr, Lq, kLongSegRows, long_segments(Lq)} : HostQ{nullptr, Lq, 0, 1});
    if (!q_off_host && Lq > kLongSegRows && (long long)n_q * long_segments(Lq) > 0x7fffffff / 8)
        return fail(MSIM_EUNSUPPORTED, "too many 128-token pieces (%d queries x %d)", n_q, long_segments(Lq));
    const int n = (!q_off_host && Lq > kLongSegRows) ? n_q * long_segments(Lq) : n_q;
    if (int rc = flat_plan(hq, n, plan)) return rc;
    out5[0] = plan.stream ? 0 : 1;
    out5[1] = plan.stream ? plan.nu : plan.nw;
    out5[2] = plan.stream ? 0 : plan.maxu;
    out5[3] = plan.stream ? 1 : plan.n_blocks();
    out5[4] = plan.stream ? plan.nu : heaviest_wave_units(hq, plan.blk_q0, plan.nw);
    return MSIM_OK;
}

size_t msim_fwd_ragged_workspace_bytes(int dtype, const int32_t *q_off_host, int n_q, int n_d, int dim) {
    if (n_q <= 0 || n_d <= 0 || !q_off_host) return 0;
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != msim::kDim) return 0;
    return flat_workspace_bytes(HostQ{q_off_host, 0, 0, 1}, n_q);
}

}  // extern "C"

namespace {

int fwd_ragged_impl(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                    const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, float *scores, int64_t ld_scores,
                    uint32_t flags, void *workspace, void *stream, const Pack13View *p13) {
    if (n_q < 0 || n_d < 0) return fail(MSIM_EINVAL, "negative size (n_q=%d n_d=%d)", n_q, n_d);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!scores || !Qt || !D || !d_off || !q_off || !q_off_host) return fail(MSIM_EINVAL, "null pointer argument");
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || !(dim == msim::kDim || dim == 320))
        return fail(MSIM_EUNSUPPORTED, "msim_fwd_ragged takes bfloat16 / float16 embeddings of width %d or 320 (dtype code %d, dim %d): "
                    "pad the queries to one length and call msim_fwd", msim::kDim, dtype, dim);
    if ((reinterpret_cast<uintptr_t>(Qt) | reinterpret_cast<uintptr_t>(D)) & 15) return fail(MSIM_EINVAL, "Qt and D must be 16-byte aligned");
    if (workspace && (reinterpret_cast<uintptr_t>(workspace) & 15)) return fail(MSIM_EINVAL, "workspace must be 16-byte aligned");
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "ld_scores=%lld < n_d=%d", (long long)ld_scores, n_d);
    const int avg_rows = (int)((flags >> 8) & 0xffffu);          // MSIM_FLAG_AVG_ROWS(n): a launch-shape hint, never a result
    flags &= ~(0xffffu << 8);
    if (flags & ~(MSIM_FLAG_REF_ROUNDING)) return fail(MSIM_EINVAL, "unknown flags 0x%x", flags);
    if (q_off_host[0] != 0) return fail(MSIM_EINVAL, "q_off[0] must be 0");
    for (int i = 0; i < n_q; ++i)
        if (q_off_host[i + 1] < q_off_host[i]) return fail(MSIM_EINVAL, "q_off must be non-decreasing (query %d)", i);
    FwdCall c;
    if (int rc = device_info(&c.di)) return rc;
    c.Q = static_cast<const uint16_t *>(Qt);
    c.D = static_cast<const uint16_t *>(D);
    c.d_off = d_off;
    c.clamp0 = d_clamp0;
    c.scores = scores;
    c.ld = ld_scores;
    c.n_q = n_q;
    c.Lq = 0;
    c.n_d = n_d;
    c.flags = flags;
    c.st = static_cast<hipStream_t>(stream);
    c.workspace = workspace;
    c.q_off = q_off;
    c.q_off_host = q_off_host;
    c.avg_rows = avg_rows;
    if (dim == 320) {
        // width 320 (ColQwen3): queries of ONE length and at most four 32-token tiles in all are a box K1sP streams without a barrier;
        // everything else goes to the flat panel kernel
        const int L0 = q_off_host[1];
        bool uniform = true;
        for (int i = 1; i < n_q && uniform; ++i) uniform = q_off_host[i + 1] - q_off_host[i] == L0;
        const int tpq = (L0 + msim::kTokTile - 1) / msim::kTokTile;
        if (uniform && L0 > 0 && is_panels(dtype, dim, (long long)n_q * tpq, tpq) && (long long)n_q * tpq <= 4) {
            c.Lq = L0;
            c.q_off = nullptr;
            c.q_off_host = nullptr;
            return dtype == MSIM_DTYPE_F16 ? panels_dispatch<true>(c) : panels_dispatch<false>(c);
        }
        return dtype == MSIM_DTYPE_F16 ? launch_batch_panels_flat<true>(c) : launch_batch_panels_flat<false>(c);
    }
    c.p13 = p13;                      // width 128; fwd_dispatch uses it for bf16 K1s plans only
    return dtype == MSIM_DTYPE_F16 ? fwd_dispatch<true>(c) : fwd_dispatch<false>(c);
}

int fwd_impl(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
             int n_d, int dim, float *scores, int64_t ld_scores, uint32_t flags, void *workspace, void *stream, const Pack13View *p13) {
    if (n_q < 0 || n_d < 0 || Lq <= 0) return fail(MSIM_EINVAL, "negative size (n_q=%d n_d=%d Lq=%d)", n_q, n_d, Lq);
    if (n_q == 0 || n_d == 0) return MSIM_OK;
    if (!scores) return fail(MSIM_EINVAL, "null pointer argument");
    if (int rc = check_common(Q, D, d_off, dtype, dim, Lq)) return rc;
    if (ld_scores < n_d) return fail(MSIM_EINVAL, "ld_scores=%lld < n_d=%d", (long long)ld_scores, n_d);
    const int avg_rows = (int)((flags >> 8) & 0xffffu);          // MSIM_FLAG_AVG_ROWS(n): a launch-shape hint, never a result
    flags &= ~(0xffffu << 8);
    if (flags & ~(MSIM_FLAG_REF_ROUNDING)) return fail(MSIM_EINVAL, "unknown flags 0x%x", flags);
    {
        const int tpq = (Lq + msim::kTokTile - 1) / msim::kTokTile;
        const bool on_flat = box_on_panels_flat(dtype, dim, n_q, Lq);
        if (on_flat || is_panels(dtype, dim, (long long)n_q * tpq, tpq)) {
            FwdCall c;
            if (int rc = device_info(&c.di)) return rc;
            c.Q = static_cast<const uint16_t *>(Q);
            c.D = static_cast<const uint16_t *>(D);
            c.d_off = d_off;
            c.clamp0 = d_clamp0;
            c.scores = scores;
            c.ld = ld_scores;
            c.n_q = n_q;
            c.Lq = Lq;
            c.n_d = n_d;
            c.flags = flags;
            c.avg_rows = avg_rows;
            c.st = static_cast<hipStream_t>(stream);
            if (on_flat)      // the box IS a flat token matrix with uniform offsets (FlatQ: q_off null, Lq)
                return dtype == MSIM_DTYPE_F16 ? launch_batch_panels_flat<true>(c) : launch_batch_panels_flat<false>(c);
            return dtype == MSIM_DTYPE_F16 ? panels_dispatch<true>(c) : panels_dispatch<false>(c);
        }
    }
    // long queries in the tuned dtype / width (pages as queries, image-to-image retrieval, the trainer's symmetric direction): 128-token
    // PIECES on K1b -- MaxSim is a sum over query tokens, and in the flat token layout a piece is nothing but another pair of token
    // offsets -- partial token sums into the scratch, added in piece order: 3-4 x the generic kernels' rate on a large corpus.
    // The piece rows are reduced 65 535 queries at a time (grid.y of segment_sum_kernel).
    if (is_long_tuned(dtype, dim, Lq) && workspace != nullptr && (long long)n_q * long_segments(Lq) <= 0x7fffffff / 8) {
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(MSIM_EINVAL, "workspace must be 16-byte aligned");
        const int n_seg = long_segments(Lq);
        float *partial = reinterpret_cast<float *>(static_cast<char *>(workspace) + kFwdWorkspaceBytes);
        FwdCall c;
        if (int rc = device_info(&c.di)) return rc;
        c.Q = static_cast<const uint16_t *>(Q);
        c.D = static_cast<const uint16_t *>(D);
        c.d_off = d_off;
        c.clamp0 = d_clamp0;
        c.scores = partial;
        c.ld = n_d;
        c.n_q = n_q * n_seg;
        c.Lq = Lq;
        c.n_d = n_d;
        c.flags = flags | msim::kFlagPartial;
        c.avg_rows = avg_rows;
        c.st = static_cast<hipStream_t>(stream);
        c.workspace = workspace;
        c.seg = kLongSegRows;
        c.n_seg = n_seg;
        const bool f16 = dtype == MSIM_DTYPE_F16;
        if (int rc = f16 ? fwd_dispatch<true>(c) : fwd_dispatch<false>(c)) return rc;
        const bool round_total = (flags & MSIM_FLAG_REF_ROUNDING) != 0;
        for (int q0 = 0; q0 < n_q; q0 += 65535) {
            const int nq = n_q - q0 < 65535 ? n_q - q0 : 65535;
            const dim3 grid((n_d + 255) / 256, nq);
            const float *part = partial + (size_t)q0 * n_seg * n_d;
            float *out = scores + (size_t)q0 * ld_scores;
            if (f16)
                hipLaunchKernelGGL(msim::segment_sum_kernel<true>, grid, dim3(256), 0, c.st, part, (long long)n_d, n_seg, n_d, out,
                                   (long long)ld_scores, round_total);
            else
                hipLaunchKernelGGL(msim::segment_sum_kernel<false>, grid, dim3(256), 0, c.st, part, (long long)n_d, n_seg, n_d, out,
                                   (long long)ld_scores, round_total);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "segment_sum_kernel launch: %s", hipGetErrorString(e));
        return MSIM_OK;
    }
    if (!is_tuned(dtype, dim, Lq)) {
        GenericCall c;
        if (int rc = device_info(&c.di)) return rc;
        c.Q = static_cast<const char *>(Q);
        c.D = static_cast<const char *>(D);
        c.d_off = d_off;
        c.clamp0 = d_clamp0;
        c.scores = scores;
        c.ld = ld_scores;
        c.n_q = n_q;
        c.Lq = Lq;
        c.n_d = n_d;
        c.row_bytes = dim * elem_bytes(dtype);
        c.flags = flags;
        c.st = static_cast<hipStream_t>(stream);
        return generic_fwd(dtype, c);
    }
    FwdCall c;
    if (int rc = device_info(&c.di)) return rc;
    c.Q = static_cast<const uint16_t *>(Q);
    c.D = static_cast<const uint16_t *>(D);
    c.d_off = d_off;
    c.clamp0 = d_clamp0;
    c.scores = scores;
    c.ld = ld_scores;
    c.n_q = n_q;
    c.Lq = Lq;
    c.n_d = n_d;
    c.flags = flags;
    c.avg_rows = avg_rows;
    c.st = static_cast<hipStream_t>(stream);
    c.workspace = workspace;
    c.p13 = p13;
    return dtype == MSIM_DTYPE_F16 ? fwd_dispatch<true>(c) : fwd_dispatch<false>(c);
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- plain similarity matrix entry point
int msim_sim_matrix(int dtype, const void *A, int n_a, const void *B, int n_b, int dim, float *out, int64_t ld_out,
                    uint32_t flags, void *stream) {
    if (n_a < 0 || n_b < 0) return fail(MSIM_EINVAL, "negative size (n_a=%d n_b=%d)", n_a, n_b);
    if (n_a == 0 || n_b == 0) return MSIM_OK;
    if (!out) return fail(MSIM_EINVAL, "null pointer argument");
    static const int32_t dummy_off[2] = {0, 0};
    if (int rc = check_smooth(A, B, dummy_off, dtype, dim, 1, 1.0f)) return rc;     // same row-layout contract as the generic kernels
    if (ld_out < n_b) return fail(MSIM_EINVAL, "ld_out=%lld < n_b=%d", (long long)ld_out, n_b);
    if (flags & ~(MSIM_FLAG_REF_ROUNDING)) return fail(MSIM_EINVAL, "unknown flags 0x%x", flags);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    msim::SimArgs a{ld_out, n_a, n_b, dim * elem_bytes(dtype), flags};
    const char *ac = static_cast<const char *>(A), *bc = static_cast<const char *>(B);
    hipStream_t st = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case MSIM_DTYPE_F32: return sim_dispatch<msim::kDtypeF32>(ac, bc, out, a, *di, st);
        case MSIM_DTYPE_F16: return sim_dispatch<msim::kDtypeF16>(ac, bc, out, a, *di, st);
        default: return sim_dispatch<msim::kDtypeBf16>(ac, bc, out, a, *di, st);
    }
}

int msim_query_compact(const void *box, int n_q, int Lq, int row_bytes, const int32_t *q_off, int32_t *counts, void *out,
                       void *stream) {
    if (n_q < 0 || Lq < 0 || row_bytes <= 0 || (row_bytes & 15)) return fail(MSIM_EINVAL, "bad size (row bytes must be a multiple of 16)");
    if (n_q == 0 || Lq == 0) return MSIM_OK;
    if (!box || (!counts && !(q_off && out))) return fail(MSIM_EINVAL, "null pointer argument");
    if (Lq > msim::kCompactMaxRows) return fail(MSIM_EUNSUPPORTED, "query boxes of more than %d rows are not compacted", msim::kCompactMaxRows);
    if (reinterpret_cast<uintptr_t>(box) & 15 || reinterpret_cast<uintptr_t>(out) & 15) return fail(MSIM_EINVAL, "buffers must be 16-byte aligned");
    hipLaunchKernelGGL(msim::query_compact_kernel, dim3(n_q), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const char *>(box), Lq, row_bytes, q_off, counts, static_cast<char *>(out));
    return launch_failed("query_compact_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- candidate reranking (K1c, maxsim_candidates.hip)
// In this unit and not with the other search entry points (abi_search.hip): K1c is built from K1s's slab helpers, and next to K1s and
// K1b the compiler emits for it the machine code it emitted when the library was one translation unit; in a unit without them two
// instantiations came out with another register allocation and schedule (104 bytes shorter, same descriptor), unmeasured.
namespace {

struct CandLayout {        // msim_fwd_candidates' workspace, every piece 16-byte aligned
    size_t status, cnt, bsum, estart, istart, rank, entries, items, total;
};

CandLayout cand_layout(int n_q, int m, int n_d) {
    const size_t E = (size_t)n_q * (size_t)m;
    const size_t nb = ((size_t)n_d + msim::kCandScanDocs - 1) / msim::kCandScanDocs;
    CandLayout L;
    size_t w = 0;
    L.status = w;   w += 16;                                             // zeroed together with the counts
    L.cnt = w;      w += align16((size_t)n_d * msim::kCandClasses * 4);
    L.bsum = w;     w += align16((2 * nb + 2) * 4);
    L.estart = w;   w += align16(((size_t)n_d + 1) * 4);
    L.istart = w;   w += align16(((size_t)n_d + 1) * 4);
    L.rank = w;     w += align16(E * 4);
    L.entries = w;  w += align16(E * sizeof(int2));
    L.items = w;    w += align16(E * sizeof(msim::CandItem));
    L.total = w;
    return L;
}

// both entries: `width` = the one row width the entry takes (128: K1c, 320: its panel form K1cP)
int fwd_candidates(const char *who, int width, int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q,
                   const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, const int64_t *cand, int m,
                   int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids, unsigned flags,
                   void *workspace, void *stream) {
    if (n_q < 0 || m < 0 || n_d < 0) return fail(MSIM_EINVAL, "negative size (n_q=%d m=%d n_d=%d)", n_q, m, n_d);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (!Qt || !q_off || !q_off_host || (!D && n_d > 0) || !d_off || !cand || !out_scores || !workspace)
        return fail(MSIM_EINVAL, "null pointer argument");
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || dim != width)
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 embeddings of width %d (dtype code %d, dim %d)", who, width, dtype,
                    dim);
    if ((reinterpret_cast<uintptr_t>(Qt) | reinterpret_cast<uintptr_t>(D) | reinterpret_cast<uintptr_t>(workspace)) & 15)
        return fail(MSIM_EINVAL, "Qt, D and workspace must be 16-byte aligned");
    if (ld_cand < m) return fail(MSIM_EINVAL, "ld_cand=%lld < m=%d", (long long)ld_cand, m);
    if (ld_scores < m) return fail(MSIM_EINVAL, "ld_scores=%lld < m=%d", (long long)ld_scores, m);
    if (flags & ~(MSIM_FLAG_REF_ROUNDING)) return fail(MSIM_EINVAL, "unknown flags 0x%x", flags);
    if ((long long)n_q * m > 0x7fffffff) return fail(MSIM_EUNSUPPORTED, "more than 2^31 - 1 entries (n_q=%d x m=%d)", n_q, m);
    if (q_off_host[0] != 0) return fail(MSIM_EINVAL, "q_off[0] must be 0");
    for (int i = 0; i < n_q; ++i) {
        const int len = q_off_host[i + 1] - q_off_host[i];
        if (len < 0) return fail(MSIM_EINVAL, "q_off must be non-decreasing (query %d)", i);
        if (len > msim::kStreamMaxUnits * msim::kUnitTok)
            return fail(MSIM_EUNSUPPORTED, "query %d has %d tokens: %s takes queries of at most %d", i, len, who,
                        msim::kStreamMaxUnits * msim::kUnitTok);
    }
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CandLayout lay = cand_layout(n_q, m, n_d);
    char *ws = static_cast<char *>(workspace);
    int32_t *status = reinterpret_cast<int32_t *>(ws + lay.status);
    int32_t *cnt = reinterpret_cast<int32_t *>(ws + lay.cnt), *bsum = reinterpret_cast<int32_t *>(ws + lay.bsum);
    int32_t *estart = reinterpret_cast<int32_t *>(ws + lay.estart), *istart = reinterpret_cast<int32_t *>(ws + lay.istart);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + lay.rank);
    int2 *entries = reinterpret_cast<int2 *>(ws + lay.entries);
    msim::CandItem *items = reinterpret_cast<msim::CandItem *>(ws + lay.items);
    const long long E = (long long)n_q * m;
    const unsigned eblocks = (unsigned)((E + 255) / 256);
    {
        const long long n16 = (long long)(lay.bsum - lay.status) / 16;     // status word + counters, a multiple of 16 bytes
        const long long blocks = (n16 + 255) / 256;
        hipLaunchKernelGGL(msim::cand_zero_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st,
                           reinterpret_cast<msim::i32x4 *>(status), n16);
    }
    hipLaunchKernelGGL(msim::cand_count_kernel, dim3(eblocks), dim3(256), 0, st, cand, (long long)ld_cand, n_q, m, (long long)id_base, n_d,
                       q_off, cnt, rank, out_scores, (long long)ld_scores, out_ids, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "cand_count_kernel launch: %s", hipGetErrorString(e));
    if (n_d == 0) return MSIM_OK;                  // every entry was out of range
    const int nb = (n_d + msim::kCandScanDocs - 1) / msim::kCandScanDocs;
    hipLaunchKernelGGL(msim::cand_block_sums_kernel, dim3(nb), dim3(256), 0, st, cnt, n_d, bsum);
    hipLaunchKernelGGL(msim::cand_scan_sums_kernel, dim3(1), dim3(256), 0, st, bsum, nb);
    hipLaunchKernelGGL(msim::cand_block_starts_kernel, dim3(nb), dim3(256), 0, st, cnt, n_d, bsum, nb, estart, istart);
    hipLaunchKernelGGL(msim::cand_place_kernel, dim3(eblocks), dim3(256), 0, st, cand, (long long)ld_cand, n_q, m, (long long)id_base, q_off,
                       cnt, rank, estart, istart, n_d, entries, items, status);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "candidate list kernels launch: %s", hipGetErrorString(e));
    // a persistent grid sized from what the host knows: at most one item per entry, as many workgroups per CU as its LDS holds
    // (K1c: two of 72 KiB; K1cP: one of 136 KiB)
    const bool f16 = dtype == MSIM_DTYPE_F16;
    const bool wide = width != msim::kDim;
    auto kern = wide ? (f16 ? msim::maxsim_candidates_panels_kernel<3, 4, true, 0> : msim::maxsim_candidates_panels_kernel<3, 4, false, 0>)
                     : (f16 ? msim::maxsim_candidates_kernel<true, 0> : msim::maxsim_candidates_kernel<false, 0>);
    const int lds_bytes = wide ? msim::kCandPanelLdsBytes : msim::kCandLdsBytes;
    static std::atomic<int> configured[2][2][kMaxDevices];
    if (int rc = allow_lds(kern, lds_bytes, configured[wide][f16])) return rc;
    const long long wg_needed = (E + 3) / 4;
    const long long wg_cap = (long long)di->cus * (di->lds_per_cu / lds_bytes);
    hipLaunchKernelGGL(kern, dim3((unsigned)(wg_needed < wg_cap ? wg_needed : wg_cap)), dim3(256), lds_bytes, st,
                       static_cast<const uint16_t *>(Qt), q_off, static_cast<const uint16_t *>(D), d_off, d_clamp0, entries, items,
                       istart + n_d, (int)E, n_q, m, n_d, out_scores, (long long)ld_scores, flags, status);
    hipLaunchKernelGGL(msim::cand_poison_kernel, dim3(eblocks), dim3(256), 0, st, status, n_q, m, out_scores, (long long)ld_scores);
    e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "%s: scoring kernel launch: %s", who, hipGetErrorString(e));
    return MSIM_OK;
}

}  // namespace

extern "C" {

size_t msim_fwd_candidates_workspace_bytes(int n_q, int m, int n_d) {
    if (n_q <= 0 || m <= 0 || n_d < 0) return 0;
    return cand_layout(n_q, m, n_d).total;
}

int msim_fwd_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                        const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, const int64_t *cand, int m, int64_t ld_cand,
                        int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids, unsigned flags, void *workspace,
                        void *stream) {
    return fwd_candidates("msim_fwd_candidates", msim::kDim, dtype, Qt, q_off, q_off_host, n_q, D, d_off, d_clamp0, n_d, dim, cand, m,
                          ld_cand, id_base, out_scores, ld_scores, out_ids, flags, workspace, stream);
}

// width 320 (ColQwen3): the inversion into work items does not depend on the row width, so neither does the workspace
size_t msim_fwd_candidates_wide_workspace_bytes(int n_q, int m, int n_d, int dim) {
    (void)dim;
    if (n_q <= 0 || m <= 0 || n_d < 0) return 0;
    return cand_layout(n_q, m, n_d).total;
}

int msim_fwd_candidates_wide(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                             const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, const int64_t *cand, int m,
                             int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids, unsigned flags,
                             void *workspace, void *stream) {
    return fwd_candidates("msim_fwd_candidates_wide", kCandWideDim, dtype, Qt, q_off, q_off_host, n_q, D, d_off, d_clamp0, n_d, dim, cand,
                          m, ld_cand, id_base, out_scores, ld_scores, out_ids, flags, workspace, stream);
}

}  // extern "C"
