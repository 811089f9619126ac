// The host layer of the FP4 index family's C ABI, once for both widths and both query codes: the argument checks of an encode entry
// (msim_f4_/f6_/f4w_/f6w_encode_rows), of a scan entry (msim_f4_/f4w_scores and their _q6) and of a list-form entry (msim_f4_/
// f4w_candidates and their _q6), the scan's launch plan (what msim_f4_/f4w_scores_plan report) and the list form's (what
// msim_f4_/f4w_candidates_plan report).  Host code only, and no kernel file is included here: what a check needs of a kernel file --
// the row width, the tile, the range and token limits -- its unit passes in, so a unit compiles the kernels it includes and no
// other (kernels in bodies of their own, host code shared).
#pragma once
#include "abi_common.hpp"

namespace msim_abi {

// a check's third answer beside MSIM_OK (nothing to do) and a refusal (both <= 0): the arguments are good and there is work to launch
constexpr int kF4Launch = 1;

// what a refusal says of the family: the row width it takes and its name
struct F4Family {
    int dim;
    const char *index;
};
constexpr F4Family kF4Narrow{128, "the fp4 index"}, kF4Wide{320, "the wide fp4 index"};

// the arguments the scan and the list form share (a query code row is e2m1 or e2m3: the checks are the same)
struct F4Queries {
    const uint8_t *codes, *scales;
    const int32_t *off;
    int n_q;
    int64_t rows;
    int max_tokens;
};
struct F4Pages {
    const uint8_t *codes, *scales;
    const int32_t *off;
    const uint8_t *clamp0;
    int n_d;
    int64_t rows;
    int dim;
};

inline int f4_wrong_width(const char *who, const F4Family &fam, int dim) {
    return fail(MSIM_EUNSUPPORTED, "%s: rows of width %d; %s takes width %d", who, dim, fam.index, fam.dim);
}

// an encode entry; `rows_per_wg`: the rows one workgroup of the unit's kernel codes
inline int f4_encode_check(const char *who, const F4Family &fam, int rows_per_wg, int dtype, const void *X, int64_t n_rows, int dim,
                           const uint8_t *codes, const uint8_t *scales) {
    if (n_rows < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%lld)", who, (long long)n_rows);
    if (dim != fam.dim) return f4_wrong_width(who, fam, dim);
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 rows (dtype code %d)", who, dtype);
    if (n_rows == 0) return MSIM_OK;
    if (!X || !codes || !scales) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(X, 16) || misaligned(codes, 16)) return fail(MSIM_EINVAL, "%s: rows and codes must be 16-byte aligned", who);
    if ((n_rows + rows_per_wg - 1) / rows_per_wg > 0x7fffffffLL)
        return fail(MSIM_EUNSUPPORTED, "%s: %lld rows exceed one launch", who, (long long)n_rows);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    return kF4Launch;
}

// The launch form of a scan: every query gets TPQ 16-token tiles, QG queries fill one wave's NT tiles, a longer query takes several
// passes; GW = the waves that share a page range of ppw pages; n_gb x n_pb workgroups.  TILE and MAX_RANGE are the kernel file's.
template <int NT_, int TILE, int MAX_RANGE>
struct F4ScanPlan {
    static constexpr int NT = NT_, D = 4;
    int QG, TPQ, passes, GW, ppw;
    long long n_groups, n_gb, n_pb;

    F4ScanPlan() = default;
    F4ScanPlan(int n_q, int max_q_tokens, int n_d, int cus) {
        const int tiles = max_q_tokens ? (max_q_tokens + TILE - 1) / TILE : 1;
        QG = 1, TPQ = NT, passes = 1;
        if (tiles <= NT) {
            TPQ = tiles;
            QG = NT / tiles;
        } else {
            passes = (tiles + NT - 1) / NT;
        }
        n_groups = ((long long)n_q + QG - 1) / QG;
        GW = n_groups <= 1 ? 1 : n_groups == 2 ? 2 : 4;
        // page ranges: enough waves to fill the chip (8 per CU, ~4 rounds); at most 16 pages a range when several query groups re-read it
        const long long want = (long long)(cus > 0 ? cus : 1) * 32;
        const long long work = n_groups * n_d;
        const int cap = n_groups <= 1 ? MAX_RANGE : 16;
        const long long per = (work + want - 1) / want;
        ppw = (int)(per < 1 ? 1 : per > cap ? cap : per);
        n_gb = (n_groups + GW - 1) / GW;
        n_pb = (((long long)n_d + ppw - 1) / ppw + 4 / GW - 1) / (4 / GW);
    }
};

// a *_scores_plan entry: plan[] = {NT, GW, D, ppw}
template <class Plan>
int f4_scan_plan_entry(const char *who, int n_q, int max_q_tokens, int n_d, int64_t d_rows, int32_t *plan) {
    if (n_q < 0 || n_d < 0 || d_rows < 0 || max_q_tokens < 0 || max_q_tokens > (1 << 20) || !plan)
        return fail(MSIM_EINVAL, "%s: bad argument", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const Plan p(n_q, max_q_tokens, n_d, di->cus);
    plan[0] = Plan::NT;
    plan[1] = p.GW;
    plan[2] = Plan::D;
    plan[3] = p.ppw;
    return MSIM_OK;
}

// a scan entry: kF4Launch and the plan of the launch in *plan
template <class Plan>
int f4_scan_check(const char *who, const F4Family &fam, const F4Queries &q, const F4Pages &d, const float *scores, int64_t ld_scores,
                  Plan *plan) {
    if (q.n_q < 0 || d.n_d < 0 || q.rows < 0 || d.rows < 0 || q.max_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, q.n_q, d.n_d,
                    (long long)q.rows, (long long)d.rows, q.max_tokens);
    if (d.dim != fam.dim) return f4_wrong_width(who, fam, d.dim);
    if (q.n_q == 0 || d.n_d == 0) return MSIM_OK;
    if ((!q.codes && q.rows > 0) || (!q.scales && q.rows > 0) || !q.off || (!d.codes && d.rows > 0) || (!d.scales && d.rows > 0) || !d.off ||
        !scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q.codes, 16) || misaligned(d.codes, 16) || misaligned(q.off, 4) || misaligned(d.off, 4) || misaligned(scores, 4))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; offsets and scores 4-byte aligned", who);
    if (ld_scores < d.n_d) return fail(MSIM_EINVAL, "%s: ld_scores=%lld < n_d=%d", who, (long long)ld_scores, d.n_d);
    if (q.max_tokens > (1 << 20)) return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, q.max_tokens, 1 << 20);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    *plan = Plan(q.n_q, q.max_tokens, d.n_d, di->cus);
    if (plan->n_gb * plan->n_pb > 0x7fffffffLL)
        return fail(MSIM_EUNSUPPORTED, "%s: %lld workgroups exceed one launch", who, plan->n_gb * plan->n_pb);
    return kF4Launch;
}

// The launch form of a list form: NT = the 16-token tiles a wave holds (the smallest of 1, 2, 4, 8 that covers max_q_tokens), one
// workgroup of `waves` waves per `waves` entries.  The chunks a wave loads ahead are the kernel file's to say.
struct F4CandLimits {
    int max_tokens, tile, waves;                   // kF4[w]CandMaxTokens, kF4[w]Tile, kF4[w]CandWaves
};
struct F4CandPlan {
    int NT;
    long long wgs;
};

// MSIM_OK, or the refusal both the plan entry and the scorers give
inline int f4_cand_plan(const char *who, const F4CandLimits &lim, int n_q, int max_q_tokens, int m, F4CandPlan *p) {
    if (n_q < 0 || m < 0 || max_q_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d max_q_tokens=%d)", who, n_q, m, max_q_tokens);
    if (max_q_tokens > lim.max_tokens) return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d above %d", who, max_q_tokens, lim.max_tokens);
    const int tiles = (max_q_tokens + lim.tile - 1) / lim.tile;
    p->NT = tiles <= 1 ? 1 : tiles <= 2 ? 2 : tiles <= 4 ? 4 : 8;
    p->wgs = ((long long)n_q * m + lim.waves - 1) / lim.waves;
    if (p->wgs > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld workgroups exceed one launch", who, p->wgs);
    return MSIM_OK;
}

// a *_candidates_plan entry: plan[] = {NT, D, waves, workgroups}; `depth(NT)`: the chunks a wave of that NT loads ahead
template <class Depth>
int f4_cand_plan_entry(const char *who, const F4CandLimits &lim, Depth depth, int n_q, int max_q_tokens, int m, int32_t *plan) {
    if (!plan) return fail(MSIM_EINVAL, "%s: null plan", who);
    F4CandPlan p;
    if (int rc = f4_cand_plan(who, lim, n_q, max_q_tokens, m, &p)) return rc;
    plan[0] = p.NT;
    plan[1] = depth(p.NT);
    plan[2] = lim.waves;
    plan[3] = (int32_t)p.wgs;
    return MSIM_OK;
}

// a list-form entry: kF4Launch and the plan of the launch in *p
inline int f4_cand_check(const char *who, const F4Family &fam, const F4CandLimits &lim, const F4Queries &q, const F4Pages &d,
                         const int64_t *cand, int m, int64_t ld_cand, const float *out_scores, int64_t ld_scores, const int64_t *out_ids,
                         F4CandPlan *p) {
    if (q.n_q < 0 || d.n_d < 0 || m < 0 || q.rows < 0 || d.rows < 0 || q.max_tokens < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n_d=%d m=%d q_rows=%lld d_rows=%lld max_q_tokens=%d)", who, q.n_q, d.n_d, m,
                    (long long)q.rows, (long long)d.rows, q.max_tokens);
    if (d.dim != fam.dim) return f4_wrong_width(who, fam, d.dim);
    if (q.n_q == 0 || m == 0) return MSIM_OK;
    if ((!q.codes && q.rows > 0) || (!q.scales && q.rows > 0) || !q.off || (!d.codes && d.rows > 0) || (!d.scales && d.rows > 0) ||
        (!d.off && d.n_d > 0) || !cand || !out_scores)
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(q.codes, 16) || misaligned(d.codes, 16) || misaligned(q.off, 4) || misaligned(d.off, 4) || misaligned(out_scores, 4) ||
        misaligned(cand, 8) || misaligned(out_ids, 8))
        return fail(MSIM_EINVAL, "%s: codes must be 16-byte aligned; ids 8-byte aligned; offsets and scores 4-byte aligned", who);
    if (ld_cand < m || ld_scores < m)
        return fail(MSIM_EINVAL, "%s: ld_cand=%lld / ld_scores=%lld < m=%d", who, (long long)ld_cand, (long long)ld_scores, m);
    if (int rc = f4_cand_plan(who, lim, q.n_q, q.max_tokens, m, p)) return rc;
    return kF4Launch;
}

}  // namespace msim_abi
