// C ABI of libmaxsim_gfx950.so (see include/maxsim.h): search over the resident corpus -- top-k, the live corpus, hard-negative
// mining and the page gather, page filters, document-level search and token-to-patch alignment.
// Host-side dispatch only: argument validation, kernel selection and launch on the caller's stream.  Nothing here allocates,
// frees or synchronises, so every entry point is hipGraph-capturable.  The kernels included below are defined and launched in
// this translation unit and in no other.
#include <hip/hip_runtime.h>

#include <atomic>

#include "../../include/maxsim.h"
#include "abi_common.hpp"
#include "topk_select.hip"
#include "live_corpus.hip"
#include "mine.hip"
#include "filter.hip"
#include "group.hip"
#include "maxsim_align.hip"

using namespace msim_abi;

extern "C" {

// ---------------------------------------------------------------- top-k selection
// Level plan: level 0 splits each row into segments of `seg0` candidates (a power of two chosen so that the
// launch has enough workgroups to fill the chip even for a single row); later levels use full segments.

// level 0 as the streaming threshold filter (topk_select.hip: topk_filter_kernel): rows of raw scores long enough for it, few
// enough winners per row, and enough (row, segment) workgroups to fill the chip -- the many-query regime, where the bitonic level
// was the one kernel of the timed step two orders off its roof
static bool topk_use_filter(const int64_t *ids, int n_q, long long n, int k) {
    if (ids != nullptr || k > msim::kTopkFilterMaxK || n < (long long)msim::kTopkFilterSeg) return false;
    return (long long)n_q * ((n + msim::kTopkFilterSeg - 1) / msim::kTopkFilterSeg) >= 512;      // two workgroups per CU at least
}

static int topk_first_segment(int n_q, long long n, int k) {
    int seg = 512;
    while (seg < 4 * k) seg <<= 1;                       // every level must shrink its input at least 4x
    while (seg < msim::kTopkSeg && (long long)n_q * ((n + seg - 1) / seg) > 1024) seg <<= 1;   // ~4 workgroups per CU is plenty
    return seg;
}
static inline long long topk_level_out(long long n, int seg, int k) { return ((n + seg - 1) / seg) * (long long)k; }
// Later levels: the smallest legal segment.  A bitonic sort of s candidates costs ~log2(s)^2 / 2 barrier-separated stages of s / 512
// passes each, so two levels of 512 (45 stages + a tiny final sort) beat one 4096-candidate sort (78 stages x 8 passes) several
// times over -- the single-workgroup last level was 157 us of a 200 us top-k at 4 queries x 125 000 documents.
static int topk_later_segment(int k) {
    int seg = 512;
    while (seg < 4 * k) seg <<= 1;
    return seg;
}
// one more workgroup-per-segment level only while the row is longer than two segments; otherwise one workgroup finishes the row
static inline bool topk_is_last(long long n, int seg) { return n <= 2LL * seg && n <= msim::kTopkSeg; }

static size_t topk_plan_bytes(int n_q, long long n, int k, int seg0) {
    if (topk_is_last(n, seg0)) return 0;
    const int seg1 = topk_later_segment(k);
    const long long na = topk_level_out(n, seg0, k);
    const long long nb = topk_is_last(na, seg1) ? 0 : topk_level_out(na, seg1, k);
    return align16((size_t)n_q * na * 4) + align16((size_t)n_q * na * 8) + align16((size_t)n_q * nb * 4) +
           align16((size_t)n_q * nb * 8);
}

size_t msim_topk_workspace_bytes(int n_q, int64_t n, int k) {
    if (n_q <= 0 || k <= 0 || k > msim::kTopkMaxK) return 0;
    // the same problem takes the filter level without explicit ids and the plain level with them: room for either
    size_t need = topk_plan_bytes(n_q, n, k, topk_first_segment(n_q, n, k));
    if (topk_use_filter(nullptr, n_q, n, k)) {
        const size_t f = topk_plan_bytes(n_q, n, k, msim::kTopkFilterSeg);
        if (f > need) need = f;
    }
    return need;
}

int msim_topk_f32(const float *scores, const int64_t *ids, int n_q, int64_t n, int64_t ld, int k, int64_t id_base,
                  float *out_scores, int64_t *out_ids, void *workspace, void *stream) {
    if (n_q < 0 || n < 0 || k <= 0) return fail(MSIM_EINVAL, "bad size (n_q=%d n=%lld k=%d)", n_q, (long long)n, k);
    if (n_q == 0) return MSIM_OK;
    if (!out_scores || !out_ids || (n > 0 && !scores)) return fail(MSIM_EINVAL, "null pointer argument");
    if (k > msim::kTopkMaxK) return fail(MSIM_EUNSUPPORTED, "k=%d > %d", k, msim::kTopkMaxK);
    if (ld < n) return fail(MSIM_EINVAL, "ld=%lld < n=%lld", (long long)ld, (long long)n);
    const bool filter0 = topk_use_filter(ids, n_q, n, k);
    const int seg0 = filter0 ? msim::kTopkFilterSeg : topk_first_segment(n_q, n, k);
    const int seg1 = topk_later_segment(k);
    if (!topk_is_last(n, seg0) && !workspace) return fail(MSIM_EINVAL, "workspace required (msim_topk_workspace_bytes)");
    hipStream_t st = static_cast<hipStream_t>(stream);

    const long long na = topk_is_last(n, seg0) ? 0 : topk_level_out(n, seg0, k);
    const long long nb = (na == 0 || topk_is_last(na, seg1)) ? 0 : topk_level_out(na, seg1, k);
    char *w = static_cast<char *>(workspace);
    float *bufs_s[2];
    int64_t *bufs_i[2];
    long long bufs_ld[2] = {na, nb};
    bufs_s[0] = reinterpret_cast<float *>(w);
    w += align16((size_t)n_q * na * 4);
    bufs_i[0] = reinterpret_cast<int64_t *>(w);
    w += align16((size_t)n_q * na * 8);
    bufs_s[1] = reinterpret_cast<float *>(w);
    w += align16((size_t)n_q * nb * 4);
    bufs_i[1] = reinterpret_cast<int64_t *>(w);

    const float *in_s = scores;
    const int64_t *in_i = ids;
    long long in_n = n, in_ld = ld, in_base = id_base;
    int which = 0, seg = seg0;
    for (;;) {
        const bool last = topk_is_last(in_n, seg);
        const long long segs = last ? 1 : (in_n + seg - 1) / seg;
        float *o_s = last ? out_scores : bufs_s[which];
        int64_t *o_i = last ? out_ids : bufs_i[which];
        const long long o_ld = last ? k : segs * k;
        if (!last && o_ld > bufs_ld[which]) return fail(MSIM_ELAUNCH, "internal: top-k level does not fit its buffer");
        for (int r0 = 0; r0 < n_q; r0 += 65535) {   // grid.y limit
            const int rows = (n_q - r0 < 65535) ? (n_q - r0) : 65535;
            if (filter0 && in_s == scores) {        // level 0: the streaming filter
                hipLaunchKernelGGL(msim::topk_filter_kernel, dim3((unsigned)segs, (unsigned)rows), dim3(msim::kTopkThreads), 0, st,
                                   in_s + (size_t)r0 * in_ld, in_n, in_ld, in_base, k, o_s + (size_t)r0 * o_ld, o_i + (size_t)r0 * o_ld, o_ld);
                continue;
            }
            hipLaunchKernelGGL(msim::topk_segment_kernel, dim3((unsigned)segs, (unsigned)rows), dim3(msim::kTopkThreads), 0, st,
                               in_s + (size_t)r0 * in_ld, in_i ? in_i + (size_t)r0 * in_ld : nullptr, in_n, in_ld, in_base, k,
                               last ? msim::kTopkSeg : seg, o_s + (size_t)r0 * o_ld, o_i + (size_t)r0 * o_ld, o_ld);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return fail(MSIM_ELAUNCH, "topk_segment_kernel launch: %s", hipGetErrorString(e));
        if (last) break;
        in_s = o_s;
        in_i = o_i;
        in_n = o_ld;
        in_ld = o_ld;
        in_base = 0;
        which ^= 1;
        seg = seg1;
    }
    return MSIM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- the live corpus (live_corpus.hip)
namespace {

constexpr int64_t kLiveMaxRowBytes = 65536;
constexpr int64_t kLiveMaxChunks = 1 << 16;          // two launches per chunk: a bounce buffer of a few rows is for small corpora

struct LiveWorkspace {
    size_t old_off, tile_sum, tile_base, total;
    int n_tiles;
};

LiveWorkspace live_workspace(int n_slots) {
    LiveWorkspace w;
    w.n_tiles = (n_slots + msim::kLiveTile - 1) / msim::kLiveTile;
    w.old_off = align16(msim::kLiveHeaderWords * sizeof(int32_t));
    w.tile_sum = w.old_off + align16(((size_t)n_slots + 1) * sizeof(int32_t));
    w.tile_base = w.tile_sum + align16((size_t)w.n_tiles * sizeof(long long));
    w.total = w.tile_base + align16((size_t)w.n_tiles * sizeof(long long));
    return w;
}

// What msim_live_compact and msim_res_live_compact share.  An entry refuses its own row format between the two checks (the second
// takes what it found on its own row arrays), returns MSIM_OK after them where there are no slots, and refuses a small bounce buffer itself.
int live_check_sizes(const char *who, int n_slots, int64_t rows_bound, int64_t bounce_bytes) {
    if (n_slots >= 0 && rows_bound >= 0 && bounce_bytes >= 0) return MSIM_OK;
    return fail(MSIM_EINVAL, "%s: negative size (n_slots=%d rows_bound=%lld bounce_bytes=%lld)", who, n_slots, (long long)rows_bound,
                (long long)bounce_bytes);
}

int live_check_args(const char *who, int n_slots, int64_t rows_bound, const int32_t *off, const uint8_t *alive, const int64_t *rows_used_out,
                    const void *workspace, const void *bounce, bool arrays_null, bool arrays_misaligned, const char *arrays) {
    if (rows_bound > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: rows_bound=%lld above 2^31 - 1", who, (long long)rows_bound);
    if (n_slots == 0) return MSIM_OK;
    if (!off || !alive || !rows_used_out || !workspace || ((arrays_null || !bounce) && rows_bound > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (arrays_misaligned || misaligned(bounce, 16) || misaligned(workspace, 16) || misaligned(off, 4) || misaligned(rows_used_out, 8))
        return fail(MSIM_EINVAL, "%s: %s, bounce and workspace must be 16-byte aligned, off 4-byte and rows_used_out 8-byte aligned", who,
                    arrays);
    return MSIM_OK;
}

// What the move loops of both run against, in two steps.  The chunking rule: a chunk is the destination rows that fit the bounce buffer
// at `unit_bytes` each.  The offset plan: carve the workspace, launch reset / lens / scan / apply; `off` then holds the new offsets.
struct LivePlan {
    int64_t chunk_rows, n_chunks;
    int32_t *hdr, *old_off;          // the status words that the move kernels obey; the offsets as they were
};

int live_plan(const char *who, hipStream_t st, void *workspace, int32_t *off, const uint8_t *alive, int n_slots, int64_t rows_bound,
              int64_t *rows_used_out, int64_t bounce_bytes, int64_t unit_bytes, LivePlan *p) {
    p->chunk_rows = rows_bound > 0 ? bounce_bytes / unit_bytes : 1;
    if (p->chunk_rows > (1 << 30)) p->chunk_rows = 1 << 30;
    p->n_chunks = (rows_bound + p->chunk_rows - 1) / p->chunk_rows;
    if (p->n_chunks > kLiveMaxChunks)
        return fail(MSIM_EUNSUPPORTED, "%s: %lld rows through a bounce buffer of %lld rows are %lld chunks (at most %lld)", who,
                    (long long)rows_bound, (long long)p->chunk_rows, (long long)p->n_chunks, (long long)kLiveMaxChunks);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    const LiveWorkspace w = live_workspace(n_slots);
    char *ws = static_cast<char *>(workspace);
    int32_t *hdr = p->hdr = reinterpret_cast<int32_t *>(ws);
    int32_t *old_off = p->old_off = reinterpret_cast<int32_t *>(ws + w.old_off);
    long long *tile_sum = reinterpret_cast<long long *>(ws + w.tile_sum);
    long long *tile_base = reinterpret_cast<long long *>(ws + w.tile_base);
    hipLaunchKernelGGL(msim::live_reset_kernel, dim3(1), dim3(64), 0, st, hdr);
    hipLaunchKernelGGL(msim::live_lens_kernel, dim3((unsigned)w.n_tiles), dim3(msim::kLiveTile), 0, st, off, alive, n_slots,
                       (long long)rows_bound, hdr, old_off, tile_sum);
    hipLaunchKernelGGL(msim::live_scan_kernel, dim3(1), dim3(msim::kLiveTile), 0, st, w.n_tiles, n_slots, (long long)rows_bound, hdr,
                       old_off, tile_sum, tile_base, reinterpret_cast<long long *>(rows_used_out));
    hipLaunchKernelGGL(msim::live_apply_kernel, dim3((unsigned)w.n_tiles), dim3(msim::kLiveTile), 0, st, off, alive, n_slots, hdr, old_off,
                       tile_base);
    return MSIM_OK;
}

}  // namespace

extern "C" {

size_t msim_live_compact_workspace_bytes(int n_slots, int64_t bounce_bytes) {
    (void)bounce_bytes;                                // the bounce buffer is the caller's; the workspace holds the slot tables only
    return n_slots <= 0 ? 0 : live_workspace(n_slots).total;
}

int msim_live_compact(void *rows, int64_t row_bytes, int64_t rows_bound, int32_t *off, const uint8_t *alive, int n_slots,
                      int64_t *rows_used_out, void *workspace, void *bounce, int64_t bounce_bytes, void *stream) {
    const char *who = "msim_live_compact";
    if (int rc = live_check_sizes(who, n_slots, rows_bound, bounce_bytes)) return rc;
    if (row_bytes <= 0 || row_bytes % 16 != 0)
        return fail(MSIM_EINVAL, "%s: row_bytes=%lld must be a positive multiple of 16", who, (long long)row_bytes);
    if (row_bytes > kLiveMaxRowBytes)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of %lld bytes (at most %lld)", who, (long long)row_bytes, (long long)kLiveMaxRowBytes);
    if (int rc = live_check_args(who, n_slots, rows_bound, off, alive, rows_used_out, workspace, bounce, !rows, misaligned(rows, 16), "rows"))
        return rc;
    if (n_slots == 0) return MSIM_OK;
    if (rows_bound > 0 && bounce_bytes < row_bytes)
        return fail(MSIM_EINVAL, "%s: a bounce buffer of %lld bytes holds no row of %lld bytes", who, (long long)bounce_bytes,
                    (long long)row_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LivePlan p;
    if (int rc = live_plan(who, st, workspace, off, alive, n_slots, rows_bound, rows_used_out, bounce_bytes, row_bytes, &p)) return rc;
    int block_rows = (int)(msim::kLiveBlockBytes / row_bytes);
    block_rows = block_rows < 1 ? 1 : block_rows > msim::kLiveMaxBlockRows ? msim::kLiveMaxBlockRows : block_rows;
    const int lpr = (int)(row_bytes / 16);
    for (int64_t k = 0; k < p.n_chunks; ++k) {
        const long long chunk0 = k * p.chunk_rows;
        const int rows_here = (int)(rows_bound - chunk0 < p.chunk_rows ? rows_bound - chunk0 : p.chunk_rows);
        const unsigned blocks = (unsigned)((rows_here + block_rows - 1) / block_rows);
        hipLaunchKernelGGL(msim::live_move_kernel<true>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, static_cast<uint8_t *>(rows),
                           lpr, (long long)rows_bound, off, p.old_off, n_slots, p.hdr, static_cast<uint8_t *>(bounce), chunk0,
                           rows_here, block_rows);
        hipLaunchKernelGGL(msim::live_move_kernel<false>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, static_cast<uint8_t *>(rows),
                           lpr, (long long)rows_bound, off, p.old_off, n_slots, p.hdr, static_cast<uint8_t *>(bounce), chunk0,
                           rows_here, block_rows);
    }
    return launch_failed("live compaction");
}

size_t msim_res_live_compact_workspace_bytes(int n_slots, int64_t b) { return msim_live_compact_workspace_bytes(n_slots, b); }

// One offset plan, two arrays moved against it.  A chunk is floor(bounce_bytes / (16 bits + 2)) destination rows: the bounce buffer
// holds the chunk's residual rows first (16 bits bytes each, so the codes behind them start 16-byte aligned) and its codes after them.
int msim_res_live_compact(uint16_t *codes, uint8_t *residuals, int bits, int64_t rows_bound, int32_t *off, const uint8_t *alive,
                          int n_slots, int64_t *rows_used_out, void *workspace, void *bounce, int64_t bounce_bytes, void *stream) {
    const char *who = "msim_res_live_compact";
    if (int rc = live_check_sizes(who, n_slots, rows_bound, bounce_bytes)) return rc;
    if (!(bits == 2 || bits == 4)) return fail(MSIM_EUNSUPPORTED, "%s: %d residual bits; the codec stores 2 or 4 per dimension", who, bits);
    if (int rc = live_check_args(who, n_slots, rows_bound, off, alive, rows_used_out, workspace, bounce, !codes || !residuals,
                                 misaligned(codes, 16) || misaligned(residuals, 16), "codes, residuals"))
        return rc;
    if (n_slots == 0) return MSIM_OK;
    const int64_t res_bytes = 16 * bits, both_bytes = res_bytes + 2;
    if (rows_bound > 0 && bounce_bytes < both_bytes)
        return fail(MSIM_EINVAL, "%s: a bounce buffer of %lld bytes holds no row of %lld + 2 bytes", who, (long long)bounce_bytes,
                    (long long)res_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LivePlan p;
    if (int rc = live_plan(who, st, workspace, off, alive, n_slots, rows_bound, rows_used_out, bounce_bytes, both_bytes, &p)) return rc;
    const int block_rows = msim::kLiveMaxBlockRows;      // 256 rows of 32 / 64 bytes: 8 / 16 KiB per workgroup
    constexpr int code_block_rows = msim::kLiveMoveThreads * msim::kLiveCodeRows;
    const int lpr = bits;                                // 16-byte pieces per residual row
    uint8_t *bounce_res = static_cast<uint8_t *>(bounce);
    uint16_t *bounce_codes = reinterpret_cast<uint16_t *>(bounce_res + p.chunk_rows * res_bytes);
    for (int64_t k = 0; k < p.n_chunks; ++k) {
        const long long chunk0 = k * p.chunk_rows;
        const int rows_here = (int)(rows_bound - chunk0 < p.chunk_rows ? rows_bound - chunk0 : p.chunk_rows);
        const unsigned blocks = (unsigned)((rows_here + block_rows - 1) / block_rows);
        const unsigned cblocks = (unsigned)((rows_here + code_block_rows - 1) / code_block_rows);
        hipLaunchKernelGGL(msim::live_move_kernel<true>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, residuals, lpr,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_res, chunk0, rows_here, block_rows);
        hipLaunchKernelGGL(msim::live_move_codes_kernel<true>, dim3(cblocks), dim3(msim::kLiveMoveThreads), 0, st, codes,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_codes, chunk0, rows_here);
        hipLaunchKernelGGL(msim::live_move_kernel<false>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, residuals, lpr,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_res, chunk0, rows_here, block_rows);
        hipLaunchKernelGGL(msim::live_move_codes_kernel<false>, dim3(cblocks), dim3(msim::kLiveMoveThreads), 0, st, codes,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_codes, chunk0, rows_here);
    }
    return launch_failed("live compaction of a compressed shard");
}

size_t msim_f4_live_compact_workspace_bytes(int n_slots, int64_t b) { return msim_live_compact_workspace_bytes(n_slots, b); }

// One offset plan, two arrays moved against it: the FP4 code rows (64 or 160 bytes) and the scale bytes of a live FP4 index.  A chunk is
// floor(bounce_bytes / (code_row_bytes + 1)) destination rows: the bounce buffer holds the chunk's code rows first (a multiple of 16
// bytes each, so the scale bytes behind them start 16-byte aligned; they need no alignment) and its scale bytes after them.
int msim_f4_live_compact(uint8_t *codes, int64_t code_row_bytes, uint8_t *scales, int64_t rows_bound, int32_t *off, const uint8_t *alive,
                         int n_slots, int64_t *rows_used_out, void *workspace, void *bounce, int64_t bounce_bytes, void *stream) {
    const char *who = "msim_f4_live_compact";
    if (int rc = live_check_sizes(who, n_slots, rows_bound, bounce_bytes)) return rc;
    if (!(code_row_bytes == 64 || code_row_bytes == 160))
        return fail(MSIM_EUNSUPPORTED, "%s: code rows of %lld bytes; an fp4 index stores 64 (width 128) or 160 (width 320)", who,
                    (long long)code_row_bytes);
    if (int rc = live_check_args(who, n_slots, rows_bound, off, alive, rows_used_out, workspace, bounce, !codes || !scales,
                                 misaligned(codes, 16), "codes"))
        return rc;
    if (n_slots == 0) return MSIM_OK;
    const int64_t both_bytes = code_row_bytes + 1;
    if (rows_bound > 0 && bounce_bytes < both_bytes)
        return fail(MSIM_EINVAL, "%s: a bounce buffer of %lld bytes holds no row of %lld + 1 bytes", who, (long long)bounce_bytes,
                    (long long)code_row_bytes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    LivePlan p;
    if (int rc = live_plan(who, st, workspace, off, alive, n_slots, rows_bound, rows_used_out, bounce_bytes, both_bytes, &p)) return rc;
    int block_rows = (int)(msim::kLiveBlockBytes / code_row_bytes);          // 256 rows of 64 bytes, 102 of 160: 16 KiB per workgroup
    block_rows = block_rows > msim::kLiveMaxBlockRows ? msim::kLiveMaxBlockRows : block_rows;
    constexpr int scale_block_rows = msim::kLiveMoveThreads * msim::kLiveCodeRows;
    const int lpr = (int)(code_row_bytes / 16);
    uint8_t *bounce_codes = static_cast<uint8_t *>(bounce);
    uint8_t *bounce_scales = bounce_codes + p.chunk_rows * code_row_bytes;
    for (int64_t k = 0; k < p.n_chunks; ++k) {
        const long long chunk0 = k * p.chunk_rows;
        const int rows_here = (int)(rows_bound - chunk0 < p.chunk_rows ? rows_bound - chunk0 : p.chunk_rows);
        const unsigned blocks = (unsigned)((rows_here + block_rows - 1) / block_rows);
        const unsigned sblocks = (unsigned)((rows_here + scale_block_rows - 1) / scale_block_rows);
        hipLaunchKernelGGL(msim::live_move_kernel<true>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, codes, lpr,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_codes, chunk0, rows_here, block_rows);
        hipLaunchKernelGGL(msim::live_move_bytes_kernel<true>, dim3(sblocks), dim3(msim::kLiveMoveThreads), 0, st, scales,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_scales, chunk0, rows_here);
        hipLaunchKernelGGL(msim::live_move_kernel<false>, dim3(blocks), dim3(msim::kLiveMoveThreads), 0, st, codes, lpr,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_codes, chunk0, rows_here, block_rows);
        hipLaunchKernelGGL(msim::live_move_bytes_kernel<false>, dim3(sblocks), dim3(msim::kLiveMoveThreads), 0, st, scales,
                           (long long)rows_bound, off, p.old_off, n_slots, p.hdr, bounce_scales, chunk0, rows_here);
    }
    return launch_failed("live compaction of an fp4 index");
}

int msim_live_mask_scores(float *scores, int64_t ld, int n_q, int64_t n, const uint8_t *alive, void *stream) {
    const char *who = "msim_live_mask_scores";
    if (n_q < 0 || n < 0) return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n=%lld)", who, n_q, (long long)n);
    if (n_q == 0 || n == 0) return MSIM_OK;
    if (!scores || !alive) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(scores, 4)) return fail(MSIM_EINVAL, "%s: scores must be 4-byte aligned", who);
    if (ld < n) return fail(MSIM_EINVAL, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    const int64_t tiles = (n + 1023) / 1024;
    if (tiles > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld columns exceed one launch", who, (long long)n);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec_ok = !misaligned(scores, 16) && ld % 4 == 0;
    const unsigned row_groups = (unsigned)(n_q < 64 ? n_q : 64);
    hipLaunchKernelGGL(msim::live_mask_kernel, dim3((unsigned)tiles, row_groups), dim3(256), 0, st, scores, (long long)ld, n_q, (long long)n,
                       alive, vec_ok);
    return launch_failed("live_mask_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- hard-negative mining and the page gather (mine.hip)
namespace {

// what msim_mine_bounds and msim_mine_mask share: the score matrix and the positives list
int mine_check(const char *who, const float *scores, int64_t ld, int n_q, int64_t n, const int64_t *pos_ids, const int32_t *pos_off,
               int64_t nnz) {
    if (n_q < 0 || n < 0 || nnz < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n=%lld nnz=%lld)", who, n_q, (long long)n, (long long)nnz);
    if (n_q == 0) return MSIM_OK;
    if (!pos_off || (nnz > 0 && !pos_ids) || (n > 0 && !scores)) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(scores, 4) || misaligned(pos_off, 4) || misaligned(pos_ids, 8))
        return fail(MSIM_EINVAL, "%s: scores and pos_off must be 4-byte aligned, pos_ids 8-byte aligned", who);
    if (ld < n) return fail(MSIM_EINVAL, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_mine_bounds(const float *scores, int64_t ld, int n_q, int64_t n, const int64_t *pos_ids, const int32_t *pos_off, int64_t nnz,
                     int64_t id_base, const uint8_t *alive, int local, float *bounds, void *stream) {
    const char *who = "msim_mine_bounds";
    if (int rc = mine_check(who, scores, ld, n_q, n, pos_ids, pos_off, nnz)) return rc;
    if (n_q == 0) return MSIM_OK;
    if (!bounds || misaligned(bounds, 4)) return fail(MSIM_EINVAL, "%s: bounds must be a 4-byte aligned pointer", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned blocks = (unsigned)((n_q + 3) / 4);
    hipLaunchKernelGGL(msim::mine_bounds_kernel, dim3(blocks), dim3(msim::kMineThreads), 0, st, scores, (long long)ld, n_q, (long long)n,
                       pos_ids, pos_off, (long long)nnz, (long long)id_base, alive, local != 0, bounds);
    return launch_failed("mine_bounds_kernel");
}

int msim_mine_mask(float *scores, int64_t ld, int n_q, int64_t n, const float *bounds, float max_ratio, const uint8_t *alive,
                   const int64_t *pos_ids, const int32_t *pos_off, int64_t nnz, int64_t id_base, void *stream) {
    const char *who = "msim_mine_mask";
    if (int rc = mine_check(who, scores, ld, n_q, n, pos_ids, pos_off, nnz)) return rc;
    if (n_q == 0 || n == 0) return MSIM_OK;
    if (misaligned(bounds, 4)) return fail(MSIM_EINVAL, "%s: bounds must be 4-byte aligned", who);
    if (bounds && max_ratio != max_ratio) return fail(MSIM_EINVAL, "%s: max_ratio is NaN", who);
    const int64_t all_tiles = (n + msim::kMineTileCols - 1) / msim::kMineTileCols;
    if (all_tiles >= 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld columns exceed one launch", who, (long long)n);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned tiles = (bounds || alive) ? (unsigned)all_tiles : 0u;     // neither: only the positives' columns change
    const int vec_ok = !misaligned(scores, 16) && ld % 4 == 0;
    const unsigned row_groups = (unsigned)(n_q < msim::kMineRowGroups ? n_q : msim::kMineRowGroups);
    auto kern = bounds ? msim::mine_mask_kernel<true> : msim::mine_mask_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(tiles + 1, row_groups), dim3(msim::kMineThreads), 0, st, scores, (long long)ld, n_q, (long long)n, bounds,
                       max_ratio, alive, pos_ids, pos_off, (long long)nnz, (long long)id_base, tiles, vec_ok);
    return launch_failed("mine_mask_kernel");
}

int msim_gather_pages(const void *rows, int64_t row_bytes, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base,
                      const int64_t *ids, int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream) {
    const char *who = "msim_gather_pages";
    if (n_slots < 0 || n_d < 0 || d_rows < 0 || pad_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_slots=%lld n_d=%d d_rows=%lld pad_rows=%lld)", who, (long long)n_slots, n_d,
                    (long long)d_rows, (long long)pad_rows);
    if (row_bytes <= 0 || row_bytes % 16 != 0)
        return fail(MSIM_EINVAL, "%s: row_bytes=%lld must be a positive multiple of 16", who, (long long)row_bytes);
    if (row_bytes > kLiveMaxRowBytes)
        return fail(MSIM_EUNSUPPORTED, "%s: rows of %lld bytes (at most %lld)", who, (long long)row_bytes, (long long)kLiveMaxRowBytes);
    if (d_rows > 0x7fffffffLL || pad_rows > 0x7fffffffLL || n_slots > 0x7fffffffLL)
        return fail(MSIM_EUNSUPPORTED, "%s: d_rows=%lld, pad_rows=%lld or n_slots=%lld above 2^31 - 1", who, (long long)d_rows,
                    (long long)pad_rows, (long long)n_slots);
    if (n_slots == 0) return MSIM_OK;
    if (!ids || !lengths || !d_off || (!rows && d_rows > 0) || (!out && pad_rows > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(rows, 16) || misaligned(out, 16) || misaligned(ids, 8) || misaligned(d_off, 4) || misaligned(lengths, 4))
        return fail(MSIM_EINVAL, "%s: rows and out must be 16-byte aligned, ids 8-byte, d_off and lengths 4-byte aligned", who);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(msim::gather_pages_kernel, dim3((unsigned)n_slots), dim3(msim::kMineThreads), 0, st,
                       static_cast<const uint8_t *>(rows), (int)(row_bytes / 16), (long long)d_rows, d_off, n_d, (long long)id_base, ids,
                       (long long)pad_rows, static_cast<uint8_t *>(out), lengths);
    return launch_failed("gather_pages_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- page filters (filter.hip)
namespace {

// what msim_filter_mask / _list / _ids share: sizes first, then (n_q == 0 || n == 0: nothing to do, *done = true), then the filter
int filter_check(const char *who, int n_q, int64_t n, const uint32_t *bits, int64_t ld_words, const int32_t *page_labels,
                 const int32_t *query_labels, const uint8_t *alive, msim::FilterArgs *f, int *mode, bool *done) {
    *done = false;
    if (n_q < 0 || n < 0 || ld_words < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n=%lld ld_words=%lld)", who, n_q, (long long)n, (long long)ld_words);
    if (n_q == 0 || n == 0) {
        *done = true;
        return MSIM_OK;
    }
    if (n > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: n=%lld above 2^31 - 1", who, (long long)n);
    const bool labels = page_labels || query_labels;
    if ((bits != nullptr) == labels)
        return fail(MSIM_EINVAL, "%s: exactly one of (bits) and (page_labels, query_labels) must be given", who);
    if (labels && (!page_labels || !query_labels)) return fail(MSIM_EINVAL, "%s: page_labels and query_labels go together", who);
    if (misaligned(bits, 4) || misaligned(page_labels, 4) || misaligned(query_labels, 4))
        return fail(MSIM_EINVAL, "%s: bits, page_labels and query_labels must be 4-byte aligned", who);
    if (bits && ld_words != 0 && ld_words < (n + 31) / 32)
        return fail(MSIM_EINVAL, "%s: ld_words=%lld < ceil(n / 32)=%lld", who, (long long)ld_words, (long long)((n + 31) / 32));
    *f = msim::FilterArgs{bits, (long long)ld_words, page_labels, query_labels, alive};
    *mode = labels ? msim::kFilterLabels : ld_words ? msim::kFilterPerQuery : msim::kFilterShared;
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_filter_pack(const uint8_t *mask, int64_t ld_mask, int rows, int64_t n, uint32_t *words, int64_t ld_words, void *stream) {
    const char *who = "msim_filter_pack";
    if (rows < 0 || n < 0) return fail(MSIM_EINVAL, "%s: negative size (rows=%d n=%lld)", who, rows, (long long)n);
    if (rows == 0 || n == 0) return MSIM_OK;
    if (!mask || !words) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(words, 4)) return fail(MSIM_EINVAL, "%s: words must be 4-byte aligned", who);
    if (ld_mask < n) return fail(MSIM_EINVAL, "%s: ld_mask=%lld < n=%lld", who, (long long)ld_mask, (long long)n);
    if (ld_words < (n + 31) / 32)
        return fail(MSIM_EINVAL, "%s: ld_words=%lld < ceil(n / 32)=%lld", who, (long long)ld_words, (long long)((n + 31) / 32));
    const int64_t tiles = (n + msim::kFilterTileCols - 1) / msim::kFilterTileCols;
    if (tiles > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld columns exceed one launch", who, (long long)n);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec_ok = !misaligned(mask, 4) && (ld_mask % 4 == 0 || rows == 1);
    const unsigned row_groups = (unsigned)(rows < msim::kFilterRowGroups ? rows : msim::kFilterRowGroups);
    hipLaunchKernelGGL(msim::filter_pack_kernel, dim3((unsigned)tiles, row_groups), dim3(msim::kFilterThreads), 0, st, mask,
                       (long long)ld_mask, rows, (long long)n, words, (long long)ld_words, vec_ok);
    return launch_failed("filter_pack_kernel");
}

int msim_filter_mask(float *scores, int64_t ld, int n_q, int64_t n, const uint32_t *bits, int64_t ld_words, const int32_t *page_labels,
                     const int32_t *query_labels, const uint8_t *alive, void *stream) {
    const char *who = "msim_filter_mask";
    msim::FilterArgs f;
    int mode = 0;
    bool done = false;
    if (int rc = filter_check(who, n_q, n, bits, ld_words, page_labels, query_labels, alive, &f, &mode, &done)) return rc;
    if (done) return MSIM_OK;
    if (!scores || misaligned(scores, 4)) return fail(MSIM_EINVAL, "%s: scores must be a 4-byte aligned pointer", who);
    if (ld < n) return fail(MSIM_EINVAL, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    const int64_t tiles = (n + msim::kFilterTileCols - 1) / msim::kFilterTileCols;
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int vec_ok = !misaligned(scores, 16) && (ld % 4 == 0 || n_q == 1);
    const int labels_vec_ok = !misaligned(page_labels, 16);
    const unsigned row_groups = (unsigned)(n_q < msim::kFilterRowGroups ? n_q : msim::kFilterRowGroups);
    auto kern = mode == msim::kFilterLabels     ? msim::filter_mask_kernel<msim::kFilterLabels>
                : mode == msim::kFilterPerQuery ? msim::filter_mask_kernel<msim::kFilterPerQuery>
                                                : msim::filter_mask_kernel<msim::kFilterShared>;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, row_groups), dim3(msim::kFilterThreads), 0, st, scores, (long long)ld, n_q, (long long)n,
                       f, vec_ok, labels_vec_ok);
    return launch_failed("filter_mask_kernel");
}

size_t msim_filter_list_workspace_bytes(int n_q, int64_t n) {
    (void)n_q, (void)n;
    return 16;                                           // the status word
}

int msim_filter_list(const uint32_t *bits, int64_t ld_words, const int32_t *page_labels, const int32_t *query_labels,
                     const uint8_t *alive, int n_q, int64_t n, int64_t id_base, int64_t *cand, int64_t ld_cand, int m_cap,
                     int32_t *counts, void *workspace, void *stream) {
    const char *who = "msim_filter_list";
    if (m_cap < 0) return fail(MSIM_EINVAL, "%s: negative size (m_cap=%d)", who, m_cap);
    msim::FilterArgs f;
    int mode = 0;
    bool done = false;
    if (int rc = filter_check(who, n_q, n, bits, ld_words, page_labels, query_labels, alive, &f, &mode, &done)) return rc;
    if (done) return MSIM_OK;
    if (!counts || !workspace || (!cand && m_cap > 0)) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(cand, 8) || misaligned(counts, 4) || misaligned(workspace, 16))
        return fail(MSIM_EINVAL, "%s: cand must be 8-byte, counts 4-byte and workspace 16-byte aligned", who);
    if (ld_cand < m_cap) return fail(MSIM_EINVAL, "%s: ld_cand=%lld < m_cap=%d", who, (long long)ld_cand, m_cap);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int32_t *status = static_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(msim::filter_status_reset_kernel, dim3(1), dim3(1), 0, st, status);
    auto kern = mode == msim::kFilterLabels     ? msim::filter_list_kernel<msim::kFilterLabels>
                : mode == msim::kFilterPerQuery ? msim::filter_list_kernel<msim::kFilterPerQuery>
                                                : msim::filter_list_kernel<msim::kFilterShared>;
    hipLaunchKernelGGL(kern, dim3((unsigned)n_q), dim3(msim::kFilterThreads), 0, st, f, (long long)n, (long long)id_base, cand,
                       (long long)ld_cand, m_cap, counts, status);
    return launch_failed("filter_list_kernel");
}

int msim_filter_ids(int64_t *ids, int64_t ld, int n_q, int64_t m, int64_t n, int64_t id_base, const uint32_t *bits, int64_t ld_words,
                    const int32_t *page_labels, const int32_t *query_labels, const uint8_t *alive, void *stream) {
    const char *who = "msim_filter_ids";
    if (m < 0) return fail(MSIM_EINVAL, "%s: negative size (m=%lld)", who, (long long)m);
    msim::FilterArgs f;
    int mode = 0;
    bool done = false;
    if (int rc = filter_check(who, n_q, n, bits, ld_words, page_labels, query_labels, alive, &f, &mode, &done)) return rc;
    if (done || m == 0) return MSIM_OK;
    if (!ids || misaligned(ids, 8)) return fail(MSIM_EINVAL, "%s: ids must be an 8-byte aligned pointer", who);
    if (ld < m) return fail(MSIM_EINVAL, "%s: ld=%lld < m=%lld", who, (long long)ld, (long long)m);
    const int64_t tiles = (m + msim::kFilterThreads - 1) / msim::kFilterThreads;
    if (tiles > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: %lld columns exceed one launch", who, (long long)m);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned row_groups = (unsigned)(n_q < 65535 ? n_q : 65535);
    auto kern = mode == msim::kFilterLabels     ? msim::filter_ids_kernel<msim::kFilterLabels>
                : mode == msim::kFilterPerQuery ? msim::filter_ids_kernel<msim::kFilterPerQuery>
                                                : msim::filter_ids_kernel<msim::kFilterShared>;
    hipLaunchKernelGGL(kern, dim3((unsigned)tiles, row_groups), dim3(msim::kFilterThreads), 0, st, ids, (long long)ld, n_q, (long long)m,
                       (long long)n, (long long)id_base, f);
    return launch_failed("filter_ids_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- document-level search (group.hip)
extern "C" {

int msim_group_reduce(const float *scores, int64_t ld, int n_q, int64_t n, const int32_t *offsets, const int32_t *pages, int n_groups,
                      int64_t id_base, float *group_scores, int64_t *group_pages, int64_t ld_out, void *stream) {
    const char *who = "msim_group_reduce";
    if (n_q < 0 || n < 0 || n_groups < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d n=%lld n_groups=%d)", who, n_q, (long long)n, n_groups);
    if (n_q == 0 || n_groups == 0) return MSIM_OK;
    if (n > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: n=%lld above 2^31 - 1", who, (long long)n);
    if (!offsets || !group_scores || !group_pages || (n > 0 && (!scores || !pages))) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(scores, 4) || misaligned(offsets, 4) || misaligned(pages, 4) || misaligned(group_scores, 4) || misaligned(group_pages, 8))
        return fail(MSIM_EINVAL, "%s: scores, offsets, pages and group_scores must be 4-byte aligned, group_pages 8-byte aligned", who);
    if (ld < n) return fail(MSIM_EINVAL, "%s: ld=%lld < n=%lld", who, (long long)ld, (long long)n);
    if (ld_out < n_groups) return fail(MSIM_EINVAL, "%s: ld_out=%lld < n_groups=%d", who, (long long)ld_out, n_groups);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long tiles = ((long long)n_groups + msim::kGroupThreads - 1) / msim::kGroupThreads;
    // rows are shared out over grid.y: 64 row groups keep a lane's page registers in use for many rows; where the documents fill
    // few tiles, more row groups (down to one row each) keep ~16 workgroups per CU in the launch
    long long row_groups = (4096 + tiles - 1) / tiles;
    row_groups = row_groups < 64 ? 64 : row_groups;
    row_groups = row_groups > n_q ? n_q : row_groups > 65535 ? 65535 : row_groups;
    hipLaunchKernelGGL(msim::group_reduce_kernel, dim3((unsigned)tiles, (unsigned)row_groups), dim3(msim::kGroupThreads), 0, st, scores,
                       (long long)ld, n_q, (long long)n, offsets, pages, n_groups, (long long)id_base, group_scores, group_pages,
                       (long long)ld_out);
    return launch_failed("group_reduce_kernel");
}

int msim_group_select(const float *scores, const int64_t *gids, const int64_t *pages, int n_q, int m, int64_t ld, int k,
                      float *out_scores, int64_t *out_gids, int64_t *out_pages, void *stream) {
    const char *who = "msim_group_select";
    static std::atomic<int> configured[kMaxDevices];
    if (n_q < 0 || m < 0 || k <= 0) return fail(MSIM_EINVAL, "%s: bad size (n_q=%d m=%d k=%d)", who, n_q, m, k);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (m > msim::kGroupSelectMaxM) return fail(MSIM_EUNSUPPORTED, "%s: m=%d > %d", who, m, msim::kGroupSelectMaxM);
    if (k > msim::kGroupSelectMaxK) return fail(MSIM_EUNSUPPORTED, "%s: k=%d > %d", who, k, msim::kGroupSelectMaxK);
    if (!scores || !gids || !pages || !out_scores || !out_gids || !out_pages) return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(scores, 4) || misaligned(out_scores, 4) || misaligned(gids, 8) || misaligned(pages, 8) || misaligned(out_gids, 8) ||
        misaligned(out_pages, 8))
        return fail(MSIM_EINVAL, "%s: scores must be 4-byte aligned, ids 8-byte aligned", who);
    if (ld < m) return fail(MSIM_EINVAL, "%s: ld=%lld < m=%d", who, (long long)ld, m);
    const DeviceInfo *di = nullptr;
    if (int rc = device_info(&di)) return rc;
    if (int rc = allow_lds(msim::group_select_kernel, msim::kGroupSelectMaxM * msim::kGroupSelectEntryBytes, configured)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    int npow2 = 64;
    while (npow2 < m) npow2 <<= 1;
    hipLaunchKernelGGL(msim::group_select_kernel, dim3((unsigned)n_q), dim3(msim::kGroupThreads),
                       (size_t)npow2 * msim::kGroupSelectEntryBytes, st, scores, gids, pages, m, (long long)ld, k, npow2, out_scores,
                       out_gids, out_pages);
    return launch_failed("group_select_kernel");
}

}  // extern "C"

// ---------------------------------------------------------------- token-to-patch alignment of listed entries (K1a, maxsim_align.hip)
namespace {

template <int DIM>
int align_launch(bool f16, const void *Qt, const int32_t *q_off, const void *D, const int32_t *d_off, const uint8_t *clamp0,
                 const int64_t *cand, float *best_sim, int32_t *best_row, float *sims, const msim::AlignArgs &a, hipStream_t st) {
    auto kern = f16 ? msim::maxsim_align_kernel<DIM, true> : msim::maxsim_align_kernel<DIM, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)((long long)a.n_q * a.m)), dim3(256), 0, st, static_cast<const uint16_t *>(Qt), q_off,
                       static_cast<const uint16_t *>(D), d_off, clamp0, cand, best_sim, best_row, sims, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(MSIM_ELAUNCH, "maxsim_align_kernel<%d> launch: %s", DIM, hipGetErrorString(e));
    return MSIM_OK;
}

}  // namespace

extern "C" {

int msim_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, const void *D,
                          const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim, const int64_t *cand, int m,
                          int64_t ld_cand, int64_t id_base, float *best_sim, int32_t *best_row, float *sims, int max_rows,
                          void *stream) {
    const char *who = "msim_align_candidates";
    if (n_q < 0 || m < 0 || n_d < 0 || q_rows < 0 || d_rows < 0 || max_q_tokens < 0 || max_rows < 0)
        return fail(MSIM_EINVAL, "%s: negative size (n_q=%d m=%d n_d=%d q_rows=%lld d_rows=%lld max_q_tokens=%d max_rows=%d)", who, n_q,
                    m, n_d, (long long)q_rows, (long long)d_rows, max_q_tokens, max_rows);
    if (n_q == 0 || m == 0) return MSIM_OK;
    if (!(dtype == MSIM_DTYPE_BF16 || dtype == MSIM_DTYPE_F16) || !(dim == msim::kDim || dim == kCandWideDim))
        return fail(MSIM_EUNSUPPORTED, "%s takes bfloat16 / float16 embeddings of width %d or %d (dtype code %d, dim %d)", who,
                    msim::kDim, kCandWideDim, dtype, dim);
    if (max_q_tokens > msim::kAlignMaxTokens)
        return fail(MSIM_EUNSUPPORTED, "%s: max_q_tokens=%d: queries of at most %d tokens", who, max_q_tokens, msim::kAlignMaxTokens);
    if ((!Qt && q_rows > 0) || !q_off || (!D && d_rows > 0) || !d_off || !cand || ((!best_sim || !best_row) && max_q_tokens > 0))
        return fail(MSIM_EINVAL, "%s: null pointer argument", who);
    if (misaligned(Qt, 16) || misaligned(D, 16)) return fail(MSIM_EINVAL, "%s: Qt and D must be 16-byte aligned", who);
    if (misaligned(q_off, 4) || misaligned(d_off, 4) || misaligned(cand, 8) || misaligned(best_sim, 4) || misaligned(best_row, 4) ||
        misaligned(sims, 4))
        return fail(MSIM_EINVAL, "%s: offsets and outputs must be 4-byte aligned, cand 8-byte aligned", who);
    if (ld_cand < m) return fail(MSIM_EINVAL, "%s: ld_cand=%lld < m=%d", who, (long long)ld_cand, m);
    if ((long long)n_q * m > 0x7fffffffLL) return fail(MSIM_EUNSUPPORTED, "%s: more than 2^31 - 1 entries (n_q=%d x m=%d)", who, n_q, m);
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
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool f16 = dtype == MSIM_DTYPE_F16;
    if (dim == msim::kDim)
        return align_launch<msim::kDim>(f16, Qt, q_off, D, d_off, d_clamp0, cand, best_sim, best_row, sims, a, st);
    return align_launch<kCandWideDim>(f16, Qt, q_off, D, d_off, d_clamp0, cand, best_sim, best_row, sims, a, st);
}

}  // extern "C"
