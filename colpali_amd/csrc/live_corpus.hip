// A live packed corpus for gfx950 (MI355X): in-place compaction of the row blob after pages were deleted, and the tombstone mask
// over a score matrix (include/maxsim.h: msim_live_*).  No scoring kernel changes: every scorer reads page c through
// off[c] .. off[c + 1], so a deleted slot only has to become an empty page and its rows have to be handed back.
//
// Compaction (msim_live_compact), all launches stream-ordered:
//   live_reset_kernel       zeroes the status word and the counters of the workspace header (a kernel, not a memset node: DESIGN §3.7).
//   live_lens_kernel        one thread per slot: checks off[c] <= off[c + 1] <= rows_bound, keeps a copy of the old offsets, sums the
//                           live lengths of its 1024-slot tile and lowers `first` to the first row of the first dead page that
//                           still owns rows -- no row below `first` changes place.
//   live_scan_kernel        one workgroup: exclusive scan of the tile sums; the total is the new rows_used.
//   live_apply_kernel       one thread per slot: new off[c] = tile base + scan inside the tile (dead slots count 0), written in
//                           place (the old offsets are read from the copy).
//   live_move_kernel<true>  destination rows [chunk, chunk + bounce rows): every row whose source differs goes source -> bounce;
//   live_move_kernel<false> the same rows go bounce -> destination.  A source row is never below its destination, so by the time a
//                           chunk's rows are written every earlier chunk is done and every later chunk's sources are untouched;
//                           inside a chunk the bounce buffer separates the reads from the writes that could land on them.
//                           A workgroup owns a run of consecutive destination rows: two binary searches over the new offsets give
//                           the slots of its first and last row, each row then finds its slot between them (a page boundary or
//                           two), and the rows move as 16-byte pieces, four in flight per lane, read once with non-temporal loads.
//   live_move_codes_kernel the same two launches for an array of 2-byte rows (the centroid codes of a compressed shard,
//                           msim_res_live_compact), one row per lane: a 16-byte piece of it would span eight rows.
//   live_move_bytes_kernel the same for an array of 1-byte rows (the scale bytes of a live FP4 index, msim_f4_live_compact).
// Every row index the device derives is checked against rows_bound before it becomes an address; a broken invariant sets the
// status word and every later kernel of the call returns at once.
//
// Mask (msim_live_mask_scores): live_mask_kernel, one lane per 4 consecutive columns: the 4 mask bytes are read once, and only
// columns of dead slots are written (-inf), 16 bytes at a time where all four are dead and the row is 16-byte aligned.
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kLiveTile = 1024;            // slots per workgroup of the offset kernels
constexpr int kLiveMoveThreads = 256;
constexpr int kLiveMaxBlockRows = 256;     // rows per workgroup of the move kernels, at most (their sources sit in LDS)
constexpr int kLiveBlockBytes = 16384;     // ... and about this many bytes: 4 x 16 B in flight per lane
constexpr int kLiveNoRow = 0x7fffffff;

// workspace header (int32 words)
constexpr int kLiveStatus = 0, kLiveFirst = 1, kLiveTotal = 2, kLiveHeaderWords = 4;
constexpr int kLiveBadOffsets = 1, kLiveBadRow = 2;

typedef __attribute__((ext_vector_type(4))) unsigned int live_u32x4;

// exclusive scan of one value per thread over a 1024-thread workgroup; *total = the workgroup's sum (uniform)
__device__ __forceinline__ long long live_block_scan(long long v, long long *wave_sums, long long *total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long inc = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const long long up = __shfl_up(inc, s);
        if (lane >= s) inc += up;
    }
    __syncthreads();                                   // the previous use of wave_sums is over
    if (lane == 63) wave_sums[wave] = inc;
    __syncthreads();
    long long base = 0, all = 0;
    for (int w = 0; w < kLiveTile / 64; ++w) {
        const long long s = wave_sums[w];
        if (w < wave) base += s;
        all += s;
    }
    *total = all;
    return base + inc - v;
}

__global__ void live_reset_kernel(int32_t *hdr) {
    if (threadIdx.x == 0) {
        hdr[kLiveStatus] = 0;
        hdr[kLiveFirst] = kLiveNoRow;
        hdr[kLiveTotal] = 0;
        hdr[3] = 0;
    }
}

__global__ __launch_bounds__(kLiveTile) void live_lens_kernel(const int32_t *__restrict__ off, const uint8_t *__restrict__ alive,
                                                              int n_slots, long long rows_bound, int32_t *__restrict__ hdr,
                                                              int32_t *__restrict__ old_off, long long *__restrict__ tile_sum) {
    __shared__ long long wave_sums[kLiveTile / 64];
    const long long c = (long long)blockIdx.x * kLiveTile + threadIdx.x;
    long long len = 0;
    if (c < n_slots) {
        const long long a = off[c], b = off[c + 1];
        const bool ok = a >= 0 && b >= a && b <= rows_bound && (c != 0 || a == 0);
        old_off[c] = (int32_t)a;
        if (c == n_slots - 1) old_off[n_slots] = (int32_t)b;
        if (!ok) {
            atomicOr(&hdr[kLiveStatus], kLiveBadOffsets);
        } else if (alive[c]) {
            len = b - a;
        } else if (b > a) {
            atomicMin(&hdr[kLiveFirst], (int32_t)a);
        }
    }
    long long total;
    live_block_scan(len, wave_sums, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ __launch_bounds__(kLiveTile) void live_scan_kernel(int n_tiles, int n_slots, long long rows_bound, int32_t *__restrict__ hdr,
                                                              const int32_t *__restrict__ old_off, const long long *__restrict__ tile_sum,
                                                              long long *__restrict__ tile_base, long long *__restrict__ rows_used_out) {
    __shared__ long long wave_sums[kLiveTile / 64];
    if (hdr[kLiveStatus]) {                              // uniform: nothing has moved, the rows in use are the old ones
        if (threadIdx.x == 0) *rows_used_out = old_off[n_slots];
        return;
    }
    long long carry = 0;
    for (int t0 = 0; t0 < n_tiles; t0 += kLiveTile) {
        const int t = t0 + threadIdx.x;
        const long long v = t < n_tiles ? tile_sum[t] : 0;
        long long total;
        const long long ex = live_block_scan(v, wave_sums, &total);
        if (t < n_tiles) tile_base[t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        if (carry > rows_bound || carry > 0x7fffffffLL) {
            atomicOr(&hdr[kLiveStatus], kLiveBadOffsets);
            *rows_used_out = old_off[n_slots];
        } else {
            hdr[kLiveTotal] = (int32_t)carry;
            *rows_used_out = carry;
        }
    }
}

__global__ __launch_bounds__(kLiveTile) void live_apply_kernel(int32_t *__restrict__ off, const uint8_t *__restrict__ alive, int n_slots,
                                                               const int32_t *__restrict__ hdr, const int32_t *__restrict__ old_off,
                                                               const long long *__restrict__ tile_base) {
    __shared__ long long wave_sums[kLiveTile / 64];
    if (hdr[kLiveStatus]) return;                        // uniform
    const long long c = (long long)blockIdx.x * kLiveTile + threadIdx.x;
    long long len = 0;
    if (c < n_slots && alive[c]) len = (long long)old_off[c + 1] - old_off[c];
    long long total;
    const long long at = tile_base[blockIdx.x] + live_block_scan(len, wave_sums, &total);
    if (c < n_slots) {
        off[c] = (int32_t)at;
        if (c == n_slots - 1) off[n_slots] = (int32_t)(at + len);
    }
}

// the slot that owns destination row d: the largest c in [lo, hi) with new_off[c] <= d, given new_off[lo] <= d < new_off[hi]
__device__ __forceinline__ int live_slot_of(const int32_t *__restrict__ new_off, int lo, int hi, int d) {
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (new_off[mid] <= d) lo = mid; else hi = mid;
    }
    return lo;
}

// TO_BOUNCE: rows -> bounce (sources), else bounce -> rows (destinations); destination rows chunk0 .. chunk0 + chunk_rows - 1
template <bool TO_BOUNCE>
__global__ __launch_bounds__(kLiveMoveThreads) void live_move_kernel(uint8_t *__restrict__ rows, int lpr /* 16-byte pieces per row */,
                                                                     long long rows_bound, const int32_t *__restrict__ new_off,
                                                                     const int32_t *__restrict__ old_off, int n_slots,
                                                                     int32_t *__restrict__ hdr, uint8_t *__restrict__ bounce,
                                                                     long long chunk0, int chunk_rows, int block_rows) {
    __shared__ int src_row[kLiveMaxBlockRows];
    if (hdr[kLiveStatus]) return;                        // uniform
    const long long total = hdr[kLiveTotal], first = hdr[kLiveFirst];
    const long long r0 = chunk0 + (long long)blockIdx.x * block_rows;
    long long r1 = r0 + block_rows;
    if (r1 > chunk0 + chunk_rows) r1 = chunk0 + chunk_rows;
    if (r1 > total) r1 = total;
    if (r0 >= r1 || r1 <= first) return;                 // past the live rows, or wholly below the first row that moves
    const int nrows = (int)(r1 - r0);
    const int s_lo = live_slot_of(new_off, 0, n_slots, (int)r0);
    const int s_hi = live_slot_of(new_off, s_lo, n_slots, (int)(r1 - 1));
    for (int t = threadIdx.x; t < nrows; t += kLiveMoveThreads) {
        const long long d = r0 + t;
        const int c = live_slot_of(new_off, s_lo, s_hi + 1, (int)d);
        const long long src = (long long)old_off[c] + (d - new_off[c]);
        int s = -1;                                      // -1: stays where it is
        if (src < d || src >= rows_bound || d >= rows_bound) atomicOr(&hdr[kLiveStatus], kLiveBadRow);
        else if (src != d) s = (int)src;
        src_row[t] = s;
    }
    __syncthreads();
    const long long row_bytes = (long long)lpr * 16;
    const int pieces = nrows * lpr;
    uint8_t *bounce_base = bounce + (r0 - chunk0) * row_bytes;
    for (int i0 = threadIdx.x; i0 < pieces; i0 += 4 * kLiveMoveThreads) {
        live_u32x4 v[4];
        long long dst[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kLiveMoveThreads;
            dst[u] = -1;
            if (i < pieces) {
                const int r = i / lpr, p = i - r * lpr;
                const int s = src_row[r];
                if (s >= 0) {
                    const long long in_bounce = (long long)r * row_bytes + p * 16;
                    if (TO_BOUNCE) {
                        v[u] = __builtin_nontemporal_load(reinterpret_cast<const live_u32x4 *>(rows + (long long)s * row_bytes + p * 16));
                        dst[u] = in_bounce;
                    } else {
                        v[u] = *reinterpret_cast<const live_u32x4 *>(bounce_base + in_bounce);
                        dst[u] = (r0 + r) * row_bytes + p * 16;
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (dst[u] >= 0) {
                if (TO_BOUNCE) *reinterpret_cast<live_u32x4 *>(bounce_base + dst[u]) = v[u];
                else *reinterpret_cast<live_u32x4 *>(rows + dst[u]) = v[u];
            }
        }
    }
}

// The same move for an array of 2-byte rows (the uint16 centroid codes of a compressed shard, msim_res_live_compact): a 16-byte
// piece of such an array spans eight rows, page boundaries and alignments, so this one works per row -- one lane per destination
// row, kLiveCodeRows rows per lane; consecutive lanes read and write consecutive 2-byte elements inside a page.
constexpr int kLiveCodeRows = 4;            // destination rows per lane: 1024 per workgroup

template <bool TO_BOUNCE>
__global__ __launch_bounds__(kLiveMoveThreads) void live_move_codes_kernel(uint16_t *__restrict__ codes, long long rows_bound,
                                                                           const int32_t *__restrict__ new_off,
                                                                           const int32_t *__restrict__ old_off, int n_slots,
                                                                           int32_t *__restrict__ hdr, uint16_t *__restrict__ bounce,
                                                                           long long chunk0, int chunk_rows) {
    if (hdr[kLiveStatus]) return;                        // uniform
    constexpr int block_rows = kLiveMoveThreads * kLiveCodeRows;
    const long long total = hdr[kLiveTotal], first = hdr[kLiveFirst];
    const long long r0 = chunk0 + (long long)blockIdx.x * block_rows;
    long long r1 = r0 + block_rows;
    if (r1 > chunk0 + chunk_rows) r1 = chunk0 + chunk_rows;
    if (r1 > total) r1 = total;
    if (r0 >= r1 || r1 <= first) return;                 // past the live rows, or wholly below the first row that moves
    const int s_lo = live_slot_of(new_off, 0, n_slots, (int)r0);
    const int s_hi = live_slot_of(new_off, s_lo, n_slots, (int)(r1 - 1));
#pragma unroll
    for (int u = 0; u < kLiveCodeRows; ++u) {
        const long long d = r0 + u * kLiveMoveThreads + threadIdx.x;
        if (d >= r1) continue;
        const int c = live_slot_of(new_off, s_lo, s_hi + 1, (int)d);
        const long long src = (long long)old_off[c] + (d - new_off[c]);
        if (src < d || src >= rows_bound || d >= rows_bound) atomicOr(&hdr[kLiveStatus], kLiveBadRow);
        else if (src != d) {
            if (TO_BOUNCE) bounce[d - chunk0] = codes[src];
            else codes[d] = bounce[d - chunk0];
        }
    }
}

// ... and for an array of 1-byte rows (the E8M0 scale bytes of a live FP4 index, msim_f4_live_compact): the same shape, the same
// early exits and status word; consecutive lanes read and write consecutive bytes inside a page.
template <bool TO_BOUNCE>
__global__ __launch_bounds__(kLiveMoveThreads) void live_move_bytes_kernel(uint8_t *__restrict__ bytes, long long rows_bound,
                                                                           const int32_t *__restrict__ new_off,
                                                                           const int32_t *__restrict__ old_off, int n_slots,
                                                                           int32_t *__restrict__ hdr, uint8_t *__restrict__ bounce,
                                                                           long long chunk0, int chunk_rows) {
    if (hdr[kLiveStatus]) return;                        // uniform
    constexpr int block_rows = kLiveMoveThreads * kLiveCodeRows;
    const long long total = hdr[kLiveTotal], first = hdr[kLiveFirst];
    const long long r0 = chunk0 + (long long)blockIdx.x * block_rows;
    long long r1 = r0 + block_rows;
    if (r1 > chunk0 + chunk_rows) r1 = chunk0 + chunk_rows;
    if (r1 > total) r1 = total;
    if (r0 >= r1 || r1 <= first) return;                 // past the live rows, or wholly below the first row that moves
    const int s_lo = live_slot_of(new_off, 0, n_slots, (int)r0);
    const int s_hi = live_slot_of(new_off, s_lo, n_slots, (int)(r1 - 1));
#pragma unroll
    for (int u = 0; u < kLiveCodeRows; ++u) {
        const long long d = r0 + u * kLiveMoveThreads + threadIdx.x;
        if (d >= r1) continue;
        const int c = live_slot_of(new_off, s_lo, s_hi + 1, (int)d);
        const long long src = (long long)old_off[c] + (d - new_off[c]);
        if (src < d || src >= rows_bound || d >= rows_bound) atomicOr(&hdr[kLiveStatus], kLiveBadRow);
        else if (src != d) {
            if (TO_BOUNCE) bounce[d - chunk0] = bytes[src];
            else bytes[d] = bounce[d - chunk0];
        }
    }
}

// grid: (column tiles of 1024, row groups); scores fp32 [n_q, ld], columns 0 .. n - 1
__global__ __launch_bounds__(256) void live_mask_kernel(float *__restrict__ scores, long long ld, int n_q, long long n,
                                                        const uint8_t *__restrict__ alive, int vec_ok) {
    const long long c0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c0 >= n) return;
    bool dead[4];
    int n_dead = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        dead[u] = c0 + u < n && alive[c0 + u] == 0;
        n_dead += dead[u];
    }
    if (!n_dead) return;
    const float ninf = -__builtin_inff();
    for (int q = blockIdx.y; q < n_q; q += gridDim.y) {
        float *p = scores + (long long)q * ld + c0;
        if (n_dead == 4 && vec_ok) {
            *reinterpret_cast<f32x4 *>(p) = f32x4{ninf, ninf, ninf, ninf};
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (dead[u]) p[u] = ninf;
        }
    }
}

}  // namespace msim
