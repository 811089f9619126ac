// K1c -- candidate reranking for gfx950 (MI355X): MaxSim of listed (query, document) entries over the resident corpus.
//
// Reference arithmetic (the same per entry as K1s / K1b, no [b,c,n,s] tensor):
//   colpali_engine/utils/processing_utils.py:179
//       einsum("bnd,csd->bcns", Q, D).max(dim=3)[0].sum(dim=2)
// restricted to the documents each query lists -- the exact second stage behind a cheap first one (pooled pages, BM25, a
// bi-encoder, a metadata filter, hard-negative mining).
//
// The candidate matrix cand [n_q, m] (global ids) is inverted on the device into per-document WORK ITEMS, so that a document is
// read once per group of queries that listed it instead of once per entry:
//   1. cand_count_kernel     one thread per entry: empty / out-of-range ids and 0-token queries are written at once; every other
//                            entry takes a rank in its (document, class) bucket by an integer atomic.  class c = the query's
//                            16-token units (1..8).
//   2. cand_block_sums_kernel / cand_scan_sums_kernel / cand_block_starts_kernel
//                            exclusive scans over the documents of (entries, work items), where a document's work items are
//                            sum_c ceil(count[d][c] / per(c)), per(c) = 8 / c entries of class c per item (<= 8 units: K1s's
//                            register budget).  The item count depends on the counts only, never on the order the atomics ran in.
//   3. cand_place_kernel     one thread per entry: its (query, column) into the CSR entry list, and the item header if it opens
//                            an item.
//   4. maxsim_candidates_kernel   a persistent grid; every wave pulls items (grid-stride over the device-built count).
// The grouping is free to vary from run to run: an entry's score is a function of its query and its document alone.
// Every index the device derives (a query's class, a list position, an item header) is checked before it becomes an address.  A
// broken invariant -- a library bug, or a device q_off that disagrees with the host copy the call validated -- sets a bit of the
// status word, and cand_poison_kernel then writes NaN over every score of the call: no score is ever left unwritten or taken from
// the wrong query.
//
// The scorer of one item is K1s's (maxsim_stream.hip): the document streams in 32-row slabs through a wave-private 2-slab LDS ring by
// LDS-DMA (XOR swizzle on the source address, pieces of the next slab issued between the MFMAs of the current one), the swapped
// 16x16x32 product against the item's query units held in registers, the per-token max table in LDS, and the token sum of
// maxsim_common.hpp (reduce_query_tokens: an order that depends on the query's length only).  Each query of an item starts on
// its own unit boundary; its tokens past the end are zero rows whose maxima the sum never reads.  So every score carries the bits
// msim_fwd_ragged gives the same query and document.
#pragma once
#include <type_traits>

#include "maxsim_common.hpp"
#include "maxsim_stream.hip"

namespace msim {

constexpr int kCandClasses = kStreamMaxUnits;     // a query of c units (1..8) is class c
constexpr int kCandScanDocs = 1024;               // documents per block of the scans (256 threads x 4)
constexpr int kCandRing = 2;                      // slabs in a wave's ring: two 4-wave workgroups share a CU (72 KiB each)
constexpr int kCandBadQuery = 1, kCandBadPlace = 2, kCandBadItem = 4;   // bits of the status word

struct CandItem {                                 // one work item: entries e0 .. e0+n-1 of the list, all of class nu, one document
    int doc, e0, n, nu;
};

__device__ __forceinline__ int cand_per(int c) { return kStreamMaxUnits / c; }

__device__ __forceinline__ void cand_doc_totals(const int32_t *__restrict__ cnt, int d, int &ent, int &items) {
    const i32x4 a = *reinterpret_cast<const i32x4 *>(cnt + (size_t)d * kCandClasses);
    const i32x4 b = *reinterpret_cast<const i32x4 *>(cnt + (size_t)d * kCandClasses + 4);
    ent = a[0] + a[1] + a[2] + a[3] + b[0] + b[1] + b[2] + b[3];
    // per(c) = 8, 4, 2, 2, 1, 1, 1, 1
    items = ((a[0] + 7) >> 3) + ((a[1] + 3) >> 2) + ((a[2] + 1) >> 1) + ((a[3] + 1) >> 1) + b[0] + b[1] + b[2] + b[3];
}

// 0. the status word and the counters start at zero.  A kernel, not hipMemsetAsync: in a captured hipGraph, a memset node of this
// HIP build wrote the right zeros on the first replay and the same wrong values on every later one (the replays then saw
// counters of ~30 000 per document); kernel nodes replay like any launch.
__global__ __launch_bounds__(256) void cand_zero_kernel(i32x4 *__restrict__ p, long long n16) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) p[i] = i32x4{0, 0, 0, 0};
}

// 1. ranks, and the entries that need no document
__global__ __launch_bounds__(256) void cand_count_kernel(const int64_t *__restrict__ cand, long long ld_cand, int n_q, int m,
                                                         long long id_base, int n_d, const int32_t *__restrict__ q_off,
                                                         int32_t *__restrict__ cnt, int32_t *__restrict__ rank,
                                                         float *__restrict__ scores, long long ld, int64_t *__restrict__ out_ids,
                                                         int32_t *__restrict__ status) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_q * m) return;
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    const int64_t id = cand[(size_t)q * ld_cand + j];
    const long long d = (long long)id - id_base;
    const bool valid = id >= 0 && d >= 0 && d < n_d;
    if (out_ids) out_ids[(size_t)q * ld + j] = valid ? id : -1;
    int r = -1;
    if (!valid) {
        scores[(size_t)q * ld + j] = -INFINITY;
    } else {
        const int len = q_off[q + 1] - q_off[q];
        if (len == 0) scores[(size_t)q * ld + j] = 0.0f;     // a sum over no tokens: what every scorer returns for it
        else if (len < 0 || len > kStreamMaxUnits * kUnitTok) atomicOr(status, kCandBadQuery);
        else r = atomicAdd(cnt + d * kCandClasses + ((len + kUnitTok - 1) / kUnitTok - 1), 1);
    }
    rank[e] = r;
}

// 256-thread exclusive scan of (a, b) pairs through LDS; returns the block totals
__device__ __forceinline__ void cand_block_scan(int &a, int &b, int &tot_a, int &tot_b) {
    __shared__ int sa[256], sb[256];
    const int t = threadIdx.x;
    sa[t] = a;
    sb[t] = b;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int xa = t >= o ? sa[t - o] : 0, xb = t >= o ? sb[t - o] : 0;
        __syncthreads();
        sa[t] += xa;
        sb[t] += xb;
        __syncthreads();
    }
    tot_a = sa[255];
    tot_b = sb[255];
    a = sa[t] - a;
    b = sb[t] - b;
    __syncthreads();
}

// 2a. (entries, items) of every block of kCandScanDocs documents
__global__ __launch_bounds__(256) void cand_block_sums_kernel(const int32_t *__restrict__ cnt, int n_d, int32_t *__restrict__ bsum) {
    int ea = 0, ia = 0;
    const int d0 = blockIdx.x * kCandScanDocs + threadIdx.x * 4;
    for (int k = 0; k < 4; ++k)
        if (d0 + k < n_d) {
            int e, i;
            cand_doc_totals(cnt, d0 + k, e, i);
            ea += e;
            ia += i;
        }
    int te, ti;
    cand_block_scan(ea, ia, te, ti);
    if (threadIdx.x == 0) {
        bsum[2 * blockIdx.x] = te;
        bsum[2 * blockIdx.x + 1] = ti;
    }
}

// 2b. exclusive scan of the block sums in place (one workgroup); bsum[2 nb], bsum[2 nb + 1] = the totals
__global__ __launch_bounds__(256) void cand_scan_sums_kernel(int32_t *__restrict__ bsum, int nb) {
    int base_e = 0, base_i = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        int e = b < nb ? bsum[2 * b] : 0, i = b < nb ? bsum[2 * b + 1] : 0;
        int te, ti;
        cand_block_scan(e, i, te, ti);
        if (b < nb) {
            bsum[2 * b] = base_e + e;
            bsum[2 * b + 1] = base_i + i;
        }
        base_e += te;
        base_i += ti;
    }
    if (threadIdx.x == 0) {
        bsum[2 * nb] = base_e;
        bsum[2 * nb + 1] = base_i;
    }
}

// 2c. first entry and first item of every document; estart[n_d], istart[n_d] = the totals
__global__ __launch_bounds__(256) void cand_block_starts_kernel(const int32_t *__restrict__ cnt, int n_d, const int32_t *__restrict__ bsum,
                                                                int nb, int32_t *__restrict__ estart, int32_t *__restrict__ istart) {
    int e4[4], i4[4];
    int ea = 0, ia = 0;
    const int d0 = blockIdx.x * kCandScanDocs + threadIdx.x * 4;
    for (int k = 0; k < 4; ++k) {
        e4[k] = i4[k] = 0;
        if (d0 + k < n_d) cand_doc_totals(cnt, d0 + k, e4[k], i4[k]);
        ea += e4[k];
        ia += i4[k];
    }
    int te, ti;
    cand_block_scan(ea, ia, te, ti);
    ea += bsum[2 * blockIdx.x];
    ia += bsum[2 * blockIdx.x + 1];
    for (int k = 0; k < 4; ++k)
        if (d0 + k < n_d) {
            estart[d0 + k] = ea;
            istart[d0 + k] = ia;
            ea += e4[k];
            ia += i4[k];
        }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        estart[n_d] = bsum[2 * nb];
        istart[n_d] = bsum[2 * nb + 1];
    }
}

// 3. the entry list (CSR by document, then class) and the item headers
__global__ __launch_bounds__(256) void cand_place_kernel(const int64_t *__restrict__ cand, long long ld_cand, int n_q, int m,
                                                         long long id_base, const int32_t *__restrict__ q_off,
                                                         const int32_t *__restrict__ cnt, const int32_t *__restrict__ rank,
                                                         const int32_t *__restrict__ estart, const int32_t *__restrict__ istart,
                                                         int n_d, int2 *__restrict__ entries, CandItem *__restrict__ items,
                                                         int32_t *__restrict__ status) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long E = (long long)n_q * m;
    if (e >= E) return;
    const int r = rank[e];
    if (r < 0) return;
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    const long long d = (long long)cand[(size_t)q * ld_cand + j] - id_base;
    const int c = (q_off[q + 1] - q_off[q] + kUnitTok - 1) / kUnitTok;
    if (d < 0 || d >= n_d || c < 1 || c > kCandClasses) {             // the count pass saw another id / length here
        atomicOr(status, kCandBadPlace);
        return;
    }
    const int32_t *cd = cnt + (size_t)d * kCandClasses;
    long long eb = estart[d], ib = istart[d];
    for (int k = 1; k < c; ++k) {
        eb += cd[k - 1];
        ib += (cd[k - 1] + cand_per(k) - 1) / cand_per(k);
    }
    const int per = cand_per(c);
    const int left = cd[c - 1] - r;
    if (left < 1 || eb < 0 || eb + r >= E || ib < 0 || ib + r / per >= E) {
        atomicOr(status, kCandBadPlace);
        return;
    }
    entries[eb + r] = make_int2(q, j);
    if (r % per == 0) items[ib + r / per] = CandItem{(int)d, (int)(eb + r), left < per ? left : per, c};
}

// 4. the scorer: one wave = one item at a time (grid-stride over the item count the scans left on the device)
template <int NU, bool F16, int AUX>
__device__ __forceinline__ void cand_item(const uint16_t *__restrict__ Qt, const int32_t *__restrict__ q_off, const uint16_t *__restrict__ D,
                                          const int32_t *__restrict__ d_off, const uint8_t *__restrict__ clamp0,
                                          const int2 *__restrict__ entries, const CandItem &h, int n_q, int m, float *__restrict__ scores,
                                          long long ld, bool ref_bf16, bool &bad, char *ring, char *tokmax, const int (&src_off)[4], const int (&rd_off)[2][kKSteps16],
                                          int lane) {
    constexpr int RING = kCandRing;
    const int r0 = d_off[h.doc];
    const int len = d_off[h.doc + 1] - r0;
    const int n_slabs = (len + kSlabRows - 1) / kSlabRows;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(D + (size_t)r0 * kDim), 0, len * kRowBytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t null_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)D, 0, 0, 0x00020000);

    // every request is 8 loads, real or through an empty descriptor: the number of loads in flight is a constant (as in K1s)
    int p = 0, p_slot = 0;
    auto request_piece = [&](int slab, int slot, int i) {
        const bool live = slab < n_slabs;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(live ? rsrc : null_rsrc, MSIM_LDS(ring + slot * kSlabBytes + i * 1024), 16, src_off[i & 3],
                                                 (live ? slab * kSlabBytes : 0) + i * 1024, 0, AUX);
    };
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) {
#pragma unroll
        for (int i = 0; i < 8; ++i) request_piece(p, p_slot, i);
        ++p;
        p_slot = p_slot + 1 == RING ? 0 : p_slot + 1;
    }

    // the item's query units, behind the first slab's DMA: unit u = unit (u mod nu) of entry u / nu
    QueryUnit qu[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const int ei = u / h.nu;
        int q = __builtin_amdgcn_readfirstlane(entries[h.e0 + ei].x);
        if (q < 0 || q >= n_q) {                         // never trust a device-built index with an address: reported, the call's
            bad = true;                                  // scores become NaN
            q = 0;
        }
        const int qs = q_off[q], qe = q_off[q + 1];
        load_query_unit(qu[u], Qt, qs + (u - ei * h.nu) * kUnitTok, qe, lane, true);
    }
    wait_vmcnt<0>();
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int ks = 0; ks < kKSteps16; ++ks) asm volatile("" : "+v"(qu[u].f[ks]));

    float mx[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) mx[u] = -INFINITY;
    int c_slot = 0;
    auto slab = [&](auto tail_c, int rows_left) {
        constexpr bool kTail = decltype(tail_c)::value;
        wait_vmcnt<8 * (RING - 2)>();     // RING - 1 requests are outstanding: all but the oldest may stay in flight
        const int nx = p, nx_slot = p_slot;
        const char *src = ring + c_slot * kSlabBytes;
        c_slot = c_slot + 1 == RING ? 0 : c_slot + 1;
        bf16x8 af[2][kKSteps16];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int ks = 0; ks < kKSteps16; ++ks) af[g][ks] = *reinterpret_cast<const bf16x8 *>(src + rd_off[g][ks]);
        slab_units<F16, NU, kTail, true>(mx, af, qu, rows_left, lane, [&](int mf) {
            if (mf % NU == 0) request_piece(nx, nx_slot, mf / NU);      // one DMA piece per NU MFMAs: 8 per slab
        });
        ++p;
        p_slot = p_slot + 1 == RING ? 0 : p_slot + 1;
    };
    const int n_full = len / kSlabRows, rem = len - n_full * kSlabRows;
    for (int s = 0; s < n_full; ++s) slab(std::false_type{}, kSlabRows);
    if (rem > 0) slab(std::true_type{}, rem);
    wait_vmcnt<0>();                      // the empty requests behind the document: the ring is free for the next item

    bool clamp = false;
    if (clamp0 != nullptr) {
        const uint64_t addr = reinterpret_cast<uint64_t>(clamp0) + (uint64_t)h.doc;
        clamp = ((scalar_load_u32(addr & ~3ull) >> ((addr & 3) * 8)) & 0xffu) != 0;
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) store_token_max(tokmax, u, mx[u], lane);
    const int rq = lane >> 3, ri = lane & 7;
    const int2 ent = rq < h.n ? entries[h.e0 + rq] : make_int2(0, 0);
    if (rq < h.n && (ent.x < 0 || ent.x >= n_q || ent.y < 0 || ent.y >= m)) bad = true;
    else if (rq < h.n) {
        const int s = rq * h.nu * kUnitTok;
        float tot = reduce_query_tokens<F16>(tokmax, s, s + (q_off[ent.x + 1] - q_off[ent.x]), ri, clamp, ref_bf16);
        if (ref_bf16) tot = round_to_input<F16>(tot);
        if (ri == 0) scores[(size_t)ent.x * ld + ent.y] = tot;
    }
}

constexpr int kCandLdsBytes = 4 * (kCandRing * kSlabBytes + kStreamTokBytes);

template <bool F16, int AUX>
__global__ __launch_bounds__(256, 2) void maxsim_candidates_kernel(const uint16_t *__restrict__ Qt,      // [T, 128] flat query tokens
                                                                const int32_t *__restrict__ q_off,   // [n_q + 1]
                                                                const uint16_t *__restrict__ D,      // [rows, 128]
                                                                const int32_t *__restrict__ d_off,   // [n_d + 1]
                                                                const uint8_t *__restrict__ clamp0,  // [n_d] or null
                                                                const int2 *__restrict__ entries,    // (query, column) by item
                                                                const CandItem *__restrict__ items,
                                                                const int32_t *__restrict__ n_items_p, int n_entries, int n_q, int m,
                                                                int n_d, float *__restrict__ scores, long long ld, unsigned flags,
                                                                int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char *ring = smem + wave * (kCandRing * kSlabBytes);
    char *tokmax = smem + 4 * (kCandRing * kSlabBytes) + wave * kStreamTokBytes;
    const int gw = blockIdx.x * 4 + wave;
    const int GW = gridDim.x * 4;
    const bool ref_bf16 = (flags & kFlagRefBf16) != 0;

    const int l16 = lane & 15, l4 = lane >> 4;
    int src_off[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) src_off[j] = l4 * kRowBytes + (((l16 ^ l4) ^ (j << 2)) << 4);
    int rd_off[2][kKSteps16];
    slab_rd_offsets16(lane, rd_off);

    // the item list is data of the preceding kernels: every header is checked before it becomes an address (at most one item per entry)
    int n_items = __builtin_amdgcn_readfirstlane(*n_items_p);
    bool bad = n_items < 0 || n_items > n_entries;
    n_items = bad ? 0 : n_items;
    for (int it = gw; it < n_items; it += GW) {
        const CandItem *hp = items + it;
        CandItem h;
        h.doc = __builtin_amdgcn_readfirstlane(hp->doc);
        h.e0 = __builtin_amdgcn_readfirstlane(hp->e0);
        h.n = __builtin_amdgcn_readfirstlane(hp->n);
        h.nu = __builtin_amdgcn_readfirstlane(hp->nu);
        if (h.doc < 0 || h.doc >= n_d || h.nu < 1 || h.nu > kStreamMaxUnits || h.n < 1 || h.n * h.nu > kStreamMaxUnits || h.e0 < 0 ||
            h.e0 > n_entries - h.n) {
            bad = true;
            continue;
        }
        switch (h.n * h.nu) {
#define MSIM_CAND_CASE(U) \
            case U: cand_item<U, F16, AUX>(Qt, q_off, D, d_off, clamp0, entries, h, n_q, m, scores, ld, ref_bf16, bad, ring, tokmax, src_off, rd_off, lane); break;
            MSIM_CAND_CASE(1)
            MSIM_CAND_CASE(2)
            MSIM_CAND_CASE(3)
            MSIM_CAND_CASE(4)
            MSIM_CAND_CASE(5)
            MSIM_CAND_CASE(6)
            MSIM_CAND_CASE(7)
            MSIM_CAND_CASE(8)
#undef MSIM_CAND_CASE
            default: break;
        }
    }
    if (bad && lane == 0) atomicOr(status, kCandBadItem);
}

// 5. a broken invariant anywhere above: every score of the call becomes NaN (never a silently wrong or unwritten one)
__global__ __launch_bounds__(256) void cand_poison_kernel(const int32_t *__restrict__ status, int n_q, int m, float *__restrict__ scores,
                                                          long long ld) {
    if (*status == 0) return;
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n_q * m) return;
    const int q = (int)(e / m), j = (int)(e - (long long)q * m);
    scores[(size_t)q * ld + j] = __builtin_nanf("");
}

}  // namespace msim
