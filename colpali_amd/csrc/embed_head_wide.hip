// K3w -- embedding head at width 320 (ColQwen3) for gfx950: the 320-wide sibling of embed_head.hip, a kernel of its own.
//
// Reference lines replaced (the tail every Col* family shares; ColQwen3 has self.dim = 320):
//       proj = self.custom_text_proj(hidden_states)              # nn.Linear(hidden, 320)
//       proj = proj / proj.norm(dim=-1, keepdim=True)            # L2 normalisation
//       proj = proj * attention_mask.unsqueeze(-1)               # padded positions -> exactly 0
// and the host steps behind them on the way to the scorer: the rows go through the same int32 row map as msim_embed_head,
// straight into a dense [B * S, 320] tensor or a packed 320-wide corpus blob.
//
// Rounding chain reproduced in the model dtype (bf16 / fp16), one rounding where torch has one:
//   y = round(acc_fp32 + bias)          nn.Linear output tensor
//   n = round(sqrt(sum_fp32(y^2)))      Tensor.norm (fp32 accumulation inside, result in the tensor dtype)
//   o = round(y / n) * mask             true division, then an exact multiply by 0 or 1
//
// Shape of the work: M = all token rows, N = 320, K = hidden size H (a multiple of 64, <= 4096).  320 FLOP per byte of hidden
// state against a ridge of ~312: the kernel sits AT the ridge, so both the matrix pipe and the hidden-state stream matter.
//
// Structure (persistent, one workgroup of 4 waves per CU, one wave per SIMD, no loader wave):
//   * row tile = 128 rows (divides the row map's 256-entry padding), K chunk = 64 elements = 128-byte LDS rows;
//   * wave w owns rows 32w .. 32w+31 of the tile and the whole 320 columns: ten 32x32 fp32 accumulator tiles = 160 VGPRs
//     (the Makefile keeps MFMA accumulators in VGPRs; one wave per SIMD has 512 registers to itself);
//   * MFMA operand roles are SWAPPED (A = weight rows = output columns, B = hidden rows): a lane ends a tile holding 160 of the
//     320 columns of ONE hidden row -- columns 32j + 8g + 4*half + 0..3 in registers 4g .. 4g+3 of tile j.  The row norm is an
//     in-lane sum of 160 squares plus ONE exchange between the two halves of the wave, the row map is read once per lane
//     (through the scalar cache), and a lane stores 40 x 8 bytes.  (One output column per lane, the other form, would need ten
//     5-step butterflies per 16 rows.)
//   * hidden-state ring: 3 chunks of [128][64] = 16 KiB each; a wave fills and reads only its own 32 rows (4 LDS-DMA
//     instructions per chunk), two chunks ahead, so this stream needs no barrier at all;
//   * weight ring: 2 chunks of [320][64] = 40 KiB each, from the XCD's L2; every wave fetches a quarter of a chunk (10 LDS-DMA
//     instructions), one chunk ahead; ONE raw s_barrier per chunk hands the slot over (behind a counted vmcnt);
//   * the bias sits in LDS as 320 floats (staged once per workgroup): 48 + 80 + 1.25 KiB = 129.25 KiB of LDS;
//   * LDS image of a chunk: 128-byte rows, the 16-byte piece index XOR-ed with (row >> 1) & 7 on the SOURCE address and on the
//     ds_read_b128, the LDS-DMA destination staying linear (swizzle on both sides or on neither): conflict free;
//   * the rings run on across row tiles: the flat sequence (tile, chunk) of a workgroup is prefetched without a bubble at a
//     tile boundary; the epilogue's stores sit between two chunks;
//   * inside a chunk the operand fetch runs one group of five MFMAs ahead of the matrix pipe, and the 14 LDS-DMA pieces of the
//     chunks being prefetched are issued two at a time behind the groups (both measured, see the loop).
// Measured and not kept (1000 x 779 x 2048 bf16, this kernel 1.16 ms): waves of 64 rows x 160 columns (36 % less LDS read
// traffic, the row norm exchanged between two waves through LDS: 1.32 ms against 1.26 ms for the form it was tried on), and two
// waves fetching the hidden states into a 4-deep ring while the other two fetch the weights (1.40 ms against 1.26 ms) -- both
// make the hidden-state slots shared, so that stream waits at the barrier too.
// One fp32 accumulator takes at most 4096 / 16 = 256 MFMA results in K order, the range in which the 128-wide kernel stays in
// the reference's rounding tier without folding (the ABI refuses larger hidden sizes).
#pragma once
#include "maxsim_common.hpp"

namespace msim {

constexpr int kHwN = 320;                            // output width
constexpr int kHwTilesN = kHwN / 32;                 // 10 accumulator tiles per wave
constexpr int kHwWaves = 4;
constexpr int kHwBM = kHwWaves * 32;                 // 128 rows per tile
constexpr int kHwBK = 64;                            // K elements per chunk (128 B per row)
constexpr int kHwThreads = kHwWaves * 64;
constexpr int kHwABytes = kHwBM * kHwBK * 2;         // 16 KiB
constexpr int kHwWBytes = kHwN * kHwBK * 2;          // 40 KiB
constexpr int kHwRingA = 3;                          // hidden-state chunks (two in flight)
constexpr int kHwRingW = 2;                          // weight chunks (one in flight)
constexpr int kHwWBase = kHwRingA * kHwABytes;                    // 48 KiB
constexpr int kHwBiasBase = kHwWBase + kHwRingW * kHwWBytes;      // 128 KiB
constexpr int kHwLds = kHwBiasBase + kHwN * 4;                    // + 320 floats
constexpr int kHwMaxH = 4096;
static_assert(kHwLds <= 160 * 1024, "embed_head_wide_kernel: rings + bias must fit the CU's LDS");
static_assert(256 % kHwBM == 0, "the row tile must divide the row map's 256-entry padding");
static_assert(kHwWBytes % (kHwWaves * 1024) == 0, "every wave fetches the same number of 1 KiB weight pieces");

struct HeadWideArgs {
    long long M;          // token rows
    int H;                // hidden size (multiple of 64, <= 4096)
    long long ld_out;     // elements between consecutive output rows (>= 320, multiple of 8)
};

template <int N>
__device__ __forceinline__ void hw_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// row_map[m] (int32, ceil(M / 256) * 256 entries):  v >= 0: write the normalised row to out row v;
//   v == -1: drop the row;  v <= -2: write a row of zeros to out row (-2 - v)   (a masked position kept in place).
template <bool F16>
__global__ __launch_bounds__(kHwThreads) void embed_head_wide_kernel(const uint16_t *__restrict__ X,     // [M, H]
                                                                  const uint16_t *__restrict__ W,     // [320, H]
                                                                  const uint16_t *__restrict__ bias,  // [320] or null
                                                                  const int32_t *__restrict__ row_map,
                                                                  uint16_t *__restrict__ out, HeadWideArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, half = lane >> 5;
    const int n_tiles = (int)((a.M + kHwBM - 1) / kHwBM);
    const int n_chunks = a.H / kHwBK;
    const int row_bytes = a.H * 2;
    const int my_tiles = (int)blockIdx.x < n_tiles ? (n_tiles - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int total = my_tiles * n_chunks;                                   // chunks this workgroup walks (= its barriers)

    // ---- bias as fp32 in LDS (zeros without one): the epilogue reads four consecutive columns per ds_read_b128
    {
        float *sb = reinterpret_cast<float *>(smem + kHwBiasBase);
        for (int n = threadIdx.x; n < kHwN; n += kHwThreads) sb[n] = bias != nullptr ? elem_to_float<F16>(bias[n]) : 0.0f;
    }
    __syncthreads();

    // ---- LDS-DMA sources.  One wave-instruction fills 1 KiB = 8 rows x 128 B linearly: lane -> (row = lane >> 3, physical
    // piece lane & 7), which holds the LOGICAL piece (lane & 7) ^ ((row >> 1) & 7) of that row.
    constexpr int kWPieces = kHwWBytes / 1024 / kHwWaves;                    // 10 per wave and chunk
    const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)W, 0, kHwN * row_bytes, 0x00020000);
    int w_src[kWPieces];
#pragma unroll
    for (int i = 0; i < kWPieces; ++i) {
        const int n = (wave * kWPieces + i) * 8 + (lane >> 3);               // weight row = output column
        w_src[i] = n * row_bytes + ((((lane & 7) ^ ((n >> 1) & 7))) << 4);
    }
    int a_src[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wave * 32 + i * 8 + (lane >> 3);                     // row inside the tile (this wave's own rows)
        a_src[i] = row * row_bytes + ((((lane & 7) ^ ((row >> 1) & 7))) << 4);
    }

    // ---- operand fetch offsets: hidden row 32 * wave + l31, weight row 32j + l31; logical piece 2 * ks + half
    int a_rd[4], w_rd[4];
    {
        const int arow = wave * 32 + l31;
        const int ax = ((arow >> 1) & 7) << 4, wx = ((l31 >> 1) & 7) << 4;   // ((32j + l31) >> 1) & 7 does not depend on j
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            a_rd[ks] = arow * 128 + ((((2 * ks + half) << 4)) ^ ax);
            w_rd[ks] = kHwWBase + l31 * 128 + ((((2 * ks + half) << 4)) ^ wx);
        }
    }

    // ---- producer cursors over the flattened (tile, chunk) sequence of this workgroup
    int pa_tile = blockIdx.x, pa_chunk = 0, pa_slot = 0, pa_left = total;     // hidden states
    int pw_chunk = 0, pw_slot = 0, pw_left = total;                          // weights
    __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)X, 0, 0, 0x00020000);
    auto open_tile = [&]() {
        if (pa_tile < n_tiles) {
            const long long row0 = (long long)pa_tile * kHwBM;
            const long long rows = a.M - row0 < kHwBM ? a.M - row0 : kHwBM;   // rows past M read as zeros (bounds check)
            a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(X + (size_t)row0 * a.H), 0, (int)(rows * row_bytes), 0x00020000);
        }
    };
    open_tile();
    auto advance_a = [&]() {
        --pa_left;
        pa_slot = (pa_slot + 1 == kHwRingA) ? 0 : pa_slot + 1;
        if (++pa_chunk == n_chunks) {
            pa_chunk = 0;
            pa_tile += gridDim.x;
            open_tile();
        }
    };
    auto advance_w = [&]() {
        --pw_left;
        pw_slot ^= 1;
        pw_chunk = (pw_chunk + 1 == n_chunks) ? 0 : pw_chunk + 1;
    };
    auto issue_a = [&]() {                           // this wave's 32 rows of the next hidden-state chunk: streamed once -> nt
        if (pa_left == 0) return;
        char *dst = smem + pa_slot * kHwABytes + wave * 4096;
        const int soff = pa_chunk * (kHwBK * 2);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, MSIM_LDS(dst + i * 1024), 16, a_src[i], soff, 0, 2);
        advance_a();
    };
    auto issue_w = [&]() {                           // this wave's quarter of the next weight chunk
        if (pw_left == 0) return;
        char *dst = smem + kHwWBase + pw_slot * kHwWBytes + wave * (kWPieces * 1024);
        const int soff = pw_chunk * (kHwBK * 2);
#pragma unroll
        for (int i = 0; i < kWPieces; ++i)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, MSIM_LDS(dst + i * 1024), 16, w_src[i], soff, 0, 0);
        advance_w();
    };
    // issue order, here and in the loop: W(q) always leaves in front of A(q + 1), so when chunk q is about to be read the only
    // loads that may still be in flight are the 4 of A(q + 1)
    issue_a();
    issue_w();
    issue_a();

    int c_slot = 0, w_slot = 0, q = 0;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        f32x16 acc[kHwTilesN];
#pragma unroll
        for (int j = 0; j < kHwTilesN; ++j) acc[j] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

        for (int ch = 0; ch < n_chunks; ++ch, ++q) {
            // chunk q has landed (this wave's share).  Behind an epilogue the previous tile's stores are in the counter too:
            // wait for everything there instead of relying on their place in the queue.
            if (ch == 0 || q + 1 >= total) hw_wait_vmcnt<0>();
            else hw_wait_vmcnt<4>();
            __builtin_amdgcn_s_barrier();   // every wave's share of W(q) has landed; everyone is done reading W(q - 1)
            // W(q + 1) -> the slot of W(q - 1), A(q + 2) -> the slot of A(q - 1) (private to this wave): their 14 LDS-DMA pieces are
            // issued two at a time BEHIND each group of MFMAs below, not here in one piece -- a wave issues in order, and in front of
            // the MFMAs the matrix pipe sat idle while the four waves queued on the CU's one vector-memory path
            const bool feed_w = pw_left != 0, feed_a = pa_left != 0;        // wave-uniform
            char *const wdst = smem + kHwWBase + pw_slot * kHwWBytes + wave * (kWPieces * 1024);
            char *const adst = smem + pa_slot * kHwABytes + wave * 4096;
            const int wsoff = pw_chunk * (kHwBK * 2), asoff = pa_chunk * (kHwBK * 2);
            auto piece = [&](int k) {       // the same order as issue_w(); issue_a(): the vmcnt bookkeeping above counts on it
                if (k < kWPieces) {
                    if (feed_w) __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, MSIM_LDS(wdst + k * 1024), 16, w_src[k], wsoff, 0, 0);
                } else if (k < kWPieces + 4) {
                    if (feed_a) __builtin_amdgcn_raw_ptr_buffer_load_lds(a_rsrc, MSIM_LDS(adst + (k - kWPieces) * 1024), 16, a_src[k - kWPieces], asoff, 0, 2);
                }
            };
            const char *sa = smem + c_slot * kHwABytes;
            const char *sw = smem + w_slot * kHwWBytes;
            c_slot = (c_slot + 1 == kHwRingA) ? 0 : c_slot + 1;
            w_slot ^= 1;
            // The chunk's 40 MFMAs in 8 groups of 5 (k-step g >> 1, column tiles 5 * (g & 1) .. + 4); the operand fetch is software-
            // pipelined by hand ONE GROUP AHEAD of the MFMAs through two fragment buffers (40 + 8 VGPRs).  Left to itself hipcc keeps
            // one fragment register and issues ds_read -> s_waitcnt lgkmcnt(0) -> v_mfma forty times per chunk: with one wave per SIMD
            // nothing else hides the LDS round trip, and every MFMA waited one out (1000 x 779 x 2048 bf16: 1.60 ms in that form, 1.26
            // ms in this one).  Five independent MFMAs are 160 cycles of matrix pipe, more than an LDS round trip.  The scheduling
            // barriers keep the compiler from folding the stages back together; the waitcnt pass still derives the counted waits.
            bf16x8 hf[2], wf[2][5];
            auto fetch = [&](int g) {
                const int ks = g >> 1, j0 = (g & 1) * 5;
                if ((g & 1) == 0) hf[ks & 1] = *reinterpret_cast<const bf16x8 *>(sa + a_rd[ks]);
#pragma unroll
                for (int i = 0; i < 5; ++i) wf[g & 1][i] = *reinterpret_cast<const bf16x8 *>(sw + w_rd[ks] + (j0 + i) * 4096);
            };
            fetch(0);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                if (g + 1 < 8) fetch(g + 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < 5; ++i)   // A = weight rows = output columns (-> accumulator rows), B = hidden rows (-> lane column)
                    acc[(g & 1) * 5 + i] = mfma32<F16>(wf[g & 1][i], hf[(g >> 1) & 1], acc[(g & 1) * 5 + i]);
                __builtin_amdgcn_sched_barrier(0);
                piece(2 * g);
                piece(2 * g + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (feed_w) advance_w();
            if (feed_a) advance_a();
        }

        // ---- epilogue: acc[j][r] of lane (l31, half) = (hidden row 32 * wave + l31, output column 32j + acc_row(r, lane))
        const long long row0 = (long long)tile * kHwBM + wave * 32;
        const int32_t *rm = row_map + row0;            // wave-uniform address: read through the scalar cache
        int v = -1;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            const int sv = rm[i];
            v = l31 == i ? sv : v;
        }
        const char *sb = smem + kHwBiasBase + half * 16;
        float ssq = 0.0f;
#pragma unroll
        for (int j = 0; j < kHwTilesN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {              // registers 4g .. 4g+3 = columns 32j + 8g + 4 * half + 0..3
                const f32x4 bv = *reinterpret_cast<const f32x4 *>(sb + (j * 32 + g * 8) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float y = round_to_input<F16>(acc[j][4 * g + e] + bv[e]);
                    acc[j][4 * g + e] = y;
                    ssq += y * y;
                }
            }
        ssq += __shfl_xor(ssq, 32);                    // the other 160 columns of the same row
        const float nrm = round_to_input<F16>(sqrtf(ssq));
        if (v != -1) {
            const bool zero = v < 0;
            uint16_t *dst = out + (size_t)(zero ? -2 - v : v) * a.ld_out + 4 * half;
#pragma unroll
            for (int j = 0; j < kHwTilesN; ++j)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    uint16_t b4[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float o = round_to_input<F16>(acc[j][4 * g + e] / nrm);
                        if (zero) o *= 0.0f;           // `proj * attention_mask`: +-0 (sign kept), NaN stays NaN
                        if constexpr (F16) b4[e] = __builtin_bit_cast(uint16_t, (_Float16)o);
                        else b4[e] = (uint16_t)(__float_as_uint(o) >> 16);
                    }
                    uint2 w2;
                    w2.x = (uint32_t)b4[0] | ((uint32_t)b4[1] << 16);
                    w2.y = (uint32_t)b4[2] | ((uint32_t)b4[3] << 16);
                    *reinterpret_cast<uint2 *>(dst + j * 32 + 8 * g) = w2;
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Backward of the norm / mask tail at width 320: the formula of embed_head_bwd_rows_kernel,
//     dproj = mask * (g - y <g, y>) / n,   y = proj / n,   n = round(||proj||)
// (n rounded to the model dtype as Tensor.norm returns it; everything else in fp32, ONE rounding of the result).
// 320 elements = 40 pieces of 16 bytes: eight lanes per row with five pieces each (piece l8 + 8k: a row's eight lanes read 128
// contiguous bytes per step), so the two reductions take three shuffle steps.  HBM-bound: 2 x 640 B read + 640 B written per row.
template <bool F16>
__global__ __launch_bounds__(256) void embed_head_wide_bwd_rows_kernel(const uint16_t *__restrict__ proj, const uint16_t *__restrict__ g,
                                                                    const int32_t *__restrict__ row_map, long long M,
                                                                    uint16_t *__restrict__ dproj) {
    const int l8 = threadIdx.x & 7;
    const long long rows_per_pass = (long long)gridDim.x * 32;
    for (long long m = (long long)blockIdx.x * 32 + (threadIdx.x >> 3); m < M; m += rows_per_pass) {
        const bool keep = row_map[m] >= 0;
        float p[5][8], gg[5][8], ss = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const bf16x8 pv = *reinterpret_cast<const bf16x8 *>(proj + m * kHwN + (l8 + 8 * k) * 8);
            const bf16x8 gv = *reinterpret_cast<const bf16x8 *>(g + m * kHwN + (l8 + 8 * k) * 8);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                p[k][i] = elem_to_float<F16>((uint16_t)pv[i]);
                gg[k][i] = elem_to_float<F16>((uint16_t)gv[i]);
                ss += p[k][i] * p[k][i];
            }
        }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
        const float n = round_to_input<F16>(sqrtf(ss));
        const float inv = 1.0f / n;
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < 5; ++k)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                p[k][i] *= inv;
                dot += gg[k][i] * p[k][i];
            }
#pragma unroll
        for (int o = 4; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            bf16x8 ov;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float d = keep ? (gg[k][i] - p[k][i] * dot) * inv : 0.0f;
                uint16_t bits;
                if constexpr (F16) bits = __builtin_bit_cast(uint16_t, (_Float16)d);
                else bits = __builtin_bit_cast(uint16_t, (__bf16)d);
                ov[i] = (short)bits;
            }
            *reinterpret_cast<bf16x8 *>(dproj + m * kHwN + (l8 + 8 * k) * 8) = ov;
        }
    }
}

}  // namespace msim
