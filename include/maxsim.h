/*
 * include/maxsim.h -- C ABI of libmaxsim_gfx950.so, the MI355X-native MaxSim
 * (ColBERT late-interaction) scorer.
 *
 * The reference (illuin-tech/colpali) has no FFI layer: its hot path is two
 * Python call sites that delegate to torch.  These entry points are what a
 * binding for that path binds instead; each cites the reference lines it
 * replaces (paths relative to the reference checkout).  INTEGRATION.md shows
 * the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions (all entry points)
 *   - plain C types only; device buffers are raw device pointers; `stream` is a
 *     hipStream_t passed as void* (NULL = the null stream);
 *   - the caller owns every buffer: nothing is allocated, freed or synchronised
 *     inside a call, so every call is asynchronous on `stream` and can be
 *     captured in a hipGraph;
 *   - return 0 on success, a negative MSIM_E* code otherwise (never throws,
 *     never aborts); msim_last_error() gives a thread-local message;
 *   - matrices are row-major and contiguous, embeddings are 16-byte aligned.
 *
 * Data layout ("packed corpus")
 *   D        bf16|f16|f32 [total_rows, dim]  every document's patch embeddings, back to back
 *   d_off    int32 [n_d + 1]         document c owns rows d_off[c] .. d_off[c+1]-1
 *   d_clamp0 uint8 [n_d] or NULL     1 = the reference would have zero-padded this
 *                                    document inside its passage block, so a
 *                                    similarity of exactly 0 also takes part in
 *                                    every per-token max
 *                                    (colpali_engine/utils/processing_utils.py:175-178,
 *                                     pad_sequence(..., padding_value=0))
 *   Q        bf16|f16|f32 [n_q, Lq, dim]     queries (same dtype as D), zero rows = padding (they add 0)
 *
 * Flat query layout (msim_fwd_ragged; bf16 / f16, dim 128 or 320) -- queries are ragged in real use
 * (colpali_engine/utils/processing_utils.py:86 appends 10 augmentation tokens to a question of any length; a batch is
 * padded to its longest member, colpali_engine/collators/visual_retriever_collator.py:82-85) and a zero row adds exactly
 * 0 to every score, so the kernels take the real tokens only:
 *   Qt       bf16|f16 [T, dim]       every query's tokens back to back
 *   q_off    int32 [n_q + 1]         query q owns tokens q_off[q] .. q_off[q+1]-1 (on the device AND on the host: the
 *                                    launch plan -- which whole queries share a workgroup -- is made on the host)
 */
#ifndef COLPALI_AMD_MAXSIM_H
#define COLPALI_AMD_MAXSIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSIM_ABI_VERSION 22

/* error codes */
#define MSIM_OK 0
#define MSIM_EINVAL (-1)      /* bad argument (null pointer, negative size, misalignment) */
#define MSIM_EUNSUPPORTED (-2) /* shape/dtype outside what the gfx950 kernels implement */
#define MSIM_ELAUNCH (-3)      /* HIP reported an error at launch/configuration time */

/* embedding element types (`dtype` argument), fed to the MFMA as is, fp32 accumulate.
 * bf16 / f16 with dim == 128 and Lq <= 128 take the tuned kernels; every other combination (fp32 embeddings,
 * other widths such as ColQwen3's 320, longer queries) takes the generic kernels, which need
 * dim * sizeof(element) to be a multiple of 32 bytes (pad the width with zero columns) and <= 4096 bytes. */
#define MSIM_DTYPE_BF16 0
#define MSIM_DTYPE_F16 1
#define MSIM_DTYPE_F32 2

/* flags for msim_fwd */
#define MSIM_FLAG_REF_ROUNDING 0x1u /* reproduce the rounding the reference applies when torch computes the
                                       contraction in the embeddings' own dtype: every similarity rounded to
                                       that dtype before the max, the token sum rounded to it
                                       (processing_utils.py:179 evaluated on bf16 / fp16 tensors) */

#define MSIM_FLAG_AVG_ROWS(n) ((uint32_t)((n) < 0 ? 0 : ((n) > 65535 ? 65535 : (n))) << 8)
                                    /* optional launch-shape hint for msim_fwd / msim_fwd_ragged: the average number of rows per document
                                       (the row offsets live on the device; the launch plan is made on the host).  Only the number of
                                       document ranges the corpus is cut into depends on it -- speed, never a score.  0 = unknown. */

int msim_abi_version(void);
const char *msim_last_error(void);

/* Number of bytes of scratch msim_fwd can use for this problem (16-byte aligned device memory, contents irrelevant: the
 * call initialises what it uses on the stream).  Non-zero exactly when the launch plan holds several query blocks (bf16 / f16,
 * width 128: more than 1280 query tokens or 64 queries in total -- a block takes whole queries, up to 1024 or 1280 tokens): the
 * workgroups of an XCD that stream the same document range for different blocks then keep in step through progress counters, so
 * that the range is fetched from HBM once and served to the others from that XCD's L2.
 * Queries longer than 128 tokens (bf16 / f16, width 128: pages as queries, the trainer's symmetric direction) are scored as
 * 128-token pieces on the tuned kernels -- MaxSim is a sum over query tokens -- and need room for the partial sums:
 * 4096 + n_q * ceil(Lq / 128) * n_d * 4 bytes.
 * Passing NULL is legal and only switches those off (no convoy; long queries take the generic kernels: the same scores up to fp32
 * summation order, 3-4 x slower on a large corpus); a non-NULL workspace must hold at least the number of bytes this function
 * reports for the same problem.  One workspace per launch in flight. */
size_t msim_fwd_workspace_bytes(int dtype, int n_q, int Lq, int n_d, int dim);

/*
 * scores[q, c] = sum_{i < Lq} max_{j in doc c} <Q[q,i,:], D[j,:]>      (fp32 accumulate)
 *
 * Replaces the arithmetic of
 *   colpali_engine/utils/processing_utils.py:179
 *       torch.einsum("bnd,csd->bcns", qs_batch, ps_batch).max(dim=3)[0].sum(dim=2)
 *   colpali_engine/loss/late_interaction_losses.py:297-298 (+ :91)
 *       torch.einsum("bnd,csd->bcns", q, d) -> amax(dim=3) -> sum(dim=2)
 * without materialising the [b, c, n, s] similarity tensor.
 *
 * scores is fp32 [n_q, ld_scores] (ld_scores >= n_d).
 */
int msim_fwd(int dtype, const void *Q, int n_q, int Lq,
                  const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                  int n_d, int dim,
                  float *scores, int64_t ld_scores,
                  uint32_t flags, void *workspace, void *stream);

/*
 * The same scores on the HOST cores: every pointer is host memory, the call is synchronous and runs on `n_threads` native
 * threads (AVX-512 / AVX2 / baseline clones picked at load time).  This is what colpali_amd.score_multi_vector runs when the
 * caller names device="cpu" -- or passes no device on a host without a GPU -- through the reference's signature
 *   colpali_engine/utils/processing_utils.py:132-187 (the reference scores on whatever device it is given: :161, :172-179;
 *   colpali_engine/utils/torch_utils.py:12-31 answers "cpu" when no accelerator is visible);
 * it is never used on behalf of a GPU request.  fp32 products and sums of the exactly widened inputs (the kernels' truth tier:
 * within 1e-5 of a float64 evaluation); MSIM_FLAG_REF_ROUNDING as in msim_fwd.  Any dim >= 1, any Lq >= 0; bf16 / f16 / f32.
 * msim_host_last_error() gives its thread-local message.
 */
const char *msim_host_last_error(void);
int msim_fwd_host(int dtype, const void *Q, int n_q, int Lq,
                  const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                  int n_d, int dim,
                  float *scores, int64_t ld_scores,
                  uint32_t flags, int n_threads);
/* The same without any packing: query q = q_rows[q] rows of `dim` elements at q_ptr[q], document c = d_rows[c] rows at d_ptr[c] -- the
 * caller's own host tensors (a list of ragged queries and passages is what the reference's callers hold: README.md:121-126); nothing
 * is copied, and only the real tokens of a ragged query are multiplied. */
int msim_fwd_host_lists(int dtype, const void *const *q_ptr, const int64_t *q_rows, int n_q,
                        const void *const *d_ptr, const int64_t *d_rows, const uint8_t *d_clamp0,
                        int n_d, int dim,
                        float *scores, int64_t ld_scores,
                        uint32_t flags, int n_threads);
/* out[i, j] = <A_i, B_j> on the host cores (score_single_vector with device="cpu": processing_utils.py:103-130) */
int msim_sim_matrix_host(int dtype, const void *A, int n_a, const void *B, int n_b, int dim,
                         float *out, int64_t ld_out, uint32_t flags, int n_threads);

/*
 * The same scores for RAGGED queries in the flat layout: scores[q, c] = sum over the tokens i of query q of
 * max_{j in doc c} <Qt[q_off[q] + i, :], D[j, :]>.  A query's score is a pure function of its own tokens and the
 * document (the token sum runs in an order fixed by the query's length alone), so it does not depend on the batch it is
 * scored in, on the kernel shape the plan picks, or on whether msim_fwd or msim_fwd_ragged computed it (for queries of up
 * to 128 tokens).  bf16 / f16 embeddings of width 128, a query of 0 .. 1280 tokens -- or of width 320 (ColQwen3,
 * models/qwen3/colqwen3/modeling_colqwen3.py:48: the flat panel kernel K1bPF), a query of 0 .. 512 tokens; MSIM_EUNSUPPORTED otherwise:
 * pad the queries to one length and call msim_fwd.  At width 320 a call of ONE query length and at most four 32-token tiles in all is
 * streamed by K1sP, whose token sum is a butterfly: there the bits depend on which kernel ran (values agree to fp32 summation
 * order); every other width-320 call of THIS entry is batch-independent like width 128.  (msim_fwd on a width-320 box whose Lq is a
 * multiple of 32 runs K1sP / K1bP -- butterfly sums as well: equal to this entry's result up to fp32 summation order, not bit for bit;
 * any other Lq <= 512 runs the flat kernel and returns this entry's bits.)  `q_off` is the device copy, `q_off_host` the host copy of the same
 * n_q + 1 numbers (read during the call only).  Workspace as msim_fwd's: msim_fwd_ragged_workspace_bytes() bytes or NULL.
 * Replaces the same reference lines as msim_fwd (processing_utils.py:172-179 with its pad_sequence of the query block).
 */
/* Which kernel shape a tuned forward call (bf16 / f16, width 128) takes for these queries -- host-only, no device work; the same
 * plan msim_fwd / msim_fwd_ragged make.  q_off_host = the n_q + 1 token offsets, or NULL for n_q uniform queries of Lq tokens
 * (more than 128 tokens: the 128-token pieces msim_fwd scores with a workspace).  out5 = { 0 = K1s (every wave holds all units:
 * HBM-bound regime) | 1 = K1b (waves share a document stream),  K1s: 16-token units per wave | K1b: waves per stream (2, 4, 8),
 * K1b: units a wave holds at most (8, 10),  query blocks (passes over a document range),  units of the heaviest wave }. */
int msim_fwd_plan(const int32_t *q_off_host, int n_q, int Lq, int32_t *out5);
size_t msim_fwd_ragged_workspace_bytes(int dtype, const int32_t *q_off_host, int n_q, int n_d, int dim);
int msim_fwd_ragged(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q,
                    const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                    int n_d, int dim,
                    float *scores, int64_t ld_scores,
                    uint32_t flags, void *workspace, void *stream);

/*
 * THE 13-BIT IMAGE of a resident bf16 corpus of width 128.  Rows the scorers see are L2-normalised, so the exponent field of (all
 * but a handful of) their values lies in [96, 127] and bits 14..12 of the 16-bit pattern are the constant 011: the image keeps the
 * other 13 bits -- 0.8125 x the bytes, lossless -- in 6656-byte slabs of 32 rows laid out in the order a wave of the few-query stream
 * kernel (K1s) consumes them.  The format is private to the library (csrc/pack13.hip) and may change with it: build the image with
 * the library that scans it.  A document that holds ONE value outside the range (zero, denormal, |x| < 2^-31, |x| >= 2, inf, NaN)
 * is FLAGGED; the forward entries below score flagged documents from the blob, so every score carries the bits msim_fwd /
 * msim_fwd_ragged return.
 *   slab_off  int32 [n_d + 1]  made by the caller: slab_off[0] = 0, slab_off[c + 1] = slab_off[c] + ceil(rows of document c / 32)
 *   image     msim_pack13_image_bytes(slab_off[n_d]) bytes, 16-byte aligned
 *   flagged   uint8 [n_d], list int32 [n_d] (the flagged ids, ascending), count int32 [1]      -- written by the encoder
 * msim_pack13_encode is one pass over the blob (asynchronous on `stream`; read `count` after synchronising).  msim_pack13_decode
 * is a test aid: the image back as [rows, 128] bf16 rows (those of flagged documents decode to other values).
 * msim_fwd_pack13 / msim_fwd_ragged_pack13 take the image beside the arguments of msim_fwd / msim_fwd_ragged and return the same
 * bits: calls whose plan is K1s (msim_fwd_plan: at most 8 queries and 128 tokens in all) on bf16 rows of width 128 scan the image
 * -- plus one list-driven launch of K1s over the blob when n_list > 0 --, every other call ignores the image and runs as without it.
 * `list` holds the n_list = *count flagged ids (NULL when n_list is 0).
 */
size_t msim_pack13_image_bytes(int64_t n_slabs);
int msim_pack13_encode(const void *D, const int32_t *d_off, const int32_t *slab_off, int n_d, int64_t n_slabs, void *image,
                       uint8_t *flagged, int32_t *list, int32_t *count, void *stream);
int msim_pack13_decode(const void *image, const int32_t *d_off, const int32_t *slab_off, int n_d, int64_t n_slabs, void *out,
                       void *stream);
int msim_fwd_pack13(int dtype, const void *Q, int n_q, int Lq, const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                    int n_d, int dim, const void *image, const int32_t *slab_off, const uint8_t *flagged, const int32_t *list,
                    int n_list, float *scores, int64_t ld_scores, uint32_t flags, void *workspace, void *stream);
int msim_fwd_ragged_pack13(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const void *D,
                           const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim, const void *image,
                           const int32_t *slab_off, const uint8_t *flagged, const int32_t *list, int n_list, float *scores,
                           int64_t ld_scores, uint32_t flags, void *workspace, void *stream);

/*
 * RERANKING: the same scores for a LIST of candidate documents per query -- the exact second stage behind a cheap first one (pooled
 * pages, BM25, a bi-encoder, a metadata filter, hard-negative mining).  For every entry (q, j) of cand [n_q, m] (row stride
 * ld_cand >= m, int64 GLOBAL ids; the shard's document c has id id_base + c):
 *     out_scores[q, j] = scores[q, cand[q, j] - id_base]   of msim_fwd_ragged on the same queries, corpus and flags -- bit for bit
 *     out_ids[q, j]    = cand[q, j]                        (out_ids: int64 [n_q, ld_scores], or NULL)
 * An entry whose id is -1, or outside [id_base, id_base + n_d), is written as (-inf, -1) and reads no document; a query of 0 tokens
 * scores 0.  A duplicate id is scored once per occurrence (identical bits).  out_scores fp32 [n_q, ld_scores], ld_scores >= m.
 * Queries in the flat layout (q_off on the device, q_off_host the same n_q + 1 numbers on the host, read during the call only), bf16 /
 * f16, width 128, 0 .. 128 tokens per query (MSIM_EUNSUPPORTED otherwise); d_clamp0 and MSIM_FLAG_REF_ROUNDING as msim_fwd (no other
 * flag).  The candidate matrix is inverted ON THE DEVICE into work items -- one document and up to eight 16-token units of the
 * queries that listed it -- so a document is read once per group of queries that listed it, not once per entry (kernel K1c,
 * maxsim_candidates.hip); the host never reads the list, so the call is asynchronous and hipGraph-capturable like the others.
 * Every index the device derives is checked before it becomes an address; a broken invariant (a device q_off that disagrees with
 * q_off_host, or a library bug) makes every score of the call NaN instead of leaving one unwritten.
 * workspace: msim_fwd_candidates_workspace_bytes(n_q, m, n_d) bytes (0 when there is no entry), 16-byte aligned, contents
 * irrelevant; one per call in flight.  After the call its first int32 is 0, or the bits of the broken invariant.
 * ld_cand >= m: a list shared by every query is passed once per row (the binding copies a broadcast view).
 */
size_t msim_fwd_candidates_workspace_bytes(int n_q, int m, int n_d);
int msim_fwd_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q,
                        const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim,
                        const int64_t *cand, int m, int64_t ld_cand, int64_t id_base,
                        float *out_scores, int64_t ld_scores, int64_t *out_ids /* or NULL */,
                        unsigned flags, void *workspace, void *stream);

/*
 * RERANKING at width 320 (ColQwen3, models/qwen3/colqwen3/modeling_colqwen3.py:48) -- an addition to ABI 22; msim_fwd_candidates
 * itself keeps refusing every width but 128.  The contract is msim_fwd_candidates' with "width 128" replaced by "width 320": for
 * every entry (q, j) of cand [n_q, m] (row stride ld_cand >= m, int64 GLOBAL ids; the shard's document c has id id_base + c)
 *     out_scores[q, j] = scores[q, cand[q, j] - id_base]   of msim_fwd_ragged on the same queries, corpus and flags
 *     out_ids[q, j]    = cand[q, j]                        (out_ids: int64 [n_q, ld_scores], or NULL)
 * An entry whose id is -1, or outside [id_base, id_base + n_d), is written as (-inf, -1) and reads no document; a query of 0 tokens
 * scores 0; a duplicate id is scored once per occurrence (identical bits).  bf16 / f16, dim == 320 ONLY (this entry does not serve
 * width 128: call msim_fwd_candidates), 0 .. 128 tokens per query; MSIM_EUNSUPPORTED for other dtypes, widths and longer queries;
 * MSIM_EINVAL for a null or misaligned pointer, ld < m, an unknown flag, a non-monotone q_off_host.  Nothing to do (n_q == 0 or
 * m == 0) returns 0 before any pointer is looked at.  d_clamp0 and MSIM_FLAG_REF_ROUNDING as msim_fwd (no other flag).
 * BITS: out_scores[q, j] carries the bits msim_fwd_ragged gives the same query and document WHEN THE FLAT PANEL KERNEL K1bPF
 * COMPUTES IT -- the MFMA chain across the column panels in K1bPF's order and the token sum in the order fixed by the query's
 * length alone -- so a reranked score does not depend on the batch, the list, the grouping into work items or a rerun.  The one
 * exception is the scan side's (see msim_fwd_ragged above): a width-320 msim_fwd_ragged call of ONE query length and at most four
 * 32-token tiles in all runs K1sP, whose token sum is a butterfly.  Against such a call the per-token maxima are identical and the
 * scores agree to fp32 summation order: |difference| <= 2 * g(L - 1) * sum_i |M_i|, g(n) = n 2^-24 / (1 - n 2^-24), L the query's
 * token count, M_i its per-token maxima.
 * The candidate matrix is inverted on the device exactly as in msim_fwd_candidates (the same kernels; work items of one document
 * and up to eight 16-token units); the item scorer is the panel form K1cP (maxsim_candidates_panels.hip).  Asynchronous on `stream`,
 * no allocation, no host synchronisation, hipGraph-capturable (the counters are zeroed by a kernel node).  Every index the device
 * derives is checked before it becomes an address; a broken invariant makes every score of the call NaN.
 * workspace: msim_fwd_candidates_wide_workspace_bytes(n_q, m, n_d, dim) bytes (0 when there is no entry), 16-byte aligned, contents
 * irrelevant; one per call in flight.  After the call its first int32 is 0, or the bits of the broken invariant.
 * NOT served at width 320: the int8 first stage (msim_i8_*: width 128 only), fp32.  The FDE encoders msim_fde_encode_* are width
 * 128 only; width 320 has encoders of its own (msim_fdew_encode_*), scored by msim_fde_scores.
 */
size_t msim_fwd_candidates_wide_workspace_bytes(int n_q, int m, int n_d, int dim);
int msim_fwd_candidates_wide(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q,
                             const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim,
                             const int64_t *cand, int m, int64_t ld_cand, int64_t id_base,
                             float *out_scores, int64_t ld_scores, int64_t *out_ids /* or NULL */,
                             unsigned flags, void *workspace, void *stream);

/*
 * TOKEN-TO-PATCH ALIGNMENT of listed entries -- an addition to ABI 22: which rows of a hit page matched each query token, and the
 * similarity map behind it (colpali_engine/interpretability/similarity_map_utils.py:9-55: einsum("bnk,bijk->bnij") of one query
 * with one image's patch grid), for pages that live in the packed corpus.  Entry (q, j) of cand [n_q, m] (row stride ld_cand >= m,
 * int64 GLOBAL ids) is resolved as msim_fwd_candidates resolves it: an id of -1, or outside [id_base, id_base + n_d), is no page.
 * For every token slot i < max_q_tokens (the caller's host bound on tokens per query, at most 128) of every entry:
 *     best_sim[q, j, i] = max_{r < len(page)} <Qt[q_off[q] + i], D[d_off[c] + r]>      fp32 accumulation
 *     best_row[q, j, i] = the FIRST r that attains it (relative to the page)
 *     sims[q, j, i, r]  = <Qt[q_off[q] + i], D[d_off[c] + r]>                           (sims != NULL: the similarity map)
 * best_sim fp32 and best_row int32 are [n_q, m, max_q_tokens]; sims fp32 is [n_q, m, max_q_tokens, max_rows] or NULL, max_rows the
 * caller's host bound on the rows of a listed page.  In sims the columns r >= len(page) and the token slots i >= len(query) hold
 * -inf.  The conventions are those of msim_pairs_argmax:
 *   - under d_clamp0[c] a token whose maximum is negative reports (0.0, -1) (the reference's zero padding row wins), and so does
 *     a flagged page of 0 rows; sims is not clamped;
 *   - an unflagged page of 0 rows, or an entry without a page, reports (-inf, -1) for the query's tokens;
 *   - a token slot past the query's end reports (0.0, -1);
 *   - an entry whose page has more than max_rows rows (whether or not sims is passed), or whose offsets break an invariant --
 *     q_off not within [0, q_rows] and non-decreasing, a query of more than max_q_tokens tokens, d_off not within [0, d_rows] --
 *     is written as NaN / -1 in full; its neighbours are untouched.  Every offset is checked on the device before it becomes an
 *     address: nothing is read or written out of bounds, and the host reads neither the list nor the offsets.
 * BITS: one fp32 accumulator chain per similarity, k ascending (v_mfma_f32_16x16x32, dim / 32 steps): the bits of a similarity
 * depend on its token row and its page row alone -- the same at any list position, in any batch, under any m, with or without sims;
 * best_sim is the maximum of its row of sims bit for bit (before the clamp).
 * bf16 / f16, dim 128 or 320 (MSIM_EUNSUPPORTED otherwise, and for max_q_tokens > 128); Qt [q_rows, dim], D [d_rows, dim] 16-byte
 * aligned.  n_q == 0 or m == 0 returns 0 before any pointer is looked at.  One 4-wave workgroup per entry (kernel K1a,
 * maxsim_align.hip); no workspace, no allocation, no synchronisation: asynchronous on `stream`, hipGraph-capturable.
 */
int msim_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                          const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int64_t d_rows, int dim,
                          const int64_t *cand, int m, int64_t ld_cand, int64_t id_base,
                          float *best_sim, int32_t *best_row,            /* [n_q, m, max_q_tokens] */
                          float *sims /* or NULL */, int max_rows,       /* [n_q, m, max_q_tokens, max_rows] */
                          void *stream);

/*
 * The same scores for two DENSE BOXES when the queries are long and the documents short -- the symmetric direction of the reference
 * trainer (trainer/contrastive_trainer.py:202-206, compute_symetric_loss: the pages as query_embeddings [B, 780, 128], the gathered
 * queries as doc_embeddings [C, 32, 128]; late_interaction_losses.py:297-298):
 *     scores[q, c] = sum_{i < Lq} max_{j < Ld} <Q[q, i, :], D[c, j, :]>
 * Q [n_q, Lq, 128], D [n_d, Ld, 128] (bf16 | f16, Ld <= 128; every row of a box takes part, zero padding rows included, as in the
 * reference), scores fp32 [n_q, ld_scores].  The long side streams, the short side is resident (kernel K1t, maxsim_batch_t.hip):
 * msim_fwd gives the same numbers up to fp32 summation order, 2-3 x slower on this shape (a 32-row document is one slab).
 * q_lengths: NULL, or int32 [n_q] that receives, as a by-product of streaming every query row, the number of rows of query q whose
 * first component is non-zero -- the `lengths` of late_interaction_losses.py:296, which msim_loss_epilogue accepts ready-made.
 */
int msim_fwd_transposed(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim,
                        float *scores, int64_t ld_scores, int32_t *q_lengths, void *stream);

/*
 * The DENSE hard-max backward of that shape on the matrix cores (round 6; maxsim_dense_t.hip) -- what autograd derives for
 * late_interaction_losses.py:297-298 when EVERY (query, document) pair carries a gradient: ColbertLoss (:140-164, the trainer's
 * default loss, trainer/colmodel_training.py:33) and ColbertSigmoidLoss (:440-465) in the trainer's symmetric direction
 * (trainer/contrastive_trainer.py:202-206).  bf16 | f16, width 128, documents of at most 64 rows (msim_dense_t_supported; every
 * other shape keeps msim_pairs_bwd).
 *   msim_fwd_transposed_route   msim_fwd_transposed (bit-identical scores) that also leaves the ROUTING: route uint8
 *                               [n_q, n_d, Lq_pad] (Lq_pad = Lq rounded up to 64; msim_dense_t_route_bytes), route[q, c, i] = the row of
 *                               document c that won the max for row i of query q (the first maximal row on a tie); bytes of rows i >= Lq are unspecified
 *                               (they never reach a result: those rows of the query image are zero and no gradient is stored for them).
 *   msim_dense_t_bwd            dQ[q, i, :] = sum_c G[q, c] * g_scale * D[c, route[q, c, i], :]
 *                               dD[c, s, :] = sum_q sum_{i : route[q, c, i] = s} G[q, c] * g_scale * Q[q, i, :]
 *                               as two GEMMs against a G-scaled one-hot operand built in registers (v_mfma_f32_16x16x32), G rounded to
 *                               the embeddings' dtype per term, fp32 sums in a fixed order (no float atomics), dQ / dD written in the
 *                               embeddings' dtype.  G fp32 [n_q, ldg]; g_scale: NULL or one device scalar (dtype code g_scale_dtype).
 *                               workspace: msim_dense_t_bwd_workspace_bytes bytes, 16-byte aligned, contents irrelevant.
 */
int msim_dense_t_supported(int dtype, int n_q, int Lq, int n_d, int Ld, int dim);
size_t msim_dense_t_route_bytes(int n_q, int Lq, int n_d);
int msim_fwd_transposed_route(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim,
                              float *scores, int64_t ld_scores, int32_t *q_lengths, uint8_t *route, void *stream);
size_t msim_dense_t_bwd_workspace_bytes(int n_q, int Lq, int n_d, int Ld, int dim);
int msim_dense_t_bwd(int dtype, const void *Q, int n_q, int Lq, const void *D, int n_d, int Ld, int dim,
                     const float *G, int64_t ldg, const void *g_scale, int g_scale_dtype, const uint8_t *route,
                     void *dQ, void *dD, void *workspace, void *stream);

/*
 * Packing queries into the flat layout: rows that are entirely zero (the model's padded positions,
 * modeling_colpali.py:72 / modeling_colqwen2.py:69; byte-wise test) are dropped, the others keep their order.
 *   msim_query_compact        device: box [n_q, Lq, row_bytes] (row_bytes a multiple of 16, Lq <= 4096).  counts != NULL:
 *                             counts[q] = rows of query q that are not all-zero.  out != NULL: those rows are copied to rows
 *                             q_off[q] .. of `out`.  (Call once for the counts, build q_off, call again to copy.)
 *   msim_host_count_nonzero_rows / msim_host_gather_nonzero_rows
 *                             host (native threads; synchronous): the same for a list of host buffers src[i] of rows[i] rows --
 *                             counts, then the copy of source i's non-zero rows to row dst_row[i] .. of `dst` (pinned staging).
 * Both forms are two passes over the same data (count, then copy to offsets built from the counts): the sources must not change in
 * between -- the copy trusts the offsets.
 */
int msim_query_compact(const void *box, int n_q, int Lq, int row_bytes, const int32_t *q_off, int32_t *counts, void *out,
                       void *stream);
int msim_host_count_nonzero_rows(const void *const *src, const int64_t *rows, int64_t row_bytes, int64_t n, int32_t *counts,
                                 int n_threads);
int msim_host_gather_nonzero_rows(void *dst, const void *const *src, const int64_t *rows, int64_t row_bytes,
                                  const int64_t *dst_row, int64_t n, int n_threads);

/*
 * MaxSim for an explicit list of (query, document) pairs, optionally reporting for every
 * (pair, query token) the document row (relative to the document) that attains the max;
 * -1 when the reference's zero padding row wins (d_clamp0).  First maximum wins on ties.
 * This is the routing autograd derives for amax in
 *   colpali_engine/loss/late_interaction_losses.py:298 -> :91 (scores_raw.amax(dim=dim_max)),
 * and the forward of the paired contractions "bnd,bsd->bns" / "bnd,blsd->blns" (:235-238, :381-384).
 * pairs: int32 [n_pairs, 2] = (query index, document index).
 * out_scores: fp32 [n_pairs] or NULL; out_argmax: int32 [n_pairs, Lq] or NULL.
 * max_doc_rows: an upper bound of the longest document's rows, or 0 = unknown.  It only selects the kernel: queries of more than
 * 128 tokens against documents of at most 128 rows (bf16 / f16, dim 128: the trainer's symmetric direction,
 * trainer/contrastive_trainer.py:202-206 -- pages as query_embeddings, queries as doc_embeddings) take the transposed pair
 * kernel (the long side streams, the short side is resident); with 0 they take the generic kernel (same results up to ties'
 * first-maximum rule, which both follow).  Short lists (<= 1024 pairs) are worked on by one workgroup per pair, long ones by one
 * wave per pair.
 */
int msim_pairs_argmax(int dtype, const void *Q, int n_q, int Lq,
                      const void *D, const int32_t *d_off, const uint8_t *d_clamp0,
                      int n_d, int dim, int max_doc_rows,
                      const int32_t *pairs, int n_pairs,
                      float *out_scores, int32_t *out_argmax, void *stream);

/*
 * The same for ALL n_q x n_d pairs (the row-major all-pairs list without the list): scores [n_q, ld_scores] and
 * out_argmax [(q * n_d + c), Lq] -- the forward of the in-batch losses whose upstream gradient is dense (ColbertLoss :152-164,
 * ColbertSigmoidLoss :444-465), which keep the routing for the backward.  A wave scores up to four queries (<= 128 tokens in all)
 * against one document, so a document is streamed once per GROUP of queries instead of once per pair.  bf16 / f16, dim 128, Lq <= 128
 * (MSIM_EUNSUPPORTED otherwise: list the pairs and call msim_pairs_argmax).  Either output may be NULL.
 */
int msim_allpairs_argmax(int dtype, const void *Q, int n_q, int Lq,
                         const void *D, const int32_t *d_off, const uint8_t *d_clamp0, int n_d, int dim,
                         float *out_scores, int64_t ld_scores, int32_t *out_argmax, void *stream);

/*
 * Backward of the contraction for a sparse set of (q, c) pairs with upstream gradient
 * g[p] = dLoss/dscores[q_p, c_p]:
 *     dQ[q, i, :]        = sum_p g[p] * D[d_off[c_p] + argmax[p, i], :]
 *     dD[d_off[c]+r, :]  = sum_{p, i : c_p = c, argmax[p, i] = r} g[p] * Q[q_p, i, :]
 * i.e. what autograd produces for einsum -> amax -> sum
 * (late_interaction_losses.py:297-298) restricted to the pairs whose upstream gradient is
 * non-zero (for ColbertPairwiseCELoss, :309-313, two per query).
 * dQ [n_q, Lq, dim] and dD [total_rows, dim] are fully overwritten (rows without a contribution are set to 0), as fp32
 * (out_dtype = MSIM_DTYPE_F32) or in the embeddings' own dtype (out_dtype = dtype: one rounding of the fp32 sum -- what autograd's
 * `.to(dtype)` would do in a launch of its own).  Deterministic: no floating-point atomics.
 * g_scale: NULL, or a DEVICE scalar (g_scale_dtype: bf16 / f16 / f32) every g[p] is multiplied by -- the loss' upstream gradient as
 * autograd hands it over (a 0-dim tensor), folded into the kernels instead of a `coef * grad` launch in front of them.
 * `pairs` must be sorted by query index; `order_by_doc` is a permutation of 0..n_pairs-1 that
 * sorts the pairs by document index (stable); `max_doc_rows` >= the longest document.
 * `workspace`: msim_pairs_bwd_workspace_bytes() bytes of 16-byte aligned device scratch (contents irrelevant), or NULL.  It is
 * non-zero when short documents (<= 64 rows) collect long entry lists -- the symmetric direction of the reference trainer
 * (trainer/contrastive_trainer.py:202-206: pages as query_embeddings, queries as doc_embeddings), dense upstream gradients or
 * queries of 256 tokens and more: every document's pair list
 * is then split over several workgroups whose partial sums are added in split order (still deterministic, still no atomics).
 * NULL is legal and only selects the one-workgroup-per-row-range form (the same values up to fp32 summation order).
 */
size_t msim_pairs_bwd_workspace_bytes(int n_q, int Lq, int n_d, int dim, int max_doc_rows, int n_pairs);
int msim_pairs_bwd(int dtype, const void *Q, int n_q, int Lq,
                   const void *D, const int32_t *d_off, int n_d, int dim, int max_doc_rows,
                   const int32_t *pairs, const int32_t *order_by_doc,
                   const float *g, const void *g_scale, int g_scale_dtype,
                   const int32_t *argmax, int n_pairs,
                   int out_dtype, void *dQ, void *dD, void *workspace, void *stream);

/*
 * Smooth-max late interaction (training losses constructed with use_smooth_max=True):
 *     scores[q, c] = sum_{i < Lq} tau * log sum_{j in doc c} exp(<Q[q,i,:], D[j,:]> / tau)
 * Replaces colpali_engine/loss/late_interaction_losses.py:40-44 (_smooth_max = tau * logsumexp(scores / tau)) applied
 * through :88-90 (_aggregate) to the einsum of :153 / :297 / :444, again without the [b, c, n, s] tensor.  Every row of a
 * document takes part (physical zero padding rows contribute exp(0), as in the reference); there is no d_clamp0 here
 * because score_multi_vector has no smooth-max mode.  dim * sizeof(element) must be a multiple of 32 bytes, <= 4096.
 *
 * msim_smooth_pairs: the same for an explicit pair list; out_lse [n_pairs, Lq] receives the natural-log
 *     lse[p, i] = log sum_j exp(<Q[q_p,i], D[j]> / tau)     (what the backward needs; either output may be NULL).
 * msim_smooth_pairs_bwd: autograd of the expression for the listed pairs with upstream gradient g[p]:
 *     w[p,i,j] = exp(<Q[q_p,i], D[j]> / tau - lse[p,i])     (softmax over the document's rows)
 *     dQ[q, i, :]       = sum_{p: q_p = q} g[p] * sum_j w[p,i,j] * D[d_off[c_p] + j, :]
 *     dD[d_off[c]+j, :] = sum_{p: c_p = c} g[p] * sum_i w[p,i,j] * Q[q_p, i, :]
 * Same conventions as msim_pairs_bwd (pairs sorted by query, order_by_doc, full overwrite, deterministic, no atomics).
 * The dQ pass splits a query's pair list over several workgroups and sums their partial results in a fixed order: it
 * needs msim_smooth_bwd_workspace_bytes(n_q, Lq, dim) bytes of scratch (16-byte aligned; 0 = none needed).
 *
 * A document without rows (d_off[c + 1] == d_off[c]): its score and every lse[p, i] of its pairs are -inf (the logsumexp over
 * nothing, as torch.logsumexp gives it).  msim_smooth_pairs_bwd accepts such pairs with that lse: they contribute nothing, and the
 * gradients of every other pair in the list are finite and unchanged.
 * A pair with an index out of range (q outside [0, n_q) or c outside [0, n_d)) is a caller error: msim_smooth_pairs skips it and
 * leaves out_scores[p] and out_lse[p, :] untouched, every other pair is computed as usual.  msim_smooth_pairs_bwd does NOT check:
 * every pair handed to it must be in range.
 * Range of g: any finite fp32 values, for every dtype.  The result is linear in the scale of g up to fp32 rounding: for fp16
 * embeddings the weights g[p] * w are normalised by the power of two at the largest |g| of each query's (dQ) / document's (dD) pair
 * list before they are split into fp16 pieces, so neither a tiny g (loss weights, gradient accumulation) nor a large one (an fp16
 * GradScaler) leaves fp16's exponent range; within one such list a weight more than 2^-24 below the largest |g| is lost, as it is
 * against fp32 accumulation anyway.  bf16 and fp32 embeddings use g as it is.
 */
int msim_smooth_fwd(int dtype, const void *Q, int n_q, int Lq,
                    const void *D, const int32_t *d_off, int n_d, int dim, float tau,
                    float *scores, int64_t ld_scores, void *stream);
int msim_smooth_pairs(int dtype, const void *Q, int n_q, int Lq,
                      const void *D, const int32_t *d_off, int n_d, int dim,
                      const int32_t *pairs, int n_pairs, float tau,
                      float *out_scores, float *out_lse, void *stream);
size_t msim_smooth_bwd_workspace_bytes(int n_q, int Lq, int dim);
int msim_smooth_pairs_bwd(int dtype, const void *Q, int n_q, int Lq,
                          const void *D, const int32_t *d_off, int n_d, int dim, int max_doc_rows,
                          const int32_t *pairs, const int32_t *order_by_doc,
                          const float *g, const float *lse, int n_pairs, float tau,
                          float *dQ, float *dD, void *workspace, void *stream);

/*
 * The [B, C]-sized epilogue of the in-batch losses, value and gradient with respect to the MaxSim scores in one launch
 * (no host synchronisation, hipGraph-capturable).  Replaces, for scores = the raw MaxSim matrix of msim_fwd / msim_pairs_argmax,
 *   colpali_engine/loss/late_interaction_losses.py:296 (lengths), :300-301 (normalisation), :303-307 (pos-aware filtering) and
 *   MSIM_LOSS_PAIRWISE  :309-313  softplus((hardest in-batch negative - positive) / T).mean()     (ColbertPairwiseCELoss)
 *   MSIM_LOSS_INFONCE   :164      cross_entropy(scores / T, pos_idx)                                (ColbertLoss)
 *   MSIM_LOSS_SIGMOID   :457-465  softplus(-scores.view(-1) / T * sign).mean(), sign +1 on the diagonal of the in-batch square,
 *                                 -1 elsewhere (C == B, offset == 0)                                (ColbertSigmoidLoss; round 6)
 * together with what autograd derives for them:
 *   PAIRWISE  pairs int32 [2B, 2] = the two (query, doc) entries per query that carry a gradient (positive, selected negative),
 *             sorted by (query, doc); coef fp32 [2B] = dLoss/dscore of each for a unit upstream gradient; order int32 [2B] = the
 *             stable by-document permutation msim_pairs_bwd wants.  Always exactly 2B pairs: nothing to read back.  C >= 2.
 *   INFONCE, SIGMOID   G fp32 [B, ld] = dLoss/dscores (dense).
 * Q [B, Lq, width] are the query embeddings (q_dtype as in msim_fwd): lengths[b] = number of tokens whose first component is
 * non-zero.  out fp32 [3] = loss, min and max of the normalised scores (the reference prints when they leave [-tol, 1+tol]).
 * q_lengths: NULL (the token counts are taken from Q here), or int32 [B] = lengths[b] ready-made (msim_fwd_transposed's by-product:
 * for 780-token "queries" -- the trainer's symmetric direction -- counting them here means one cache line per token on one CU).
 * loss_out: NULL, or one element of q_dtype that receives the loss rounded to the embeddings' dtype (what the reference's forward
 * returns: bf16 in -> bf16 scalar) -- no cast launch behind the kernel.
 * workspace: msim_loss_epilogue_workspace_bytes(B, C) bytes, 16-byte aligned, ZERO-FILLED once by the caller before its first use
 * (the call leaves it ready for the next one); one workspace per stream.  0 bytes (workspace may be NULL) for small batches --
 * B <= 1024 and B * C <= 262 144, BASELINE config 5's 32 x 256 among them: one workgroup reads the whole score matrix, one wave per
 * row, and keeps the per-row terms in LDS; larger ones run one workgroup per row and a ticket.  offset + B <= C.
 */
#define MSIM_LOSS_PAIRWISE 0
#define MSIM_LOSS_INFONCE 1
#define MSIM_LOSS_SIGMOID 2
size_t msim_loss_epilogue_workspace_bytes(int B, int C);
int msim_loss_epilogue(int mode, const float *scores, int64_t ld, int B, int C,
                       const void *Q, int q_dtype, int Lq, int width, int offset,
                       float temperature, int normalize, int filter, float filter_threshold, float filter_factor,
                       float *G, int32_t *pairs, float *coef, int32_t *order,
                       void *workspace, float *out, void *loss_out, const int32_t *q_lengths, void *stream);

/*
 * Embedding head: the last three lines of every Col* model forward, producing the scorer's corpus format.
 *     y   = X @ W^T + bias                       nn.Linear(hidden, 128)
 *     y   = y / ||y||_2                          (row-wise, rounding chain of the model dtype)
 *     out = y * mask
 * Replaces colpali_engine/models/paligemma/colpali/modeling_colpali.py:67-77 and
 * colpali_engine/models/qwen2/colqwen2/modeling_colqwen2.py:65-74 (identical in the other families), and the
 * unbind / .cpu() / pad_sequence / H2D round trip between the model and the scorer (README.md:121-126,
 * processing_utils.py:172-178): rows can be written straight into the packed corpus blob msim_fwd streams.
 *   X [M, H] bf16|f16 hidden states (row-major, H a multiple of 64), W [128, H], bias [128] or NULL (same dtype)
 *   row_map int32, ceil(M / 256) * 256 entries (the padding is never dereferenced for rows >= M but must be readable):
 *       v >= 0   write the normalised row m to out row v
 *       v == -1  drop row m (masked position of an unpadded corpus)
 *       v <= -2  write a row of (signed) zeros to out row -2 - v   (masked position kept in place: the dense model output)
 *   out [rows, ld_out] same dtype as X, ld_out >= 128 elements.
 */
int msim_embed_head(int dtype, const void *X, int64_t M, int H,
                    const void *W, const void *bias, int n_out,
                    const int32_t *row_map, void *out, int64_t ld_out, void *stream);

/*
 * Row map of the DENSE form of msim_embed_head (the model forward's own output layout): row m keeps its place,
 *   row_map[m] = (mask[m] != 0 && (extra == NULL || extra[m] != 0)) ? m : -2 - m,    -1 for the tile padding m in [M, ceil(M / 256) * 256)
 * i.e. `proj * attention_mask.unsqueeze(-1)` (modeling_colpali.py:72) and the optional `proj * image_mask` (:74-77) as one launch in
 * front of the head.  mask / extra: [M] elements of `kind` 0 = 1-byte (bool / uint8 / int8), 1 = int16, 2 = int32, 3 = int64, 4 = fp32,
 * 5 = bf16, 6 = fp16 (a floating zero of either sign counts as masked); row_map: int32 [ceil(M / 256) * 256].
 */
int msim_embed_head_row_map(const void *mask, int mask_kind, const void *extra, int extra_kind, int64_t M, int32_t *row_map, void *stream);

/*
 * Row map of the PACKING form of msim_embed_head (pages written back to back into the resident corpus, masked positions dropped:
 * what replaces README.md:121-126 `torch.unbind(embeddings.to("cpu"))` + the scorer's per-block pad_sequence):
 *   row_map[b * S + s] = keep(b, s) ? *rows_before + (kept positions of pages < b) + (kept positions of page b before s) : -1
 *   counts[b] = kept positions of page b (int64, device);  *rows_after = *rows_before + sum of counts;  tile padding of the map = -1.
 * mask / extra as in msim_embed_head_row_map, [B * S] elements; rows_before / rows_after: device int64; they must NOT alias (the page workgroups read *rows_before while another one writes *rows_after).
 */
int msim_embed_head_writer_map(const void *mask, int mask_kind, const void *extra, int extra_kind, int B, int S, const int64_t *rows_before,
                               int64_t *counts, int32_t *row_map, int64_t *rows_after, void *stream);

/*
 * Backward of the norm / mask tail of the embedding head -- what torch autograd derives for
 *   colpali_engine/models/paligemma/colpali/modeling_colpali.py:70  proj = proj / proj.norm(dim=-1, keepdim=True)
 *                                                                :72  proj = proj * attention_mask.unsqueeze(-1)      (+ :74-77)
 * with respect to the nn.Linear output (:67), for a model whose head runs inside the training graph
 * (trainer/contrastive_trainer.py:135-162 back-propagates through it):
 *   dproj[m, :] = row_map[m] >= 0 ? (g[m, :] - y <g[m, :], y>) / n : 0,    y = proj[m, :] / n,    n = ||proj[m, :]|| rounded to dtype
 *   proj [M, 128] = the Linear output, grad_out [M, 128] = the upstream gradient, dproj [M, 128]: dense rows, dtype bf16 | f16;
 *   row_map as in msim_embed_head (>= 0: the position was kept; < 0: masked, gradient exactly 0).
 * The GEMMs on either side (proj itself; dX = dproj W, dW = dproj^T X, db = sum dproj) are plain library GEMMs, left to the host.
 */
int msim_embed_head_bwd(int dtype, const void *proj, const void *grad_out, const int32_t *row_map, int64_t M, int n_out,
                        void *dproj, void *stream);

/*
 * The embedding head at width 320 (ColQwen3: nn.Linear(hidden, 320), the same three lines behind it): msim_embed_head with
 * n_out = 320, a kernel of its own.  Same rounding chain, same row map (built by msim_embed_head_row_map / _writer_map, which do
 * not depend on the width).
 *   X [M, H] bf16|f16 (H a multiple of 64, <= 4096), W [320, H], bias [320] or NULL (same dtype); X, W and out 16-byte aligned
 *   out [rows, ld_out] same dtype as X, ld_out >= 320 elements and a multiple of 8 (whole 8-byte stores: one store form only).
 * msim_embed_head_wide_bwd: msim_embed_head_bwd for proj, grad_out, dproj of [M, 320] (dense rows, 16-byte aligned).
 * MSIM_EUNSUPPORTED for n_out != 320 (msim_embed_head / msim_embed_head_bwd take 128), other dtypes, H % 64 != 0 or H > 4096, and
 * more rows than an int32 row map addresses; MSIM_EINVAL for null pointers, negative sizes, misaligned buffers and a bad ld_out.
 */
int msim_embed_head_wide(int dtype, const void *X, int64_t M, int H, const void *W, const void *bias, int n_out,
                         const int32_t *row_map, void *out, int64_t ld_out, void *stream);
int msim_embed_head_wide_bwd(int dtype, const void *proj, const void *grad_out, const int32_t *row_map, int64_t M, int n_out,
                             void *dproj, void *stream);

/*
 * Plain similarity matrix, no reduction:   out[i, j] = <A[i, :], B[j, :]>   (fp32 accumulate)
 * Replaces colpali_engine/utils/processing_utils.py:126  torch.einsum("bd,cd->bc", qs, ps)   (score_single_vector, the
 * bi-encoder scorer of the same processor class) and the contraction of
 * colpali_engine/interpretability/similarity_map_utils.py:50  torch.einsum("nk,ijk->nij", query, image_grid).
 *   A [n_a, dim], B [n_b, dim] (bf16 | f16 | f32, rows a multiple of 32 bytes, <= 4096), out fp32 [n_a, ld_out].
 *   MSIM_FLAG_REF_ROUNDING: round every dot product to the input dtype (what torch stores for 16-bit inputs).
 */
int msim_sim_matrix(int dtype, const void *A, int n_a, const void *B, int n_b, int dim,
                    float *out, int64_t ld_out, uint32_t flags, void *stream);

/*
 * Hierarchical token pooling (Ward clustering of a page's patch embeddings, mean-pooling every cluster):
 * replaces colpali_engine/compression/token_pooling/hierarchical_token_pooling.py:83-146, i.e. torch.mm + SciPy's
 * linkage(method="ward") on the rows of 1 - E E^T + fcluster(criterion="maxclust") + the per-cluster mean / normalize,
 * which the reference runs page by page on the CPU.
 *
 * msim_pool_cluster: labels[r0 + i] = 0-based flat cluster of row i of page c (r0 = d_off[c]), numbered as SciPy numbers
 *   them; n_clusters[c] = number of clusters (<= max(n_c / pool_factor, 1)).
 *   E [rows, dim] packed pages (bf16 | f16 | f32, rows a multiple of 32 bytes), d_off int32 [n_pages + 1];
 *   max_rows >= the longest page (<= 32768; pages of at most 2048 rows keep the clustering state in LDS, longer ones in their own
 *   region of X_ws, which is dead after the distance pass); ws_off int64 [n_pages + 1] = exclusive prefix sums of n_c * n_c (element offsets
 *   of page c in both workspaces); X_ws fp32 and D_ws fp64 each of ws_off[n_pages] elements.
 * msim_pool_reduce: out[out_off[c] + k, :] = normalize(mean of the rows of page c labelled k), k < out_off[c+1] - out_off[c],
 *   in E's dtype; `dim` logical columns, ld_in / ld_out = elements between consecutive rows of E / out.
 */
int msim_pool_cluster(int dtype, const void *E, const int32_t *d_off, int n_pages, int dim, int max_rows,
                      const int64_t *ws_off, int pool_factor, float *X_ws, double *D_ws,
                      int32_t *labels, int32_t *n_clusters, void *stream);
int msim_pool_reduce(int dtype, const void *E, const int32_t *d_off, int n_pages, int dim, int ld_in,
                     const int32_t *labels, const int32_t *out_off, void *out, int ld_out, void *stream);

/*
 * Host-side helper of the drop-in's upload path (no device work): copies n separate host buffers into one destination image,
 *     memcpy(dst + dst_off[i], src[i], nbytes[i])   for i < n,
 * with up to n_threads threads (contiguous runs of buffers of about equal bytes per thread).  The reference hands the scorer a
 * python list of per-page tensors (README.md:121-126) and re-pads it per block with pad_sequence (processing_utils.py:172-178);
 * here the pages are gathered once into a pinned staging buffer and uploaded.  Native because a thousand small memcpy calls
 * issued from python threads fight over the interpreter lock (70 ms stalls in a 10 ms call were measured).
 */
int msim_host_gather(void *dst, const void *const *src, const int64_t *dst_off, const int64_t *nbytes, int64_t n, int n_threads);
/* The same for a BYTE RANGE of the image: buffer i holds image bytes prefix[i] .. prefix[i+1]-1 (prefix: n + 1 non-decreasing numbers);
 * bytes [lo, hi) of the image are copied to dst (dst[0] = image byte lo), cut into equal byte shares over a persistent pool of native
 * threads (no thread is started per call).  The upload path sends the image through a bounded pinned staging buffer chunk by chunk:
 * one call per chunk, nothing per page on the Python side. */
int msim_host_gather_range(void *dst, const void *const *src, const int64_t *prefix, int64_t n, int64_t lo, int64_t hi, int n_threads);
/* The same gather in two calls: `begin` hands the request to a persistent native thread and returns at once, `wait` blocks until it is
 * done and returns its result.  One request in flight per process (a second `begin` before `wait` is MSIM_EINVAL); the buffers must
 * stay valid until `wait` returns.  The upload path gathers chunk k + 1 this way while the calling thread issues chunk k's H2D copy
 * and the MaxSim launches of the passages that have arrived (colpali_amd/corpus.py: upload_image). */
int msim_host_gather_range_begin(void *dst, const void *const *src, const int64_t *prefix, int64_t n, int64_t lo, int64_t hi, int n_threads);
int msim_host_gather_range_wait(void);
/* The library's host threads (the gather pool's workers and the driver thread above, present and future) run on the listed CPUs from
 * now on.  The upload path calls it when the caller's pages turn out to live on another NUMA node than the one the threads sit on
 * (colpali_amd/_lib.py: gather_cpus_for): a memcpy that READS across the socket link is the slower direction. */
int msim_host_threads_affinity(const int32_t *cpus, int n_cpus);

/*
 * Row-wise top-k of a score matrix with the deterministic order
 * (score descending, id ascending).
 *   scores fp32 [n_q, ld]; the candidates of row q are columns 0..n-1
 *   ids    int64 [n_q, ld] or NULL: id of column j (NULL: id = id_base + j)
 *   out_scores fp32 [n_q, k], out_ids int64 [n_q, k]; rows with fewer than k
 *   candidates are padded with (-inf, -1).
 * The reference only exposes top-k through the experimental
 *   colpali_engine/utils/processing_utils.py:189-219 (get_topk_plaid, k=10 default);
 * retrieval users otherwise call torch.topk on score_multi_vector's output.
 * Needs msim_topk_workspace_bytes(n_q, n, k) bytes of scratch.
 */
size_t msim_topk_workspace_bytes(int n_q, int64_t n, int k);
int msim_topk_f32(const float *scores, const int64_t *ids, int n_q, int64_t n, int64_t ld,
                  int k, int64_t id_base,
                  float *out_scores, int64_t *out_ids, void *workspace, void *stream);
/*
 * msim_topk_f32 takes 1 <= k <= 1024 (MSIM_EUNSUPPORTED beyond).  DEEP TOP-K: the same selection for 1 <= k <= MSIM_TOPK_DEEP_MAX_K,
 * for the long lists a cheap first stage hands to a rerank (k <= 1024 is accepted so that the two entries can be compared bit for
 * bit; callers send such a k to msim_topk_f32).  Arguments and result are those of msim_topk_f32:
 *   ids NULL: id = id_base + column; else int64 [n_q, ld], and an entry whose id is negative is no entry;
 *   the order is (score descending, id ascending); -0.0 and +0.0 tie and come back as +0.0; a -inf score with a valid id is an
 *   entry and ranks last, by id; rows with fewer than k entries are padded with (-inf, -1); NaN is outside the contract.
 * The result is a function of the row's (score, id) set only -- not of the launch shape, of n_q or of scheduling -- so lists can be
 * merged across shards and are reproducible bit for bit.  (Two entries with the same score AND the same id are interchangeable.)
 * out_scores / out_ids are contiguous [n_q, k]; rows of scores / ids may start at any 4- / 8-byte aligned address (odd ld).
 * MSIM_EUNSUPPORTED: k > 8192, n >= 2^31.  MSIM_EINVAL: a negative size, k <= 0, a null pointer (scores may be NULL when n == 0),
 * ld < n, scores / out_scores not 4-byte or ids / out_ids not 8-byte aligned, no (or a not 16-byte aligned) workspace when
 * msim_topk_deep_workspace_bytes(n_q, n, k) > 0.  n_q == 0 returns MSIM_OK with nothing launched.  msim_topk_deep_workspace_bytes
 * is 0 for arguments the entry refuses.
 * Asynchronous on `stream`; allocates nothing and reads nothing back.  The launch sequence is fixed by (n_q, n, k, ids == NULL),
 * never by the data, so the call can be captured in a hipGraph; what it counts into the workspace it zeroes itself, on the stream,
 * in every call, so a replay is correct.  Method (colpali_amd/csrc/topk_deep.hip): a radix select on the 32-bit order-preserving
 * image of the score, most significant byte first, finds the key of the k-th entry; ties at that key go to the smallest ids (the
 * select continues into the id, or -- rows split over several workgroups -- an ordered count in column order); the survivors, at
 * most k, are sorted in LDS at 12 B per entry: 96 KiB at k = 8192 of the CU's 160 KiB, which is where the limit comes from.
 */
#define MSIM_TOPK_DEEP_MAX_K 8192
size_t msim_topk_deep_workspace_bytes(int n_q, int64_t n, int k);
int msim_topk_deep_f32(const float *scores, const int64_t *ids, int n_q, int64_t n, int64_t ld, int k, int64_t id_base,
                       float *out_scores, int64_t *out_ids, void *workspace, void *stream);

/*
 * FIXED DIMENSIONAL ENCODINGS (FDE; Dhulipala et al., "MUVERA", NeurIPS 2024): one vector of F values per page and per query whose
 * inner product approximates MaxSim -- a first stage that is one dense GEMM, reranked exactly by msim_fwd_candidates (fde.hip).
 * Configuration: reps R >= 1, k_sim in 1..6 (B = 2^k_sim buckets), d_proj in {8, 16, 32, 64}; F = R * B * d_proj must be a multiple
 * of 256 and at most 65536; bf16 / f16 rows of width 128 (MSIM_EUNSUPPORTED otherwise).  G fp32 [R, k_sim, 128] and S fp32
 * [R, d_proj, 128] (entries +-1) on the device, drawn by the caller.  For rep r:
 *     phi_r(x) = sum_i 2^i [<G[r, i], x> > 0]        psi_r(x) = S[r] x / sqrt(d_proj)
 * Entry (r * B + b) * d_proj + j of an encoding is psi_r(v)[j], where v is
 *     msim_fde_encode_queries: the SUM of the query's tokens with phi_r = b (zeros if none);
 *     msim_fde_encode_docs:    the MEAN of the page's rows with phi_r = b.  An empty bucket with fill_empty = 1 takes the row p whose
 *                              phi_r(p) has the smallest Hamming distance to b (the lowest row index on a tie); with fill_empty = 0,
 *                              and for a page of 0 rows, zeros.
 * Inputs in the packed layout: rows X [n_rows, 128], item i = rows off[i] .. off[i + 1] - 1 (off int32 [n + 1] on the device; an item
 * whose offsets fall outside 0 .. n_rows is written as NaN).  out [n, F] in the input dtype, computed in fp32 and rounded once;
 * deterministic (no float atomics: reruns are bit-identical).  codes: uint8 [n_rows, R] = phi_r of every row, or NULL.
 * Asynchronous on `stream`, no allocation, no host synchronisation: hipGraph-capturable.
 */
int msim_fde_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim,
                         const float *G, const float *S, int reps, int ksim, int dproj, int fill_empty,
                         void *out, uint8_t *codes /* or NULL */, void *stream);
int msim_fde_encode_queries(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t n_rows, int dim,
                            const float *G, const float *S, int reps, int ksim, int dproj,
                            void *out, uint8_t *codes /* or NULL */, void *stream);
/*
 * scores[q, c] = sum_f Fq[q, f] * Fd[c, f] in fp32 (Fq [n_q, F], Fd [n_d, F] contiguous, bf16 | f16, 16-byte aligned; scores fp32
 * [n_q, ld_scores], ld_scores >= n_d).  A streamed MFMA GEMM; a query's scores have the same bits whatever other queries share the
 * call (the summation order depends on F only).  F: a positive multiple of 256, at most 65536.  No workspace.
 */
int msim_fde_scores(int dtype, const void *Fq, int n_q, const void *Fd, int n_d, int F, float *scores, int64_t ld_scores,
                    void *stream);

/*
 * FIXED DIMENSIONAL ENCODINGS AT WIDTH 320 (ColQwen3; fde_wide.hip): the two encoders above for rows X [n_rows, 320], with
 * G fp32 [R, k_sim, 320] and S fp32 [R, d_proj, 320].  The same arithmetic with 128 replaced by 320 -- sign dots in fp32 on the
 * unrounded row values, SUM for queries, MEAN for pages, fill_empty by Hamming distance with the lowest row index on a tie,
 * psi_r(v) = S[r] v / sqrt(d_proj) in fp32, rounded once on store --, the same argument lists, configuration space and refusals
 * (all before any device work), with `dim` required to be 320 (MSIM_EUNSUPPORTED otherwise).  An item whose offsets fall outside
 * 0 .. n_rows or run backwards is written as NaN.  No float atomics: an item's bits do not depend on the other items of the
 * launch or on reruns.  The encodings are scored by msim_fde_scores, which depends on F alone.  Asynchronous on `stream`, no
 * allocation, no host synchronisation: hipGraph-capturable.
 */
int msim_fdew_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim,
                          const float *G, const float *S, int reps, int ksim, int dproj, int fill_empty,
                          void *out, uint8_t *codes /* or NULL */, void *stream);
int msim_fdew_encode_queries(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t n_rows, int dim,
                             const float *G, const float *S, int reps, int ksim, int dproj,
                             void *out, uint8_t *codes /* or NULL */, void *stream);

/*
 * INT8 TOKEN-LEVEL INDEX (int8_index.hip): an int8 copy of a packed corpus, scored token by token on int8 MFMAs -- a first stage
 * for two-stage search that keeps MaxSim's structure, reranked exactly by msim_fwd_candidates.  All arithmetic is IEEE fp32 on the
 * bf16 / f16 values; division is correctly rounded; rint rounds half to even.
 *   Pages (msim_i8_encode_docs): page c with a_c = max |x| over its rows and columns, inv = 127.0f / a_c, per element
 *     d8 = (x == 0) ? 0 : clamp(rint(x * inv), -127, 127), scale sd_c = a_c / 127.0f.  A page with a_c = 0 gets codes 0 and scale
 *     0 (the x == 0 rule is the formula wherever inv is finite; it also fixes the codes of a page whose a_c is so small that inv
 *     overflows to +inf: zeros stay 0, everything else becomes +-127).  Codes int8 [n_rows, 128] at the rows of the input (row r
 *     of the corpus is row r of the codes); scales fp32 [n_d].  A page whose offsets fall outside 0 .. n_rows gets a NaN scale and
 *     no codes.
 *   Queries (msim_i8_encode_queries): every token row i of the flat layout is quantized the same way with its own row max:
 *     codes q8 [n_rows, 128], scales sq [n_rows].
 *   Score (msim_i8_scores): I_ij = sum_k q8_ik d8_jk (exact int32); M_ic = max_j I_ij, then max(M_ic, 0) where clamp0[c] is set;
 *     scores[q, c] = fl32(sd_c * T), T = the SEQUENTIAL fp32 sum in token order of fl32(float(M_ic) * sq_i) (no fused multiply-add).
 *     A page of 0 rows scores -inf; a query of 0 tokens scores 0 against every other page.  A score's bits depend on its query and
 *     page only (not on the batch, the tiling or a rerun).  max_q_tokens: the caller's upper bound on every query's token
 *     count, from which the launch plan gives each query Q = 16 * ceil(max_q_tokens / 16) token slots (rounded up to a multiple of
 *     128 above 128).  A query longer than Q, or with offsets outside 0 .. q_rows, scores NaN; a query within Q but above
 *     max_q_tokens is scored normally.  When a page's offsets fall outside 0 .. d_rows, every page scored by the same wave (a range
 *     of at most 63 consecutive pages) scores NaN.  clamp0: uint8 [n_d] or NULL.  scores fp32 [n_q, ld_scores], ld_scores >= n_d.  No workspace.
 * Width 128 only (MSIM_EINVAL otherwise); bf16 / f16 inputs (MSIM_EUNSUPPORTED otherwise).  Codes 16-byte aligned, offsets,
 * scales and scores 4-byte aligned.  A call with nothing to do returns 0 before it looks at a pointer.  Asynchronous on `stream`,
 * no allocation, no host synchronisation: hipGraph-capturable.
 */
int msim_i8_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim,
                        int8_t *codes, float *scales, void *stream);
int msim_i8_encode_queries(int dtype, const void *Qt, int64_t n_rows, int dim, int8_t *codes, float *scales, void *stream);
int msim_i8_scores(const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                   const int8_t *d8, const float *sd, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                   int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);

/*
 * 1-BIT SIGN INDEX (binary_index.hip; additions to ABI 22): one sign bit per dimension of every corpus row -- 16 bytes per row, 1/16
 * of the bf16 shard -- scored token by token against the UN-binarised query on int8 MFMAs: a first stage for two-stage search,
 * reranked exactly by msim_fwd_candidates (or msim_res_candidates over a residual-compressed shard).
 *   Encode (msim_bin_encode_rows): for a row x of a bf16 / f16 blob of width 128, s_k = -1 where the sign bit of the stored 16-bit
 *     element is set (this includes -0.0 and negative NaNs), +1 otherwise: an integer operation on the sign bit, no arithmetic.
 *     The row is stored as 16 bytes: dimension k is bit (k & 7) of byte (k >> 3), and a set bit means +1 (the residual codec's
 *     little-endian bit string).  codes uint8 [n_rows, 16] in the input's row order.
 *   Queries: quantized by msim_i8_encode_queries, unchanged: q8 int8 [T, 128], sq fp32 [T].
 *   Score (msim_bin_scores): I_ij = sum_k q8_ik s_jk (exact int32, |I| <= 127 * 128); M_ic = max_j I_ij over the rows of page c,
 *     then max(M_ic, 0) where clamp0[c] is set; scores[q, c] = the SEQUENTIAL fp32 sum in token order of fl32(float(M_ic) * sq_i)
 *     (no fused multiply-add).  A page of 0 rows scores -inf; a query of 0 tokens scores 0 against every page that has rows.  A
 *     score's bits depend on its query and page only (not on the batch, the tiling, the page's position or a rerun).  No row that
 *     is not the page's takes part in M_ic -- in particular not the all-(-1) row that zero bits past the end of the codes would
 *     decode to.  max_q_tokens, a query longer than its token slots or with offsets outside 0 .. q_rows (NaN), and a page whose
 *     offsets fall outside 0 .. d_rows (NaN for every page scored by the same wave, a range of at most 63 consecutive pages): as
 *     msim_i8_scores.  clamp0: uint8 [n_d] or NULL.  scores fp32 [n_q, ld_scores], ld_scores >= n_d.  No workspace.
 *     msim_bin_scores_plan writes the launch form msim_bin_scores takes for the same arguments on the current device: plan[0] = NT
 *     (16-token tiles a wave holds), plan[1] = GW (waves that share one page range: 1, 2 or 4), plan[2] = D (chunks read ahead),
 *     plan[3] = pages per wave range (1 .. 63).  A query longer than 16 NT tokens takes ceil(tokens / (16 NT)) passes over its range.
 * Width 128 and bf16 / f16 only (MSIM_EUNSUPPORTED otherwise); a null or misaligned pointer or a negative size is MSIM_EINVAL; both
 * are decided before the device is touched.  Rows and codes 16-byte aligned; scales, offsets and scores 4-byte aligned.  A call with
 * nothing to do returns 0 before it looks at a pointer.  Asynchronous on `stream`, no allocation, no host synchronisation:
 * hipGraph-capturable.
 */
int msim_bin_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes, void *stream);
int msim_bin_scores_plan(int n_q, int max_q_tokens, int n_d, int64_t d_rows, int32_t *plan /* [4] */);
int msim_bin_scores(const int8_t *q8, const float *sq, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                    const uint8_t *codes, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                    int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);

/*
 * FP4 INDEX (fp4_index.hip; additions to ABI 22): every corpus row and every query token as 128 OCP e2m1 values and one power-of-two
 * scale -- 65 bytes per row, half of the int8 index -- scored token by token on the block-scaled MFMA
 * (v_mfma_scale_f32_16x16x128_f8f6f4, one instruction per 16 rows x 16 tokens): a first stage for two-stage search, reranked
 * exactly by msim_fwd_candidates (or msim_res_candidates over a residual-compressed shard).
 *   Row code (msim_f4_encode_rows; pages and query tokens alike): for a row x of a bf16 / f16 blob of width 128, on the stored values
 *     in fp32: a = max_k |x_k|.  If a == 0 every nibble is 0 and the scale byte is 127.  Otherwise e = the smallest integer with
 *     a <= 6 * 2^e, clamped to [-32, 32] (taken from a's exponent and mantissa fields, no logarithm); y_k = min(|x_k| * 2^-e, 6),
 *     the scaling by a power of two being exact; the code is the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0 .. 7), a tie
 *     going to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the nibble is
 *     sign << 3 | code with x's sign bit when the code is not 0, and 0 otherwise (so -0.0 and everything that rounds to 0 store
 *     0).  Dimension k is nibble (k & 1) of byte (k >> 1), the low nibble holding the even k.  The scale byte is e + 127 (E8M0).
 *     codes uint8 [n_rows, 64] and scales uint8 [n_rows] in the input's row order.  NaN elements are unspecified: the codes and
 *     the scale of a row that holds one may be anything (nothing is read or written out of bounds).
 *   Score (msim_f4_scores): with v() the decoded grid value, I_ij = sum_k v(q_ik) v(d_jk) -- a multiple of 1/4 with |I| <= 4608,
 *     exact in fp32 in any order; Z_ij = I_ij * 2^(eq_i + ed_j), exact; M_ic = max_j Z_ij over the rows of page c, then
 *     max(M_ic, 0) where clamp0[c] is set; scores[q, c] = the SEQUENTIAL fp32 sum of M_ic in token order.  A page of 0 rows scores
 *     -inf; a query of 0 tokens scores 0 against every page that has rows.  A score's bits depend on its query and page only (not
 *     on the batch, the tiling, the page's position or a rerun).  No row that is not the page's takes part in M_ic -- in particular
 *     not the zero row that zero bytes past the end of the codes and scales decode to.  One scale per ROW, not per 32-element
 *     block: with different block scales the four block sums of a row would no longer add exactly and the bits would depend on
 *     the hardware's undocumented order.  Scale bytes outside 95 .. 159 never come out of msim_f4_encode_rows; with them Z may
 *     round and the bits are unspecified.  max_q_tokens, a query longer than its token slots or with offsets outside 0 .. q_rows
 *     (NaN), and a page whose offsets fall outside 0 .. d_rows (NaN for every page scored by the same wave, a range of at most 63
 *     consecutive pages): as msim_i8_scores.  clamp0: uint8 [n_d] or NULL.  scores fp32 [n_q, ld_scores], ld_scores >= n_d.  No
 *     workspace.
 *     msim_f4_scores_plan writes the launch form msim_f4_scores takes for the same arguments on the current device: plan[0] = NT
 *     (16-token tiles a wave holds), plan[1] = GW (waves that share one page range: 1, 2 or 4), plan[2] = D (chunks read ahead),
 *     plan[3] = pages per wave range (1 .. 63).  A query longer than 16 NT tokens takes ceil(tokens / (16 NT)) passes over its range.
 *     The plan describes both scorers: msim_f4_scores_q6 takes the same launch form for the same arguments.
 *   E2M3 QUERY TOKENS (msim_f6_encode_rows, msim_f4_scores_q6; additions to ABI 22): the pages stay FP4, the query tokens are coded
 *   as OCP e2m3 (FP6), which the same instruction takes as its B operand at the FP4 rate.  The stored index is the same index.
 *   Query row code (msim_f6_encode_rows; bf16 / f16, width 128; NaN elements unspecified, as above): a = max_k |x_k|.  If a == 0
 *     every field is 0 and the scale byte is 127.  Otherwise e = the smallest integer with a <= 7.5 * 2^e, clamped to [-32, 32],
 *     read from a's exponent and mantissa fields: a = m * 2^E (1 <= m < 2) gives e = E - 2 + (m > 1.875).  y_k = min(|x_k| * 2^-e,
 *     7.5); the code is the nearest of the 32 e2m3 magnitudes -- codes 0 .. 7 the subnormals i/8, code 8 (j + 1) + i the normal
 *     (1 + i/8) * 2^j for j = 0 .. 2, i = 0 .. 7 -- a tie going to the even code.  The 6-bit field is sign << 5 | code, and 0 when
 *     the code is 0 (so -0.0 and everything that rounds to 0 store 0).  Scale byte = e + 127.  A token is 96 code bytes and 1 scale
 *     byte: dimension k is the 6-bit field at bit 6 (k mod 32) of the little-endian 24-byte group k / 32.  codes uint8
 *     [n_rows, 96], scales uint8 [n_rows].
 *   Score (msim_f4_scores_q6): as msim_f4_scores with v(q) a multiple of 1/8: I_ij is a multiple of 1/16 with
 *     |I| <= 128 * 7.5 * 6 = 5760 (92 160 sixteenths, below 2^24: exact in fp32 in any order); Z, M, clamp0, the sequential sum, the
 *     0-row page (-inf), the 0-token query (0), broken offsets (NaN) and every argument but q6 [q_rows, 96] as msim_f4_scores.
 * Width 128 and bf16 / f16 only (MSIM_EUNSUPPORTED otherwise); a null or misaligned pointer or a negative size is MSIM_EINVAL; both
 * are decided before the device is touched.  Rows and codes 16-byte aligned; offsets and scores 4-byte aligned; scale bytes
 * unaligned.  A call with nothing to do returns 0 before it looks at a pointer.  Asynchronous on `stream`, no allocation, no host
 * synchronisation: hipGraph-capturable.
 */
int msim_f4_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes, uint8_t *scales, void *stream);
int msim_f4_scores_plan(int n_q, int max_q_tokens, int n_d, int64_t d_rows, int32_t *plan /* [4] */);
int msim_f4_scores(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                   const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                   int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);
int msim_f6_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes /* [n_rows, 96] */, uint8_t *scales,
                        void *stream);
int msim_f4_scores_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                      const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                      int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);

/*
 * FP4 CANDIDATES (fp4_candidates.hip; additions to ABI 22): the LIST form of msim_f4_scores / msim_f4_scores_q6 -- the FP4 score of
 * the pages a candidate list names and of no other, the middle stage of a three-stage search: a cheap stage 1 makes a long list, the
 * 65-byte FP4 rows cut it, msim_fwd_candidates (or msim_res_candidates) orders the survivors exactly.
 *   cand int64 [n_q, m] GLOBAL ids with row stride ld_cand >= m; the index holds pages id_base .. id_base + n_d - 1.  Queries, index
 *   and every other argument as msim_f4_scores (msim_f4_candidates_q6: q6 [q_rows, 96] as msim_f4_scores_q6).
 *   out_scores[q, j] (fp32 [n_q, ld_scores], ld_scores >= m) has EXACTLY the bits msim_f4_scores (for _q6: msim_f4_scores_q6) writes
 *     at [q, cand[q, j] - id_base] for the same coded queries and index: a score's bits depend on its query and page only.
 *   out_ids[q, j] (int64 [n_q, ld_scores], or NULL) = cand[q, j].
 *   An id of -1, or outside [id_base, id_base + n_d), is written as (-inf, -1) and reads nothing.  A page of 0 rows scores -inf.  A
 *     query of 0 tokens scores 0 against every page that has rows.  A duplicate id is scored once per occurrence.
 *   Every index is checked before it becomes an address.  A page whose offsets break 0 <= d_off[c] <= d_off[c + 1] <= d_rows scores
 *     NaN, and so does a page longer than msim_f4_scores' range limit of 2^23 rows; a query whose offsets break 0 <= q_off[q] <=
 *     q_off[q + 1] <= q_rows, or that holds more tokens than the launch has slots for (16 * plan[0], at most 128), scores NaN against
 *     every page that has rows.  In each case only the affected entries become NaN; nothing is left unwritten.  Base addresses are
 *     formed in 64 bits: the code array may exceed 2 GiB.
 *   max_q_tokens (0 .. 128): the caller's bound on a query's token count; it chooses the 16-token tiles a wave holds, so a 32-token
 *     query does not pay for eight.  One wave scores one entry, four waves a workgroup, one workgroup per four consecutive entries.
 *     msim_f4_candidates_plan writes that launch form: plan[0] = NT (tiles a wave holds: 1, 2, 4 or 8), plan[1] = D (16-row chunks
 *     read ahead), plan[2] = waves per workgroup, plan[3] = workgroups.  It touches no device.
 * No workspace, no allocation, no host read of the list, no synchronisation: hipGraph-capturable, and the list may be rewritten on
 * the device between replays.  MSIM_EINVAL: a negative size, a null or misaligned pointer (codes 16-byte, ids 8-byte, offsets and
 * scores 4-byte aligned; scale bytes unaligned), ld_cand < m or ld_scores < m.  MSIM_EUNSUPPORTED: dim != 128, max_q_tokens > 128,
 * more workgroups than one launch holds (ceil(n_q m / 4) >= 2^31).  n_q == 0 or m == 0: MSIM_OK before a pointer is looked at,
 * nothing launched.  All of it is decided before the device is touched.
 */
int msim_f4_candidates_plan(int n_q, int max_q_tokens, int m, int32_t *plan /* [4]: NT, D, waves per workgroup, workgroups */);
int msim_f4_candidates(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                       const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                       int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores,
                       int64_t ld_scores, int64_t *out_ids /* or NULL */, void *stream);
int msim_f4_candidates_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                          const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                          int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores,
                          int64_t ld_scores, int64_t *out_ids /* or NULL */, void *stream);

/*
 * FP4 INDEX AT WIDTH 320 (fp4_wide_index.hip; additions to ABI 22): the FP4 index for 320-wide (ColQwen3) shards, a sibling of
 * msim_f4_* as msim_fwd_candidates_wide is of msim_fwd_candidates.  Every corpus row and every query token is 320 OCP e2m1 values and
 * ONE power-of-two scale -- 161 bytes per row instead of 640.  A 320-wide row is 2 1/2 K blocks of
 * v_mfma_scale_f32_16x16x128_f8f6f4: 16 rows x 16 tokens take three instructions, chained through the C operand, the third with
 * half of its K block empty.  A first stage for two-stage search, reranked exactly by msim_fwd_candidates_wide.
 *   Row code (msim_f4w_encode_rows; pages and query tokens alike): msim_f4_encode_rows' rule over 320 dimensions, for a row x of a
 *     bf16 / f16 blob of width 320, on the stored values in fp32: a = max over all 320 |x_k|.  If a == 0 every nibble is 0 and the
 *     scale byte is 127.  Otherwise e = the smallest integer with a <= 6 * 2^e, clamped to [-32, 32] (taken from a's exponent and
 *     mantissa fields); y_k = min(|x_k| * 2^-e, 6); the code is the nearest of {0, 0.5, 1, 1.5, 2, 3, 4, 6} (codes 0 .. 7), a tie
 *     going to the even code; the nibble is sign << 3 | code with x's sign bit when the code is not 0, and 0 otherwise.  Dimension k
 *     is nibble (k & 1) of byte (k >> 1) of a 160-byte row, the low nibble holding the even k.  The scale byte is e + 127 (E8M0).
 *     codes uint8 [n_rows, 160] and scales uint8 [n_rows] in the input's row order.  NaN elements are unspecified, as above.
 *   Score (msim_f4w_scores): as msim_f4_scores.  I_ij = sum_{k<320} v(q_ik) v(d_jk) -- a multiple of 1/4 with
 *     |I| <= 320 * 36 = 11 520 (46 080 quarters, below 2^24), and so is every partial sum: exact in fp32 in any order, which one
 *     scale per ROW keeps true across the three K blocks; Z_ij = I_ij * 2^(eq_i + ed_j), exact; M_ic = max_j Z_ij over the rows of
 *     page c, then max(M_ic, 0) where clamp0[c] is set; scores[q, c] = the SEQUENTIAL fp32 sum of M_ic in token order.  A page of 0
 *     rows scores -inf; a query of 0 tokens scores 0 against every page that has rows.  A score's bits depend on its query and page
 *     only.  No row that is not the page's takes part in M_ic.  Scale bytes outside 95 .. 159: unspecified bits, as above.
 *     max_q_tokens, a query longer than its token slots or with offsets outside 0 .. q_rows (NaN over that query), and a page whose
 *     offsets fall outside 0 .. d_rows (NaN for every page scored by the same wave, a range of at most 63 consecutive pages): as
 *     msim_f4_scores.  A wave's range holds at most 2^23 rows, which keeps every 32-bit buffer offset below 2^31 at 160 bytes per
 *     row (a longer range is written as NaN).  clamp0: uint8 [n_d] or NULL.  scores fp32 [n_q, ld_scores], ld_scores >= n_d.  No
 *     workspace.
 *     msim_f4w_scores_plan writes the launch form msim_f4w_scores takes for the same arguments on the current device: plan[0] = NT
 *     (16-token tiles a wave holds), plan[1] = GW (waves that share one page range: 1, 2 or 4), plan[2] = D (chunks read ahead),
 *     plan[3] = pages per wave range (1 .. 63).  A query longer than 16 NT tokens takes ceil(tokens / (16 NT)) passes over its range.
 *     The plan describes both scorers: msim_f4w_scores_q6 takes the same launch form for the same arguments.
 *   E2M3 QUERY TOKENS (fp6_wide_query.hip: msim_f6w_encode_rows, msim_f4w_scores_q6; additions to ABI 22): the pages stay FP4, the
 *   query tokens are coded as OCP e2m3 (FP6), which the same instruction takes as its B operand.  The stored index is the same index.
 *   Query row code (msim_f6w_encode_rows; bf16 / f16, width 320; NaN elements unspecified, as above): msim_f6_encode_rows' rule
 *     over 320 dimensions.  a = max over all 320 |x_k|.  If a == 0 every field is 0 and the scale byte is 127.  Otherwise e = the
 *     smallest integer with a <= 7.5 * 2^e, clamped to [-32, 32], read from a's exponent and mantissa fields: a = m * 2^E
 *     (1 <= m < 2) gives e = E - 2 + (m > 1.875).  y_k = min(|x_k| * 2^-e, 7.5); the code is the nearest of the 32 e2m3 magnitudes
 *     -- codes 0 .. 7 the subnormals i/8, code 8 (j + 1) + i the normal (1 + i/8) * 2^j for j = 0 .. 2, i = 0 .. 7 -- a tie going
 *     to the even code.  The 6-bit field is sign << 5 | code, and 0 when the code is 0 (so -0.0 and everything that rounds to 0
 *     store 0).  Scale byte = e + 127.  A token is 240 code bytes and 1 scale byte: dimension k is the 6-bit field at bit 6 k of the
 *     little-endian row.  codes uint8 [n_rows, 240], scales uint8 [n_rows].
 *     As operands, for lane group l4 = lane >> 4: K blocks 0 and 1 (b = 0, 1) take the lane's 24 bytes at byte 96 b + 24 l4,
 *     dimensions 128 b + 32 l4 .. + 31, the partners of the 16 FP4 bytes the page side holds there; K block 2 takes the lane's 12
 *     bytes at byte 192 + 12 l4, dimensions 256 + 16 l4 .. + 15, as fields 0 .. 15 of the operand with registers 3 .. 5 zero, the
 *     partners of the page side's 8 bytes (nibbles 0 .. 15).
 *   Score (msim_f4w_scores_q6): as msim_f4w_scores with v(q) a multiple of 1/8: I_ij is a multiple of 1/16 with
 *     |I| <= 320 * 7.5 * 6 = 14 400 (230 400 sixteenths, below 2^24), and so is every partial sum through the chained C operand:
 *     exact in fp32 in any order; Z, M, clamp0, the sequential sum in token order, the 0-row page (-inf), the 0-token query (0),
 *     broken offsets (NaN), the range limit and every argument but q6 [q_rows, 240] as msim_f4w_scores.
 * Width 320 and bf16 / f16 only (MSIM_EUNSUPPORTED otherwise -- width 128 is msim_f4_*'s, which refuses 320 in turn); a null or
 * misaligned pointer or a negative size is MSIM_EINVAL; both are decided before the device is touched.  Rows and codes 16-byte
 * aligned; offsets and scores 4-byte aligned; scale bytes unaligned.  A call with nothing to do returns 0 before it looks at a
 * pointer.  Asynchronous on `stream`, no allocation, no host synchronisation: hipGraph-capturable.
 */
int msim_f4w_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes /* [n_rows, 160] */, uint8_t *scales,
                         void *stream);
int msim_f4w_scores_plan(int n_q, int max_q_tokens, int n_d, int64_t d_rows, int32_t *plan /* [4] */);
int msim_f4w_scores(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                    const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                    int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);
int msim_f6w_encode_rows(int dtype, const void *X, int64_t n_rows, int dim, uint8_t *codes /* [n_rows, 240] */, uint8_t *scales,
                         void *stream);
int msim_f4w_scores_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                       const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                       int64_t d_rows, int dim, float *scores, int64_t ld_scores, void *stream);

/*
 * FP4 CANDIDATES AT WIDTH 320 (fp4_wide_candidates.hip; additions to ABI 22): the LIST form of msim_f4w_scores -- the FP4 score of
 * the pages a candidate list names and of no other, the middle stage of a three-stage search on a 320-wide shard: a cheap stage 1
 * makes a long list, the 161-byte FP4 rows cut it, msim_fwd_candidates_wide orders the survivors exactly.  The sibling of
 * msim_f4_candidates, argument for argument.
 *   cand int64 [n_q, m] GLOBAL ids with row stride ld_cand >= m; the index holds pages id_base .. id_base + n_d - 1.  Queries, index
 *   and every other argument as msim_f4w_scores.
 *   out_scores[q, j] (fp32 [n_q, ld_scores], ld_scores >= m) has EXACTLY the bits msim_f4w_scores writes at
 *     [q, cand[q, j] - id_base] for the same coded queries and index: every partial sum is exact in fp32, the maxima are taken over
 *     the page's own rows only and the sum runs in token order from 0.0f, so a score's bits depend on its query and page only.
 *   out_ids[q, j] (int64 [n_q, ld_scores], or NULL) = cand[q, j].
 *   Order of resolution per entry: an id of -1, or outside [id_base, id_base + n_d), is written as (-inf, -1) and reads nothing; a
 *     page whose offsets break 0 <= d_off[c] <= d_off[c + 1] <= d_rows, or that is longer than msim_f4w_scores' range limit of 2^23
 *     rows, scores NaN; a page of 0 rows scores -inf; a query whose offsets break 0 <= q_off[q] <= q_off[q + 1] <= q_rows, or that
 *     holds more tokens than the launch has slots for (16 * plan[0], at most 128), scores NaN; a query of 0 tokens scores 0.  A
 *     duplicate id is scored once per occurrence.  Every index is checked before it becomes an address; only the affected entries
 *     become NaN; nothing is left unwritten.  Base addresses are formed in 64 bits: the code array may exceed 2 GiB.
 *   max_q_tokens (0 .. 128): the caller's bound on a query's token count; it chooses the 16-token tiles a wave holds.  One wave
 *     scores one entry, four waves a workgroup, one workgroup per four consecutive entries.  msim_f4w_candidates_plan writes that
 *     launch form: plan[0] = NT (tiles a wave holds: 1, 2, 4 or 8), plan[1] = D (16-row chunks read ahead), plan[2] = waves per
 *     workgroup, plan[3] = workgroups.  It touches no device.
 * No workspace, no allocation, no host read of the list, no synchronisation: hipGraph-capturable, and the list may be rewritten on
 * the device between replays.  MSIM_EINVAL: a negative size, a null or misaligned pointer (codes 16-byte, ids 8-byte, offsets and
 * scores 4-byte aligned; scale bytes unaligned), ld_cand < m or ld_scores < m.  MSIM_EUNSUPPORTED: dim != 320 (width 128 is
 * msim_f4_candidates', which refuses 320 in turn), max_q_tokens > 128, more workgroups than one launch holds
 * (ceil(n_q m / 4) >= 2^31).  n_q == 0 or m == 0: MSIM_OK before a pointer is looked at, nothing launched.  All of it is decided
 * before the device is touched.
 *   msim_f4w_candidates_q6 (fp6_wide_candidates.hip; an addition to ABI 22) is the list form of msim_f4w_scores_q6: q6
 *     [q_rows, 240] e2m3 fields from msim_f6w_encode_rows, every other argument, every check, refusal and result as
 *     msim_f4w_candidates, and out_scores[q, j] has EXACTLY the bits msim_f4w_scores_q6 writes at [q, cand[q, j] - id_base].  It takes
 *     the same launch form for the same arguments: msim_f4w_candidates_plan describes both.
 */
int msim_f4w_candidates_plan(int n_q, int max_q_tokens, int m, int32_t *plan /* [4]: NT, D, waves per workgroup, workgroups */);
int msim_f4w_candidates(const uint8_t *q4, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                        const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                        int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores,
                        int64_t ld_scores, int64_t *out_ids /* or NULL */, void *stream);
int msim_f4w_candidates_q6(const uint8_t *q6, const uint8_t *qs, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                           const uint8_t *d4, const uint8_t *ds, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d,
                           int64_t d_rows, int dim, const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores,
                           int64_t ld_scores, int64_t *out_ids /* or NULL */, void *stream);

/*
 * CENTROID-CODE INDEX (centroid_index.hip; additions to ABI 22): every corpus row stored as the uint16 id of its nearest of K
 * centroids, pages scored by centroid interaction (PLAID's first stage) -- a first stage for two-stage search that reads 2 bytes
 * per row, reranked exactly by msim_fwd_candidates.  C: K centroid rows [K, 128] in the dtype of the rows they meet; K a multiple
 * of 256, 256 <= K <= 2048 (the fp16 table of 32 query tokens, K x 64 B, has to fit the 160 KiB LDS).
 *   Encode (msim_cent_encode_docs): code[r] = argmax_k <row_r, C_k>, each dot product one fp32-accumulated MFMA chain (products
 *     exact, k ascending in steps of 32); on equal fp32 values the lowest k wins.  codes uint16 [n_rows] in the corpus's row order
 *     (row r of the input is entry r of the codes).  max_doc_rows: the caller's upper bound on a page's row count.  A page whose
 *     offsets fall outside 0 .. n_rows, or that is longer than max_doc_rows, gets no codes and status[c] = 1 (every other page:
 *     0); status int32 [n_d] or NULL.
 *   Table (msim_cent_table): S[i, k] = fp16(fl32 <q_i, C_k>) (the same chain, rounded to nearest even once) for every token of the
 *     flat layout, written to table as [n_q * nb][K][32] fp16, nb = max(1, ceil(max_q_tokens / 32)): block b of query q holds its
 *     tokens 32 b .. 32 b + 31, 0 where the query has no such token (and everywhere for a query whose offsets fall outside
 *     0 .. q_rows or that is longer than 32 nb).  msim_cent_table_bytes(n_q, max_q_tokens, K) = n_q * nb * K * 64.  A table's bits
 *     depend on its query and the centroids only.
 *   Score (msim_cent_scores): M_i = max_j S[i, code_j] over the page's rows j (an exact maximum of fp16 values), max(M_i, 0)
 *     where clamp0[c] is set; scores[q, c] = the SEQUENTIAL fp32 sum in token order of float(M_i), carried across the 32-token
 *     blocks.  A page of 0 rows scores -inf, flagged or not; a query of 0 tokens scores 0 against every page that has rows.  A
 *     page with a code >= K, or whose offsets fall outside 0 .. d_rows, scores NaN (the code is checked before it becomes an
 *     address; other pages are not affected); so does every page against a query whose offsets fall outside 0 .. q_rows or that
 *     is longer than 32 nb.  A score's bits depend on its query, the centroids and the page's codes only -- not on the batch,
 *     the page's position, the launch plan or a rerun; no float atomics.  table and max_q_tokens: as passed to msim_cent_table.
 *     clamp0: uint8 [n_d] or NULL.  scores fp32 [n_q, ld_scores], ld_scores >= n_d.  d_rows <= 2^31 - 1025.  No workspace.
 *     msim_cent_scores_plan writes the launch plan of the same arguments: plan[0] = nb, plan[1] = pages per wave (1 .. 64),
 *     plan[2] = waves per workgroup, plan[3] = workgroups (a workgroup scores one query against plan[1] * plan[2] consecutive
 *     pages).
 * Width 128, bf16 / f16 and max_q_tokens <= 128 only (MSIM_EUNSUPPORTED otherwise); K outside the rule is MSIM_EINVAL.  Rows,
 * centroids, table and codes 16-byte aligned; offsets, status and scores 4-byte aligned.  A call with nothing to do (n_d == 0,
 * n_q == 0, max_doc_rows == 0) returns 0 before it looks at a pointer.  Asynchronous on `stream`, no allocation, no host
 * synchronisation: hipGraph-capturable.
 */
int msim_cent_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows,
                          const void *C, int K, uint16_t *codes, int32_t *status /* or NULL */, void *stream);
size_t msim_cent_table_bytes(int n_q, int max_q_tokens, int K);
int msim_cent_table(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int dim,
                    const void *C, int K, void *table, void *stream);
int msim_cent_scores_plan(int n_q, int max_q_tokens, int K, int n_d, int64_t d_rows, int32_t *plan /* [4] */);
int msim_cent_scores(const void *table, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int K,
                     const uint16_t *codes, const int32_t *d_off, const uint8_t *clamp0 /* or NULL */, int n_d, int64_t d_rows,
                     float *scores, int64_t ld_scores, void *stream);

/*
 * RESIDUAL-COMPRESSED CORPUS (residual_codec.hip; additions to ABI 22): PLAID's second half.  Every corpus row is its centroid code
 * (msim_cent_encode_docs) plus `bits` of residual per dimension, and candidate lists are reranked from those rows alone: no
 * full-precision embedding is kept.  Width 128, bf16 / f16, bits 2 or 4, K as for the centroid index (MSIM_EUNSUPPORTED / MSIM_EINVAL
 * as there).  34 / 66 bytes per row instead of 256.
 *   Code.  For row x with code c: e_k = fl32(float(x_k) - float(C[c]_k)), one fp32 subtraction per dimension; the bucket b_k is the
 *     number of cutoffs t with t <= e_k (a value equal to a cutoff goes to the upper bucket).  cutoffs: fp32 [2^bits - 1],
 *     non-decreasing.
 *   Packing.  residuals: uint8 [rows, 16 * bits]; dimension k occupies bits [k * bits, k * bits + bits) of its row read as a
 *     little-endian bit string (bit i = bit i % 8 of byte i / 8).  Rows are 32 / 64 bytes and 16-byte aligned; the 8 consecutive k
 *     one lane feeds an MFMA are one 16- / 32-bit little-endian field.
 *   Decode.  xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k]): one fp32 addition, ONE rounding to nearest even to the corpus
 *     dtype, and no renormalisation (ColBERTv2's Python path renormalises the decoded row; PLAID's kernels do not, and neither does
 *     this).  weights: fp32 [2^bits].
 * msim_res_encode_docs: rows D [n_rows, 128] and their codes -> residuals, one pass (a row is read once; its centroid row comes
 *   through L2).  A row whose code is >= K is written as all-zero buckets and its code stays as it is, so its page scores NaN below,
 *   as in msim_cent_scores: such a code never becomes an address.
 * msim_res_decode_rows: xhat of rows row0 .. row1 - 1 (0 <= row0 <= row1 <= n_rows) -> out [row1 - row0, 128] in the corpus dtype;
 *   rows outside the range are not touched.  A row whose code is >= K decodes to NaN.
 * msim_res_candidates: msim_fwd_candidates' contract over the compressed rows -- cand [n_q, m] int64 GLOBAL ids with row stride
 *   ld_cand >= m, page c has id id_base + c; an id of -1 or outside [id_base, id_base + n_d) is (-inf, -1) and reads nothing; a
 *   query of 0 tokens scores 0; queries of 0 .. 128 tokens in the flat layout (MSIM_EUNSUPPORTED beyond); d_clamp0 as msim_fwd; a
 *   duplicate id is scored once per occurrence.  out_scores[q, j] has exactly the bits msim_fwd_candidates (flags 0) gives the same
 *   query against the page decoded by msim_res_decode_rows: the same fp32 MFMA chain over the four 32-wide k steps with the same
 *   k-to-lane mapping, an exact maximum over the page's rows, the same token sum.  The page is decoded slab by slab in registers
 *   into LDS and never written to memory.  A page with a code >= K, or whose offsets fall outside 0 <= d_off[c] <= d_off[c + 1] <=
 *   d_rows, scores NaN (checked before anything becomes an address; other pages are not affected); a device q_off that disagrees
 *   with q_off_host makes every score of the call NaN.  One wave scores one entry.
 *   workspace: msim_res_candidates_workspace_bytes(n_q, m, n_d) bytes (0 when there is no entry), 16-byte aligned, initialised by
 *   the call (by a kernel); it does not depend on the number of rows.  After the call its first int32 is 0, or 1 for a broken q_off.
 * msim_res_scores: the FULL SCAN of the compressed shard (residual_scan.hip) -- out_scores[q, c] for every query q and every page c,
 *   row stride ld_scores >= n_d (columns >= n_d of a wider matrix are not written).  Bit identity: entry (q, c) has exactly the
 *   bits msim_fwd_ragged (flags 0) gives the same query against the page decoded by msim_res_decode_rows: the same fp32 MFMA chain
 *   over the four 32-wide k steps with the same k-to-lane mapping, an exact maximum over the page's rows, the same token sum (a
 *   pure function of the token values and the query's length, so the bits do not depend on which queries share a wave).  A wave
 *   holds a group of consecutive queries (at most 8 queries and 8 units of 16 tokens) and decodes a page once per group, not once
 *   per query.  Formats as msim_res_candidates: bf16 / f16, width 128, bits 2 or 4, K a multiple of 256 in 256 .. 2048, queries
 *   of 0 .. 128 tokens in the flat layout (MSIM_EUNSUPPORTED beyond), d_clamp0 as msim_fwd.  A query of 0 tokens scores 0; a page
 *   of 0 rows scores what the scan of the decompressed page gives (-inf, or 0 when flagged).  A page with a code >= K, or whose
 *   offsets fall outside 0 <= d_off[c] <= d_off[c + 1] <= d_rows, scores NaN in its column for every query with at least one token
 *   (checked before anything becomes an address; no other column changes); a device q_off that disagrees with q_off_host makes
 *   every score of the call NaN.
 *   workspace: msim_res_scores_workspace_bytes(n_q, n_d) bytes (0 when n_q <= 0 or n_d <= 0), 16-byte aligned, initialised by the
 *   call (by a kernel, not a memset node); a function of n_q alone (status words plus the query-group table), never of the row
 *   count.  After the call its first int32 is 0, or 1 for a broken q_off.
 *   MSIM_EINVAL also for ld_scores < n_d and for a q_off_host that does not start at 0 or decreases.  No float atomics.
 * MSIM_EINVAL for a negative size, a null or misaligned pointer (rows, centroids, residuals, out, workspace: 16 bytes), ld < m.  A
 * call with nothing to do (n_rows == 0, row0 == row1, n_q == 0, m == 0, n_d == 0 for the scan) returns 0 before it looks at a
 * pointer.  Asynchronous on `stream`, no allocation, no host synchronisation: hipGraph-capturable.
 */
int msim_res_encode_docs(int dtype, const void *D, int64_t n_rows, int dim, const uint16_t *codes, const void *C, int K,
                         const float *cutoffs, int bits, uint8_t *residuals, void *stream);
int msim_res_decode_rows(int dtype, const uint16_t *codes, const uint8_t *residuals, int64_t n_rows, int64_t row0, int64_t row1,
                         const void *C, int K, const float *weights, int bits, int dim, void *out, void *stream);
size_t msim_res_candidates_workspace_bytes(int n_q, int m, int n_d);
int msim_res_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                        const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                        const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows, int dim, const int64_t *cand, int m,
                        int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores, int64_t *out_ids /* or NULL */,
                        void *workspace, void *stream);
size_t msim_res_scores_workspace_bytes(int n_q, int n_d);
int msim_res_scores(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                    const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                    const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows, int dim, float *out_scores, int64_t ld_scores,
                    void *workspace, void *stream);

/*
 * THE COMPRESSED SHARD AT WIDTH 320 (ColQwen3; residual_wide.hip, residual_wide_scan.hip; additions to ABI 22): the centroid-code
 * first stage, the residual codec, the candidate rerank and the full scan over rows of 320 dimensions.  The entries above keep refusing dim == 320 (MSIM_EUNSUPPORTED); these take
 * dim == 320 ONLY (anything else, and a dtype other than bf16 / f16: MSIM_EUNSUPPORTED).  K a multiple of 256 in 256 .. 2048
 * (MSIM_EINVAL otherwise), bits 2 or 4 (MSIM_EUNSUPPORTED otherwise), queries of 0 .. 128 tokens (MSIM_EUNSUPPORTED beyond).  A row
 * costs 2 + 80 = 82 bytes at 2 bits and 2 + 160 = 162 at 4, instead of 640.
 * msim_cent_wide_encode_docs: the contract of msim_cent_encode_docs over D [n_rows, 320] and C [K, 320] -- code[r] = argmax_k
 *   <row_r, C_k>, each dot product ONE fp32-accumulated MFMA chain (v_mfma_f32_16x16x32) from zero over the ten 32-wide k steps in
 *   ascending order; the lowest k wins equal values.  max_doc_rows and status (int32 [n_d] or NULL) as there: a page whose offsets
 *   fall outside 0 .. n_rows, or that is longer than max_doc_rows, is skipped and reported 1, nothing of it becomes an address.
 * msim_cent_wide_table: msim_cent_table over Qt [q_rows, 320] -- S[i, k] = fp16(fl32 <q_i, C_k>), the same chain, rounded to nearest
 *   even once -- into the SAME table[n_q * nb][K][32] fp16 layout, msim_cent_table_bytes(n_q, max_q_tokens, K) bytes.  The scan reads
 *   the table and the codes only, so msim_cent_scores, msim_cent_scores_plan and msim_cent_table_bytes serve the wide index unchanged.
 * msim_res_wide_encode_docs / msim_res_wide_decode_rows: the codec above on the 40 chunks of 8 dimensions of a row.
 *   Code.  e_k = fl32(float(x_k) - float(C[c]_k)); the bucket b_k is the number of cutoffs t with t <= e_k.
 *   Packing.  residuals: uint8 [rows, 40 * bits]; dimension k occupies bits [k * bits, k * bits + bits) of its row read as a
 *     little-endian bit string: 80 bytes per row at 2 bits, 160 at 4, 16-byte aligned.
 *   Decode.  xhat_k = round_to_dtype(float(C[c]_k) + weights[b_k]): one fp32 addition, ONE rounding, no renormalisation.
 *   A row whose code is >= K is encoded as all-zero buckets and decodes to the NaN row; such a code never becomes an address.
 *   msim_res_wide_decode_rows writes rows row0 .. row1 - 1 (0 <= row0 <= row1 <= n_rows) -> out [row1 - row0, 320].
 * msim_res_wide_candidates: msim_res_candidates' contract over the wide rows.  out_scores[q, j] has exactly the bits
 *   msim_fwd_candidates_wide (flags 0) gives the same query against the page decoded by msim_res_wide_decode_rows: per (32-row slab,
 *   16-token unit) one fp32 accumulator from zero chained across the panels p = 0, 1, 2 (128 + 128 + 64 dimensions) with the k steps
 *   ascending inside each; rows past the page's end in the last slab are masked to -inf behind the MFMAs, never zero-filled; an exact
 *   maximum over the page's rows; the same token sum.  The page is decoded slab by slab in registers into LDS and never written to
 *   memory.  An id of -1 or outside [id_base, id_base + n_d) is (-inf, -1) and reads nothing; a query of 0 tokens scores 0; a page of
 *   0 rows scores -inf (0 when flagged in d_clamp0); a duplicate id is scored once per occurrence.  A page with a code >= K, or whose
 *   offsets fall outside 0 <= d_off[c] <= d_off[c + 1] <= d_rows, scores NaN (checked before anything becomes an address; other pages
 *   are not affected); a device q_off that disagrees with q_off_host makes every score of the call NaN.  One wave scores one entry.
 *   workspace: msim_res_wide_candidates_workspace_bytes(n_q, m, n_d) bytes (0 when there is no entry), 16-byte aligned, initialised
 *   by the call (by a kernel); it does not depend on the number of rows.  After the call its first int32 is 0, or 1 for a broken q_off.
 * msim_res_wide_scores: the FULL SCAN of the wide compressed shard (residual_wide_scan.hip), msim_res_scores' contract and argument
 *   list over the wide rows -- out_scores[q, c] for every query q and every page c, row stride ld_scores >= n_d (columns >= n_d of a
 *   wider matrix are not written).  Bit identity: entry (q, c) has exactly the bits msim_res_wide_candidates gives the same query
 *   against page c -- that is, the bits msim_fwd_candidates_wide (flags 0), and the flat panel kernel behind msim_fwd_ragged at width
 *   320 (K1bPF), give against the page decoded by msim_res_wide_decode_rows: the same chain, tail mask and exact maximum, and the same
 *   token sum (a pure function of the token values and the query's length, so the bits do not depend on which queries share a wave).
 *   A scan of the decoded pages that the few-query panel kernel serves (ONE query length and at most four 32-token tiles: K1sP) adds
 *   the tokens in another fp32 order: the bound stated for msim_fwd_candidates_wide, |delta| <= 2 gamma(L - 1) sum_i |M_i|, covers
 *   it.  A wave holds a group of consecutive queries (at most 8 queries and 8 units of 16 tokens) in registers and decodes a page
 *   once per group, not once per query.  A query of 0 tokens scores 0; a page of 0 rows scores -inf (0 when flagged in d_clamp0).  A
 *   page with a code >= K, or whose offsets fall outside 0 <= d_off[c] <= d_off[c + 1] <= d_rows, scores NaN in its column for every
 *   query with at least one token (checked before anything becomes an address; no other column changes); a device q_off that
 *   disagrees with q_off_host makes every score of the call NaN.
 *   workspace: msim_res_wide_scores_workspace_bytes(n_q, n_d) bytes (0 when n_q <= 0 or n_d <= 0), 16-byte aligned, initialised by
 *   the call (by a kernel, not a memset node); a function of n_q alone (status words plus the query-group table), never of the row
 *   count.  After the call its first int32 is 0, or 1 for a broken q_off.  MSIM_EINVAL also for ld_scores < n_d; MSIM_EUNSUPPORTED
 *   for d_rows >= 2^31.  n_q == 0 or n_d == 0 is nothing to do.
 * MSIM_EINVAL for a negative size, a null or misaligned pointer (rows, centroids, residuals, out, table, workspace: 16 bytes),
 * ld < m, a q_off_host that does not start at 0 or decreases; MSIM_EUNSUPPORTED for d_rows >= 2^31 in msim_res_wide_candidates.  A
 * call with nothing to do returns 0 before it looks at a pointer.  Every refusal happens before the device is touched.
 * Asynchronous on `stream`, no allocation, no host synchronisation, no float atomics: hipGraph-capturable.
 */
int msim_cent_wide_encode_docs(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows,
                               const void *C, int K, uint16_t *codes, int32_t *status /* or NULL */, void *stream);
int msim_cent_wide_table(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens, int dim,
                         const void *C, int K, void *table, void *stream);
int msim_res_wide_encode_docs(int dtype, const void *D, int64_t n_rows, int dim, const uint16_t *codes, const void *C, int K,
                              const float *cutoffs, int bits, uint8_t *residuals, void *stream);
int msim_res_wide_decode_rows(int dtype, const uint16_t *codes, const uint8_t *residuals, int64_t n_rows, int64_t row0, int64_t row1,
                              const void *C, int K, const float *weights, int bits, int dim, void *out, void *stream);
size_t msim_res_wide_candidates_workspace_bytes(int n_q, int m, int n_d);
int msim_res_wide_candidates(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q,
                             const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights, int bits,
                             const int32_t *d_off, const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows, int dim,
                             const int64_t *cand, int m, int64_t ld_cand, int64_t id_base, float *out_scores, int64_t ld_scores,
                             int64_t *out_ids /* or NULL */, void *workspace, void *stream);
size_t msim_res_wide_scores_workspace_bytes(int n_q, int n_d);
int msim_res_wide_scores(int dtype, const void *Qt, const int32_t *q_off, const int32_t *q_off_host, int n_q, const uint16_t *codes,
                         const uint8_t *residuals, const void *C, int K, const float *weights, int bits, const int32_t *d_off,
                         const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows, int dim, float *out_scores, int64_t ld_scores,
                         void *workspace, void *stream);

/*
 * ROWS OUT OF THE COMPRESSED SHARD (residual_align.hip; additions to ABI 22): the two operations that return rows, decoded inside
 * the kernel that consumes them.  No decoded copy of a listed page is written to memory, and nothing reads the list on the host.
 * Formats as msim_res_candidates: bf16 / f16, width 128, bits 2 or 4, K a multiple of 256 in 256 .. 2048 -- MSIM_EUNSUPPORTED for
 * anything else, K included (these two entry points have no other K to offer).
 * msim_res_align_candidates: msim_align_candidates' contract, conventions, output shapes and return codes over the compressed rows
 *   (codes, residuals, C, K, weights, bits in place of D): cand [n_q, m] GLOBAL ids with row stride ld_cand >= m, queries of 0 ..
 *   128 tokens in the flat layout (max_q_tokens > 128: MSIM_EUNSUPPORTED), best_sim / best_row [n_q, m, max_q_tokens], sims
 *   [n_q, m, max_q_tokens, max_rows] or NULL.  ARITHMETIC: for every entry, best_sim, best_row and sims hold exactly the bits
 *   msim_align_candidates gives the same queries and list over the output of msim_res_decode_rows for the whole shard (rows 0 ..
 *   d_rows), every -inf / 0.0 / NaN / -1 convention included: the operand of the MFMA chain is built by the decode helper
 *   msim_res_decode_rows uses, in the lane layout of K1a, and everything behind the operand is K1a.  A row whose code is >= K is the
 *   NaN row msim_res_decode_rows writes (its similarities are NaN exactly as over the decoded page; the code never becomes an
 *   address; no other row or entry changes).  An entry whose page is longer than max_rows, or whose offsets fall outside 0 <=
 *   d_off[c] <= d_off[c + 1] <= d_rows, is NaN / -1 in full and reads nothing.
 * msim_res_gather_pages: msim_gather_pages' contract over the compressed rows: out [n_slots, pad_rows, 128] in the corpus dtype
 *   holds exactly the bytes msim_gather_pages (row_bytes 256) gives the same ids over that decoded output -- the first min(rows,
 *   pad_rows) rows of page ids[s] - id_base decoded, exact zeros behind them, all zeros for an id of -1, an id outside [id_base,
 *   id_base + n_d) or broken offsets; lengths[s] = the rows decoded.  A row whose code is >= K is written as the NaN row.  Every
 *   byte of out is written.
 * MSIM_EINVAL for a negative size, a null or misaligned pointer (Qt, centroids, residuals, out: 16 bytes; cand / ids: 8; codes: 2;
 * the rest: 4), ld_cand < m.  n_q == 0, m == 0 or n_slots == 0 returns 0 before any pointer is looked at.  No workspace, no
 * allocation, no host synchronisation: asynchronous on `stream` and hipGraph-capturable.
 */
int msim_res_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                              const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights, int bits,
                              const int32_t *d_off, const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows, int dim,
                              const int64_t *cand, int m, int64_t ld_cand, int64_t id_base,
                              float *best_sim, int32_t *best_row, float *sims /* or NULL */, int max_rows, void *stream);
int msim_res_gather_pages(int dtype, const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights,
                          int bits, int dim, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base,
                          const int64_t *ids, int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream);

/*
 * ROWS OUT OF THE COMPRESSED SHARD AT WIDTH 320 (residual_wide_align.hip; additions to ABI 22): msim_res_align_candidates and
 * msim_res_gather_pages over the rows of a 320-wide compressed shard, with their argument lists.  Formats as
 * msim_res_wide_candidates: bf16 / f16, dim == 320, bits 2 or 4 -- MSIM_EUNSUPPORTED for anything else (the two 128-wide entries
 * above keep refusing dim 320) -- and K a multiple of 256 in 256 .. 2048: a K outside that range is MSIM_EINVAL, the code every
 * msim_res_wide_* entry gives it (the 128-wide pair above answers MSIM_EUNSUPPORTED there).  max_q_tokens > 128: MSIM_EUNSUPPORTED.
 * msim_res_wide_align_candidates: msim_align_candidates' contract (dim 320), conventions, output shapes and return codes over the
 *   compressed rows.  ARITHMETIC: for every entry, best_sim, best_row and sims hold exactly the bits msim_align_candidates (dim 320)
 *   gives the same queries and list over the output of msim_res_wide_decode_rows for the whole shard (rows 0 .. d_rows), every -inf
 *   / 0.0 / NaN / -1 convention included: the operand of the chain of ten MFMAs is built by the decode helper
 *   msim_res_wide_decode_rows uses, in the lane layout of K1a, and everything behind the operand is K1a.  A row whose code is >= K
 *   is the NaN row msim_res_wide_decode_rows writes (the code never becomes an address; no other row or entry changes).  An entry
 *   whose page is longer than max_rows, or whose offsets fall outside 0 <= d_off[c] <= d_off[c + 1] <= d_rows, is NaN / -1 in full
 *   and reads nothing.
 * msim_res_wide_gather_pages: out [n_slots, pad_rows, 320] in the corpus dtype holds exactly the bytes msim_gather_pages (row_bytes
 *   640) gives the same ids over that decoded output -- the first min(rows, pad_rows) rows of page ids[s] - id_base decoded, exact
 *   zeros behind them, all zeros for an id of -1, an id outside [id_base, id_base + n_d) or broken offsets; lengths[s] = the rows
 *   decoded.  A row whose code is >= K is written as the NaN row.  Every byte of out is written.
 * MSIM_EINVAL for a negative size, a null or misaligned pointer (Qt, centroids, residuals, out: 16 bytes; cand / ids: 8; codes: 2;
 * the rest: 4), ld_cand < m; MSIM_EUNSUPPORTED above the 2^31 - 1 limits (n_q x m, d_rows, pad_rows, n_slots) -- all before the
 * device is touched.  n_q == 0, m == 0 or n_slots == 0 returns 0 before any pointer is looked at.  No workspace, no allocation, no
 * host synchronisation: asynchronous on `stream` and hipGraph-capturable.
 */
int msim_res_wide_align_candidates(int dtype, const void *Qt, const int32_t *q_off, int n_q, int64_t q_rows, int max_q_tokens,
                                   const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights,
                                   int bits, const int32_t *d_off, const uint8_t *d_clamp0 /* or NULL */, int n_d, int64_t d_rows,
                                   int dim, const int64_t *cand, int m, int64_t ld_cand, int64_t id_base,
                                   float *best_sim, int32_t *best_row, float *sims /* or NULL */, int max_rows, void *stream);
int msim_res_wide_gather_pages(int dtype, const uint16_t *codes, const uint8_t *residuals, const void *C, int K, const float *weights,
                               int bits, int dim, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base,
                               const int64_t *ids, int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream);

/*
 * LIVE CORPUS (live_corpus.hip; additions to ABI 22): a packed corpus whose pages can be deleted and whose rows can be handed
 * back, without a change to any scorer.  A page's slot c never moves (its id stays id_base + c); `alive` uint8 [n_slots] is the
 * tombstone mask (0 = deleted).
 *
 * msim_live_compact moves the rows of live pages down over the rows of deleted ones, in place and in slot order, and rewrites
 * off int32 [n_slots + 1] so that a deleted slot becomes an empty page (off[c + 1] == off[c]): new off[c] = the sum of
 * off[j + 1] - off[j] over the live slots j < c.  Afterwards *rows_used_out (int64, device) = new off[n_slots].  Calling it again
 * changes nothing.  rows [rows_bound, row_bytes bytes each]: row_bytes a positive multiple of 16 (MSIM_EINVAL otherwise), at most
 * 65536 (MSIM_EUNSUPPORTED); one call moves rows of any element type (bf16 / f32 embedding rows, int8 code rows).  rows_bound:
 * rows the array holds at least, off[n_slots] <= rows_bound <= 2^31 - 1; every row index the device derives is checked against it
 * before it becomes an address.  The rows go through `bounce` (bounce_bytes >= row_bytes, 16-byte aligned, caller-owned) in
 * chunks of floor(bounce_bytes / row_bytes) destination rows, two stream-ordered launches per chunk (rows -> bounce, bounce ->
 * rows): a parallel in-place move could overwrite rows another workgroup has not read yet.  Rows below the first deleted page
 * are neither read nor written.  ceil(rows_bound / chunk rows) must not exceed 65536 (MSIM_EUNSUPPORTED).
 * workspace: msim_live_compact_workspace_bytes(n_slots, bounce_bytes) bytes, 16-byte aligned; the call initialises it (by a
 * kernel).  Its first int32 is a status word, valid once the call's work is done: 0 = done; otherwise an invariant was broken
 * (bit 0: off not non-decreasing from 0 or above rows_bound; bit 1: a derived row outside the array), nothing further was moved
 * and *rows_used_out = the old off[n_slots].  n_slots == 0 returns 0 before it looks at a pointer.
 *
 * msim_live_mask_scores writes -inf into scores[q, c] (fp32 [n_q, ld], ld >= n, 4-byte aligned) for every q where alive[c] == 0,
 * c < n, and touches nothing else: the mask is read once per column, only columns of deleted slots are written.
 *
 * Both are asynchronous on `stream`, allocate nothing, never synchronise with the host and are hipGraph-capturable.
 */
size_t msim_live_compact_workspace_bytes(int n_slots, int64_t bounce_bytes);
int msim_live_compact(void *rows, int64_t row_bytes, int64_t rows_bound, int32_t *off, const uint8_t *alive, int n_slots,
                      int64_t *rows_used_out, void *workspace, void *bounce, int64_t bounce_bytes, void *stream);
int msim_live_mask_scores(float *scores, int64_t ld, int n_q, int64_t n, const uint8_t *alive, void *stream);

/*
 * LIVE COMPRESSED SHARD (residual_live.hip, live_corpus.hip; additions to ABI 22): a residual-compressed corpus that is filled from
 * bf16 / f16 pages which are never kept, and whose deleted pages hand their rows back in place.  Formats as the residual-compressed
 * corpus above: bf16 / f16, width 128, bits 2 or 4, K a multiple of 256 in 256 .. 2048.
 *
 * msim_res_append encodes the pages D [n_rows, 128] with offsets d_off int32 [n_d + 1] in one pass and writes row r of D to row
 * dst_row0 + r of codes (uint16 [dst_rows]) and of residuals (uint8 [dst_rows, 16 * bits]).  codes and residuals are the BASE
 * pointers of the arrays, 16-byte aligned; dst_row0 is arbitrary, so a code may land on any 2-byte boundary.  Bit identity with the
 * two-call composition: the code of a row is what msim_cent_encode_docs gives (the same fp32 MFMA chain, k ascending, the lowest k
 * on equal values), and its residual bytes are what msim_res_encode_docs gives for that row and that code (one fp32 subtraction
 * per dimension, a value equal to a cutoff goes to the upper bucket, the same little-endian packing).  A row is read from memory
 * once.  max_doc_rows and status (int32 [n_d] or NULL) as msim_cent_encode_docs: a page whose offsets fall outside 0 .. n_rows, or
 * that is longer than max_doc_rows, gets status 1 and not one byte of either array is written for it; every other page gets 0.
 * Bytes outside rows dst_row0 .. dst_row0 + n_rows - 1 are never written: every destination row the device derives is checked
 * against dst_rows before it becomes an address.  MSIM_EINVAL for a negative size, dst_row0 + n_rows > dst_rows, dim != 128, K
 * outside the rule, a null pointer or a misaligned one (D, C, codes, residuals: 16 bytes; d_off, status, cutoffs: 4);
 * MSIM_EUNSUPPORTED for fp32 rows, bits other than 2 or 4 and max_doc_rows above 65535 * 256.  n_d == 0 or max_doc_rows == 0
 * returns 0 before it looks at a pointer.
 *
 * msim_res_live_compact is msim_live_compact for the two arrays of such a shard: ONE offset plan (one rewrite of off, the rule,
 * status word, `first` row below which nothing is read or written, idempotence and bounds checks of msim_live_compact), against
 * which both codes (uint16 [rows_bound]) and residuals (uint8 [rows_bound, 16 * bits]) move.  The 2-byte codes move per row (a
 * 16-byte piece of them would span eight rows and cross page boundaries and alignments), the residual rows as 16-byte pieces.
 * Both go through `bounce` (16-byte aligned, caller-owned) in chunks of
 *     chunk rows = floor(bounce_bytes / (16 * bits + 2))      destination rows (at least 1: MSIM_EINVAL otherwise),
 * the chunk's residual rows first and its codes behind them, with the two-launch discipline of msim_live_compact per array
 * (source -> bounce, then bounce -> destination).  ceil(rows_bound / chunk rows) must not exceed 65536 (MSIM_EUNSUPPORTED).
 * workspace: msim_res_live_compact_workspace_bytes(n_slots, bounce_bytes) bytes, 16-byte aligned, initialised by the call (by a
 * kernel); its first int32 is the status word of msim_live_compact: non-zero means an invariant was broken, nothing further was
 * moved and *rows_used_out = the old off[n_slots].  codes, residuals, bounce and workspace 16-byte aligned, off 4-byte,
 * rows_used_out 8-byte (MSIM_EINVAL); bits other than 2 or 4 and rows_bound > 2^31 - 1 are MSIM_EUNSUPPORTED.  n_slots == 0 returns
 * 0 before it looks at a pointer.
 *
 * msim_f4_live_compact (an addition to ABI 22) is msim_live_compact for the two arrays of a live FP4 index (msim_f4_encode_rows,
 * msim_f4w_encode_rows): ONE offset plan, with the semantics of msim_live_compact -- the new offsets in place, *rows_used_out, the
 * status word, nothing at or past rows_bound touched, a second call a no-op -- against which both codes (uint8 [rows_bound,
 * code_row_bytes], code_row_bytes 64 for width 128 or 160 for width 320) and scales (uint8 [rows_bound], one E8M0 byte per row)
 * move.  The code rows move as 16-byte pieces, the scale bytes per row.  Both go through `bounce` (16-byte aligned, caller-owned)
 * in chunks of
 *     chunk rows = floor(bounce_bytes / (code_row_bytes + 1))      destination rows (at least 1: MSIM_EINVAL otherwise),
 * the chunk's code rows first and its scale bytes behind them, with the two-launch discipline of msim_live_compact per array.
 * ceil(rows_bound / chunk rows) must not exceed 65536 (MSIM_EUNSUPPORTED).  workspace:
 * msim_f4_live_compact_workspace_bytes(n_slots, bounce_bytes) bytes (the size msim_live_compact_workspace_bytes gives), 16-byte
 * aligned, initialised by the call; its first int32 is the status word of msim_live_compact.  Refused before the device is
 * touched: a negative size or a null pointer (MSIM_EINVAL); codes, bounce or workspace not 16-byte aligned, off not 4-byte,
 * rows_used_out not 8-byte aligned (MSIM_EINVAL; scales may have any alignment, as in msim_f4_encode_rows); code_row_bytes other
 * than 64 or 160 and rows_bound > 2^31 - 1 (MSIM_EUNSUPPORTED).  n_slots == 0 returns 0 before it looks at a pointer.
 *
 * All three are asynchronous on `stream`, allocate nothing, never synchronise with the host and are hipGraph-capturable.
 */
int msim_res_append(int dtype, const void *D, const int32_t *d_off, int n_d, int64_t n_rows, int dim, int max_doc_rows, const void *C,
                    int K, const float *cutoffs, int bits, uint16_t *codes, uint8_t *residuals, int64_t dst_row0, int64_t dst_rows,
                    int32_t *status /* or NULL */, void *stream);
size_t msim_res_live_compact_workspace_bytes(int n_slots, int64_t bounce_bytes);
int msim_res_live_compact(uint16_t *codes, uint8_t *residuals, int bits, int64_t rows_bound, int32_t *off, const uint8_t *alive,
                          int n_slots, int64_t *rows_used_out, void *workspace, void *bounce, int64_t bounce_bytes, void *stream);
size_t msim_f4_live_compact_workspace_bytes(int n_slots, int64_t bounce_bytes);
int msim_f4_live_compact(uint8_t *codes, int64_t code_row_bytes /* 64 or 160 */, uint8_t *scales, int64_t rows_bound, int32_t *off,
                         const uint8_t *alive, int n_slots, int64_t *rows_used_out, void *workspace, void *bounce,
                         int64_t bounce_bytes, void *stream);

/*
 * HARD-NEGATIVE MINING AND THE PAGE GATHER (mine.hip; additions to ABI 22).  Mining is "mask the score matrix of the full scan, then
 * msim_topk_f32": no scorer and no selection kernel changes.
 *
 * scores fp32 [n_q, ld], ld >= n, 4-byte aligned: column c is page id_base + c.  The positives of query q are
 * pos_ids[pos_off[q] .. pos_off[q + 1]) (int64 GLOBAL ids; pos_off int32 [n_q + 1], read on the device and clipped to [0, nnz], so
 * a broken pair yields an empty list, never an address).  An id that is negative or outside [id_base, id_base + n) is ignored;
 * duplicates are allowed.
 *
 * msim_mine_bounds: bounds[q] (fp32 [n_q]) = max over the in-shard positives of scores[q, id - id_base] (alive != NULL: those with
 * alive[id - id_base] != 0 only: a deleted page is not there), or +inf where the query has none (local != 0: -inf instead -- what a rank that holds no positive contributes to an all-reduce MAX).
 *
 * msim_mine_mask writes -inf, in place, into scores[q, c] (c < n) where
 *     c is an in-shard positive of q,  or  alive != NULL and alive[c] == 0 (uint8 [n]),  or
 *     bounds != NULL and scores[q, c] > max_ratio * bounds[q]   (ONE fp32 multiply, then the reference's own comparison,
 *     loss/bi_encoder_losses.py:58-59; with bounds[q] < 0 the threshold therefore lies ABOVE the positive's score, as there;
 *     a NaN threshold (0 x inf) drops nothing)
 * and touches nothing else: only changing columns are stored.  bounds is what msim_mine_bounds wrote earlier on the same stream
 * (or the all-reduced maximum of several shards); NULL skips the comparison (max_ratio is then ignored; NaN is MSIM_EINVAL
 * otherwise).  With bounds == NULL and alive == NULL only the positives' columns are written.
 *
 * msim_gather_pages: out [n_slots, pad_rows, row_bytes] <- the rows of page ids[s] (int64 [n_slots] GLOBAL ids) of the packed
 * corpus rows [d_rows, row_bytes] / d_off int32 [n_d + 1]: min(len, pad_rows) rows copied, every row after them zero,
 * lengths[s] (int32) = the rows copied.  A slot whose id is negative or outside [id_base, id_base + n_d), or whose offsets are not
 * 0 <= d_off[c] <= d_off[c + 1] <= d_rows, is a page of zeros of length 0.  Every byte of out is written.  row_bytes: a positive
 * multiple of 16 (MSIM_EINVAL otherwise), at most 65536; rows and out 16-byte aligned; d_rows, pad_rows, n_slots <= 2^31 - 1
 * (MSIM_EUNSUPPORTED).  Bytes moved: n_slots x pad_rows x row_bytes written + the copied rows read + 12 per slot.
 *
 * MSIM_EINVAL for a negative size, a null or misaligned pointer, ld < n.  n_q == 0 (n_slots == 0) returns 0 before a pointer is
 * looked at.  All three are asynchronous on `stream`, allocate nothing, never synchronise with the host and are hipGraph-capturable.
 */
int msim_mine_bounds(const float *scores, int64_t ld, int n_q, int64_t n, const int64_t *pos_ids, const int32_t *pos_off, int64_t nnz,
                     int64_t id_base, const uint8_t *alive /* or NULL */, int local, float *bounds, void *stream);
int msim_mine_mask(float *scores, int64_t ld, int n_q, int64_t n, const float *bounds /* or NULL */, float max_ratio,
                   const uint8_t *alive /* or NULL */, const int64_t *pos_ids, const int32_t *pos_off, int64_t nnz, int64_t id_base,
                   void *stream);
int msim_gather_pages(const void *rows, int64_t row_bytes, int64_t d_rows, const int32_t *d_off, int n_d, int64_t id_base,
                      const int64_t *ids, int64_t n_slots, int64_t pad_rows, void *out, int32_t *lengths, void *stream);

/*
 * PAGE FILTERS (filter.hip; additions to ABI 22): which pages of a shard each query may return -- a tenant, a collection, the pages a
 * metadata query matched.  A filter either masks a score matrix ("mask, then msim_topk_f32", as mining does) or becomes a candidate
 * list for msim_fwd_candidates; no scorer and no selection kernel changes.
 *
 * A filter over the n pages of a shard (page c has id id_base + c) is given in exactly one of two forms:
 *     bits         uint32 words, bit c % 32 of word c / 32 is page c (1 = allowed).  ld_words == 0: ONE row of ceil(n / 32) words
 *                  shared by every query; otherwise [n_q, ld_words], ld_words >= ceil(n / 32), one row per query.  Bits at
 *                  positions >= n are never relied upon: every consumer clips to n.
 *     labels       page_labels int32 [n] and query_labels int32 [n_q]: page c is allowed for q iff page_labels[c] ==
 *                  query_labels[q].  No [n_q, n] object exists anywhere.
 * alive (uint8 [n], or NULL) is ANDed in: alive[c] == 0 is a deleted page, allowed for nobody.
 *
 * msim_filter_pack: mask bytes [rows, ld_mask] (ld_mask >= n, any alignment; non-zero = allowed) -> words [rows, ld_words],
 * ld_words >= ceil(n / 32).  Words 0 .. ceil(n / 32) - 1 of every row are written, bits at positions >= n as 0.  One wave ballot
 * yields two words; the mask is read 4 bytes per lane where its rows are 4-byte aligned.
 *
 * msim_filter_mask writes -inf, in place, into scores[q, c] (fp32 [n_q, ld], ld >= n, 4-byte aligned; c < n) wherever page c is not
 * allowed for q or is not alive, and touches nothing else: the scores are never read, only changing columns are stored (a kept
 * column keeps its bits, NaN and -0.0 included), 16 bytes at a time where four neighbours change and the rows are 16-byte aligned;
 * rows of any 4-byte alignment work.
 *
 * msim_filter_list, the ordered compaction: for every query row q the GLOBAL ids id_base + c of its allowed and alive pages go,
 * ascending, into cand[q, 0 .. count) (int64 [n_q, ld_cand], ld_cand >= m_cap); cand[q, count .. m_cap) = -1; counts[q] (int32) =
 * the true count.  A shared filter writes the same list into all n_q rows.  A row with more than m_cap allowed pages keeps its first
 * m_cap, reports the true count and sets the status word (msim_fwd_candidates' convention): the first int32 of `workspace`
 * (msim_filter_list_workspace_bytes(n_q, n) bytes, 16-byte aligned, initialised by the call) is 0 once the call's work is done, or
 * 1 when a row overflowed.  The order is by construction, not by sorting: one workgroup per row walks the row in passes of
 * S = 8192 columns (256 lanes x one 32-bit word), and a popcount per lane, a wave prefix, a per-wave carry through LDS and a running
 * carry across passes give every page its position.  No atomics.  n <= 2^31 - 1 (MSIM_EUNSUPPORTED).
 *
 * msim_filter_ids: in ids (int64 [n_q, ld], m columns, GLOBAL ids) every id inside [id_base, id_base + n) that is not allowed for
 * its row, or not alive, becomes -1, in place.  -1 and ids outside the shard are left alone: another rank holds them, and
 * msim_fwd_candidates answers them with (-inf, -1).
 *
 * MSIM_EINVAL for a negative size, a null or misaligned pointer, ld < n (ld_mask < n, ld_cand < m_cap, ld < m, 0 < ld_words <
 * ceil(n / 32)), and for both or neither of (bits) and (page_labels, query_labels).  n_q == 0 (rows == 0) or n == 0 returns 0
 * before a pointer is looked at (and writes nothing).  All are asynchronous on `stream`, allocate nothing, never synchronise with
 * the host and are hipGraph-capturable.
 */
int msim_filter_pack(const uint8_t *mask, int64_t ld_mask, int rows, int64_t n, uint32_t *words, int64_t ld_words, void *stream);
int msim_filter_mask(float *scores, int64_t ld, int n_q, int64_t n, const uint32_t *bits /* or NULL */, int64_t ld_words,
                     const int32_t *page_labels /* or NULL */, const int32_t *query_labels /* or NULL */,
                     const uint8_t *alive /* or NULL */, void *stream);
size_t msim_filter_list_workspace_bytes(int n_q, int64_t n);
int msim_filter_list(const uint32_t *bits /* or NULL */, int64_t ld_words, const int32_t *page_labels /* or NULL */,
                     const int32_t *query_labels /* or NULL */, const uint8_t *alive /* or NULL */, int n_q, int64_t n,
                     int64_t id_base, int64_t *cand, int64_t ld_cand, int m_cap, int32_t *counts, void *workspace, void *stream);
int msim_filter_ids(int64_t *ids, int64_t ld, int n_q, int64_t m, int64_t n, int64_t id_base, const uint32_t *bits /* or NULL */,
                    int64_t ld_words, const int32_t *page_labels /* or NULL */, const int32_t *query_labels /* or NULL */,
                    const uint8_t *alive /* or NULL */, void *stream);

/*
 * DOCUMENT-LEVEL SEARCH (group.hip; additions to ABI 22): the n pages of a shard belong to G documents, and a search returns the
 * top-k DOCUMENTS, each scored by its best page.  No scorer and no selection kernel changes: msim_group_reduce sits between a score
 * matrix and msim_topk_f32, msim_group_select behind msim_fwd_candidates and behind the all-gather of a sharded search.
 *
 * The grouping is a CSR over LOCAL page indices (page c has id id_base + c): offsets int32 [n_groups + 1], pages int32 [n]; document
 * g owns pages[offsets[g] .. offsets[g + 1]), ascending.  Documents may have any length >= 1 and their pages need not be contiguous.
 *
 * msim_group_reduce: scores fp32 [n_q, ld] (ld >= n, 4-byte aligned, any row alignment) -> group_scores fp32 [n_q, ld_out] and
 * group_pages int64 [n_q, ld_out] (ld_out >= n_groups; columns 0 .. n_groups - 1 are written, nothing else).  Entry (q, g) is the
 * best page of document g for query q under the project's order: the higher score first, equal floats tie (-0.0 and +0.0 tie, as in
 * msim_topk_f32), and on a tie the lower page wins.  group_scores holds the winner's own bits, group_pages its GLOBAL id.  A
 * document whose pages all score -inf (or that owns no page) is (-inf, -1).  NaN is outside the contract, as for msim_topk_f32.
 * A gather: every output has one owner, there is no atomic, the result does not depend on scheduling.  A document is reduced by
 * one lane, one wave or one workgroup by its length: up to MSIM_GROUP_THREAD_MAX pages by a lane, up to MSIM_GROUP_WAVE_MAX by a
 * wave, longer ones by the 256 lanes of the workgroup.  HBM traffic: 4 B per scored pair read, 12 B per (q, g) written; the CSR is
 * read once per workgroup into registers (the workgroup form re-reads it per row, from L2).  Offsets are clipped to [0, n] and a
 * page index outside [0, n) is skipped before it becomes an address.  n <= 2^31 - 1 (MSIM_EUNSUPPORTED).
 *
 * msim_group_select, the grouped top-k of candidate rows: scores fp32, gids int64 (document ids), pages int64 (page ids), each
 * [n_q, ld] with m columns (ld >= m).  An entry with gid < 0 or a score of -inf is no entry.  Per row the best entry of every
 * document by (score descending, page id ascending) survives, the survivors are ordered by (score descending, document id
 * ascending), the first k go to out_scores / out_gids / out_pages (each contiguous [n_q, k]) and the rest of the row is
 * (-inf, -1, -1).  Scores come back as msim_topk_f32 returns them (-0.0 as +0.0).  One workgroup per row, two bitonic sorts in
 * dynamic LDS of 20 B per entry (80 KiB at m = 4096).  m <= MSIM_GROUP_SELECT_MAX_M, k <= MSIM_GROUP_SELECT_MAX_K
 * (MSIM_EUNSUPPORTED beyond).
 *
 * MSIM_EINVAL for a negative size, k <= 0, a null or misaligned pointer, ld < n, ld_out < n_groups, ld < m.  n_q == 0 or
 * n_groups == 0 (msim_group_reduce), n_q == 0 or m == 0 (msim_group_select) return 0 before a pointer is looked at and write
 * nothing.  Both are asynchronous on `stream`, allocate nothing, never synchronise with the host and are hipGraph-capturable.
 */
#define MSIM_GROUP_THREAD_MAX 16     /* a document of at most this many pages is reduced by one lane */
#define MSIM_GROUP_WAVE_MAX 1024     /* ... of at most this many by one wave; longer ones by the workgroup */
#define MSIM_GROUP_SELECT_MAX_M 4096 /* widest candidate row of msim_group_select */
#define MSIM_GROUP_SELECT_MAX_K 1024 /* largest k of msim_group_select */
int msim_group_reduce(const float *scores, int64_t ld, int n_q, int64_t n, const int32_t *offsets, const int32_t *pages, int n_groups,
                      int64_t id_base, float *group_scores, int64_t *group_pages, int64_t ld_out, void *stream);
int msim_group_select(const float *scores, const int64_t *gids, const int64_t *pages, int n_q, int m, int64_t ld, int k,
                      float *out_scores, int64_t *out_gids, int64_t *out_pages, void *stream);

/*
 * PERSISTENCE (digest.hip; additions to ABI 22): the digest a saved shard or index is verified by (colpali_amd/persist.py,
 * DESIGN.md section 3.23).  msim_digest sums over bytes in HBM -- what actually landed on the device --, msim_digest_host computes
 * the same sum over host memory.  It detects corruption, truncation and misplacement.  It is NOT a cryptographic hash: anyone who
 * can write the file can make any digest they like.
 *
 * The contract (tests/digest_truth.py restates it in numpy uint64; all arithmetic is mod 2^64):
 *   - the nbytes bytes at `data` are read as little-endian 64-bit words w_0 .. w_{n-1}, n = ceil(nbytes / 8); the last word is
 *     zero-padded past nbytes;
 *   - word i has the absolute index g_i = pos / 8 + i (`pos`: the byte offset of `data` in the object it is a part of);
 *   - acc[0] += sum_i mix(w_i + (g_i + 1) * MSIM_DIGEST_C0),    acc[1] += sum_i mix((w_i ^ MSIM_DIGEST_K) + (g_i + 1) * MSIM_DIGEST_C1)
 *   - mix is the splitmix64 finaliser:  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31.
 * The result is ADDED INTO acc (the caller zeroes it, or carries a running sum), hence
 *   - it does not depend on the launch plan: integer addition commutes (rerun identity, bit for bit);
 *   - chunks compose: the digest of a buffer is the sum of the digests of any cover of it by pieces that start on 8-byte boundaries,
 *     each with its own `pos`;
 *   - a trailing all-zero word still counts (mix(0 + k) != 0 for the k used): length and position are covered.
 *
 * msim_digest: `data` and `acc` (uint64 [2]) are device pointers; one kernel on `stream` (16-byte loads on the aligned body, one word
 * on its own in front when `data` is 8- but not 16-byte aligned, the byte tail read by one lane; per-lane accumulators, a wave fold,
 * two 64-bit integer atomics per workgroup).  No allocation, no synchronisation, hipGraph-capturable (a replay adds again).
 * `pos` and `nbytes` may exceed 2^32.  msim_digest_host: both pointers are host pointers; one thread.
 * MSIM_EINVAL, before any device work: acc == NULL; data == NULL with nbytes > 0; pos % 8 != 0; `data` not 8-byte aligned.
 * nbytes == 0 is a successful no-op.
 */
#define MSIM_DIGEST_C0 0x9E3779B97F4A7C15ull /* lane 0's position multiplier (odd) */
#define MSIM_DIGEST_C1 0xC2B2AE3D27D4EB4Full /* lane 1's position multiplier (odd) */
#define MSIM_DIGEST_K 0xD6E8FEB86659FD93ull  /* lane 1 reads w ^ K (odd) */
int msim_digest(const void *data, size_t nbytes, uint64_t pos, uint64_t *acc /* device, [2] */, void *stream);
int msim_digest_host(const void *data, size_t nbytes, uint64_t pos, uint64_t acc[2]);

#ifdef __cplusplus
}
#endif
#endif /* COLPALI_AMD_MAXSIM_H */
