"""colpali_amd -- MI355X (gfx950) native late-interaction scorer.

Drop-in for the MaxSim hot path of illuin-tech/colpali:
  * score_multi_vector            <- BaseVisualRetrieverProcessor.score_multi_vector
                                     (colpali_engine/utils/processing_utils.py:132-187)
  * ColbertPairwiseCELoss (+ ColbertLoss, ColbertSigmoidLoss, ColbertModule)
                                  <- colpali_engine/loss/late_interaction_losses.py:255-313 (:110-164, :401-465, :6-107)
  * ShardedRetriever / topk       -- sharded-corpus top-k with an RCCL all-gather merge (no reference equivalent); lists of up to
                                     TOPK_MAX_K = 8192 entries per row, in one order (score desc, id asc) at every length
  * rerank                        -- exact MaxSim of per-query candidate lists; two-stage search (ShardedRetriever.search(prefilter=))
  * align / Alignment             -- which page row matched each query token of a search hit, and its similarity maps
  * mine_hard_negatives / gather_pages -- hard negatives by the model's own MaxSim score over the resident corpus, and the padded
                                     box of the chosen pages for ColbertNegativeCELoss / ColbertPairwiseNegativeCELoss
  * PageFilter                    -- filtered search (ShardedRetriever.search(filter=), LiveCorpus.search(filter=)): the top-k within
                                     one tenant's / collection's pages, by masking the scan or by listing and reranking them
  * PageGroups                    -- document-level search (ShardedRetriever.search(group_by=), LiveCorpus.search(group_by=)): pages
                                     grouped into documents, the top-k DOCUMENTS, each scored by (and returned with) its best page
  * FdeIndex / fde_scores         -- fixed dimensional encodings (MUVERA): a one-GEMM first stage for prefilter=
  * Int8Index / int8_scores       -- an int8 copy of the corpus scored token by token on int8 MFMAs: a first stage for prefilter=
  * BinaryIndex / binary_scores   -- one sign bit per dimension of every corpus row (16 bytes per row), scored against the int8
                                     queries on int8 MFMAs: a token-level first stage for prefilter= at 1/16 of the bf16 shard
  * Fp4Index / fp4_scores         -- every corpus row and query token as 128 e2m1 values and one power-of-two scale (65 bytes per
                                     row), scored on the block-scaled FP4 MFMA: a token-level first stage for prefilter=
  * fp6_scores                    -- the same Fp4Index scored with e2m3 (FP6) query tokens, at the same MFMA rate: the better
                                     first stage, ShardedRetriever(..., fp4_score_fn=fp6_scores)
  * fp4_rerank_scores / fp6_rerank_scores -- the list form of the two: the FP4 score of the pages a candidate list names (65 bytes
                                     per row read, the scan's bits); the middle stage of a three-stage search,
                                     ShardedRetriever.search(prefilter=fde, n_candidates=m1, refine=fp4_index, n_refine=m2)
  * Fp4WideIndex / fp4_wide_scores -- the FP4 index of a 320-wide (ColQwen3) shard: 160 bytes of e2m1 nibbles and one scale byte
                                     per row, three chained block-scaled MFMAs per 16 rows x 16 tokens: a first stage for prefilter=
  * fp4_wide_rerank_scores        -- its list form: the FP4 score of the pages a candidate list names (161 bytes per row read, the
                                     scan's bits); search(prefilter=pooled, n_candidates=m1, refine=fp4_wide_index, n_refine=m2)
  * fp6_wide_scores / fp6_wide_rerank_scores -- the same Fp4WideIndex scored with e2m3 (FP6) query tokens, scan and list form:
                                     ShardedRetriever(..., fp4_wide_score_fn=fp6_wide_scores,
                                     fp4_wide_rerank_fn=fp6_wide_rerank_scores)
  * FdeWideIndex / fde_wide_scores -- the fixed dimensional encodings of a 320-wide (ColQwen3) shard, by an encoder of its own and
                                     the scorer of fde_scores: the one-GEMM first stage at width 320, and the front of
                                     search(prefilter=fde_wide, n_candidates=m1, refine=fp4_wide_index, n_refine=m2)
  * LiveCorpus.fp4_index / drop_fp4_index -- the FP4 index of a shard that changes (width 128 and 320), kept in step: add encodes
                                     the new rows, compact moves code rows and scale bytes (msim_f4_live_compact); its stage-1
                                     scores, and those of any Fp4Index / Fp4WideIndex passed as prefilter=, are tombstone-masked
  * CentroidIndex / centroid_scores -- rows stored as the id of their nearest centroid, pages scored by table lookups (PLAID's
                                     centroid interaction): a first stage for prefilter= at 2 bytes per row
  * ResidualCorpus / residual_rerank_scores -- PLAID's second half: the shard itself as centroid codes + 2 / 4 residual bits per
                                     dimension (34 / 66 bytes per row instead of 256), candidate lists reranked straight from them
  * residual_scores               -- the full scan of such a shard, a page decoded once per group of queries: the score matrix
                                     behind ShardedRetriever(rc, score_fn=residual_scores) -- search, filter=, group_by=, mine
  * residual_align / residual_gather_pages -- align and gather_pages over such a shard, the listed pages decoded inside the kernel
                                     (align and gather_pages dispatch to them on a ResidualCorpus)
  * CentroidWideIndex / centroid_wide_scores, ResidualWideCorpus / residual_wide_rerank_scores -- the same two at width 320
                                     (ColQwen3): 82 / 162 bytes per row instead of 640, stage 1 by prefilter=rc.index, candidate
                                     lists reranked straight from the compressed rows (the live form exists at width 128 only)
  * residual_wide_scores          -- the full scan of a ResidualWideCorpus, residual_scores at width 320: the score matrix behind
                                     ShardedRetriever(rc, score_fn=residual_wide_scores) -- search, filter=, group_by=, mine
  * residual_wide_align / residual_wide_gather_pages -- align and gather_pages over a ResidualWideCorpus, the listed pages decoded
                                     inside the kernel (align and gather_pages dispatch to them on a ResidualWideCorpus)
  * LiveResidualCorpus           -- such a shard filled incrementally from pages that are never kept: add (one fused encode pass),
                                     delete, compact in place; the lifecycle LiveCorpus gives the bf16 shard
  * save / load / verify_file     -- every shard and index class as one flat, versioned file (no pickle), streamed through the pinned
                                     double buffer and verified chunk by chunk by a digest computed on the device (msim_digest)
  * embedding_head / CorpusWriter <- the projection / L2-norm / mask tail of every Col* forward
                                     (models/paligemma/colpali/modeling_colpali.py:67-77), writing the packed corpus;
                                     width 128, and width 320 (ColQwen3: the width is the weight's, CorpusWriter(width=320))
The compute lives in hand-written HIP kernels behind a C ABI (include/maxsim.h,
colpali_amd/csrc/); this package is the thin host-side mirror of the reference interface.
"""
from .align import Alignment, align
from .binary_index import BinaryIndex, binary_scores, binary_scores_from_codes
from .centroid import CentroidIndex, centroid_scores, train_centroids
from .corpus import PackedCorpus, PackedQueries, block_clamp0, pack_passages, pack_queries
from . import loss
from .embed import CorpusWriter, embedding_head
from .fp4_index import (Fp4Index, fp4_quantize_queries, fp4_rerank_scores, fp4_scores, fp4_scores_from_codes, fp6_quantize_queries,
                        fp6_rerank_scores, fp6_scores)
from .fp4_wide_index import (Fp4WideIndex, fp4_wide_quantize_queries, fp4_wide_rerank_scores, fp4_wide_scores,
                             fp4_wide_scores_from_codes, fp6_wide_quantize_queries, fp6_wide_rerank_scores, fp6_wide_scores)
from .fde import FdeConfig, FdeIndex, encode_queries, fde_scores
from .fde_wide import FdeWideIndex, fde_wide_encode_queries, fde_wide_scores
from .filter import PageFilter
from .group import PageGroups, group_reduce, group_select
from .int8_index import Int8Index, int8_scores, quantize_queries
from .live import LiveCorpus
from .live_residual import LiveResidualCorpus
from .mine import gather_pages, mine_hard_negatives
from .loss import (ColbertLoss, ColbertModule, ColbertNegativeCELoss, ColbertPairwiseCELoss,
                   ColbertPairwiseNegativeCELoss, ColbertSigmoidLoss, maxsim, maxsim_paired)
from .persist import ShardFileError, digest, load, save, verify_file
from .pooling import HierarchicalTokenPooler, TokenPoolingOutput
from .patch import patch_colpali_engine, unpatch_colpali_engine
from .residual import (ResidualCorpus, residual_align, residual_gather_pages, residual_rerank_scores, residual_scores,
                       train_residual_codec)
from .residual_wide import (CentroidWideIndex, ResidualWideCorpus, centroid_wide_scores, residual_wide_align,
                            residual_wide_gather_pages, residual_wide_rerank_scores, residual_wide_scores)
from .retrieval import (TOPK_MAX_K, ExactMaxSimIndex, ResidualMaxSimIndex, ShardedRetriever, create_plaid_index, get_topk_plaid, merge_gathered,
                        rerank, shard_range, shard_topk, topk)
from .scoring import (get_similarity_maps_from_embeddings, get_torch_device, maxsim_scores, score_multi_vector,
                      score_single_vector, similarity_matrix)

__all__ = [
    "Alignment",
    "align",
    "CorpusWriter",
    "HierarchicalTokenPooler",
    "TokenPoolingOutput",
    "embedding_head",
    "FdeConfig",
    "FdeIndex",
    "encode_queries",
    "fde_scores",
    "FdeWideIndex",
    "fde_wide_encode_queries",
    "fde_wide_scores",
    "Int8Index",
    "int8_scores",
    "quantize_queries",
    "BinaryIndex",
    "binary_scores",
    "binary_scores_from_codes",
    "Fp4Index",
    "fp4_scores",
    "fp4_scores_from_codes",
    "fp4_quantize_queries",
    "fp6_scores",
    "fp6_quantize_queries",
    "fp4_rerank_scores",
    "fp6_rerank_scores",
    "Fp4WideIndex",
    "fp4_wide_scores",
    "fp4_wide_rerank_scores",
    "fp4_wide_scores_from_codes",
    "fp4_wide_quantize_queries",
    "fp6_wide_scores",
    "fp6_wide_quantize_queries",
    "fp6_wide_rerank_scores",
    "CentroidIndex",
    "centroid_scores",
    "train_centroids",
    "ResidualCorpus",
    "ResidualMaxSimIndex",
    "residual_align",
    "residual_gather_pages",
    "residual_rerank_scores",
    "residual_scores",
    "train_residual_codec",
    "CentroidWideIndex",
    "centroid_wide_scores",
    "ResidualWideCorpus",
    "residual_wide_align",
    "residual_wide_gather_pages",
    "residual_wide_rerank_scores",
    "residual_wide_scores",
    "LiveCorpus",
    "LiveResidualCorpus",
    "PageFilter",
    "PageGroups",
    "group_reduce",
    "group_select",
    "mine_hard_negatives",
    "gather_pages",
    "ColbertLoss",
    "ColbertModule",
    "ColbertNegativeCELoss",
    "ColbertPairwiseNegativeCELoss",
    "maxsim_paired",
    "ColbertPairwiseCELoss",
    "ColbertSigmoidLoss",
    "PackedCorpus",
    "PackedQueries",
    "maxsim",
    "ShardedRetriever",
    "ExactMaxSimIndex",
    "create_plaid_index",
    "get_topk_plaid",
    "merge_gathered",
    "rerank",
    "shard_range",
    "shard_topk",
    "topk",
    "TOPK_MAX_K",
    "block_clamp0",
    "get_torch_device",
    "maxsim_scores",
    "pack_passages",
    "patch_colpali_engine",
    "unpatch_colpali_engine",
    "pack_queries",
    "score_multi_vector",
    "score_single_vector",
    "similarity_matrix",
    "get_similarity_maps_from_embeddings",
    "save",
    "load",
    "verify_file",
    "digest",
    "ShardFileError",
]
