"""E2M3 (FP6) query tokens against the FP4 index, without a GPU: the truth helper (tests/fp6_truth.py) on its own edge cases, the
contract's point on numpy alone (the first stage's error against the exact MaxSim is smaller with e2m3 queries than with e2m1
ones), the ABI's argument checks (no device work), the Python layer's refusals, exports, and
ShardedRetriever(fp4_score_fn=<the e2m3 truth>) over gloo worlds of 2 and 3: every rank must get the unsharded answer."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fp4_truth as ft
from tests import fp6_truth as f6

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def _bf16(v):
    return int(ft.raw_bits(torch.tensor([[v]], dtype=torch.bfloat16))[0, 0])


def edge_rows():
    """raw bf16 rows for the encoder's edges, shared with the GPU test: (raw uint16 [n, 128], {name: row})"""
    raw = np.zeros((16, 128), dtype=np.uint16)
    ties = [(f6.GRID[c] + f6.GRID[c + 1]) / 2 for c in range(31)]              # every midpoint of neighbouring codes, exact in bf16
    raw[0, 0] = _bf16(7.5)
    raw[0, 1:32] = [_bf16(t) for t in ties]
    raw[0, 40:71] = [_bf16(-t) for t in ties]
    raw[1, 100] = _bf16(7.5 * 2.0 ** -9)                                        # the same ties at e = -9, other lanes
    raw[1, 3:34] = [_bf16(t * 2.0 ** -9) for t in ties]
    raw[2] = 0                                                                  # a row of +0.0
    raw[3] = 0x8000                                                             # a row of -0.0
    raw[4, 7] = _bf16(7.5 * 2.0 ** 3)                                           # the maximum exactly 7.5 * 2^3 ...
    raw[4, 8] = _bf16(2.0 ** 3)
    raw[5] = raw[4]
    raw[5, 7] += 1                                                              # ... and one bf16 ulp above
    raw[6, 9] = _bf16(1.875 * 2.0 ** -4)                                        # m = 1.875 exactly ...
    raw[6, 10] = _bf16(-(2.0 ** -6))
    raw[7] = raw[6]
    raw[7, 9] += 1                                                              # ... and one ulp above
    raw[8, 0], raw[8, 1] = 0x0001, 0x8001                                       # bf16 subnormals only: far below 7.5 * 2^-32
    raw[9, 0], raw[9, 1], raw[9, 2] = _bf16(2.0 ** -31), _bf16(-(2.0 ** -36)), _bf16(2.0 ** -35)     # e clamps at -32; 1/16 ties to 0
    raw[10, 0], raw[10, 1] = _bf16(-(2.0 ** 40)), _bf16(2.0 ** 33)              # e clamps at +32: saturates at -7.5
    raw[11, 5] = _bf16(7.5 * 2.0 ** 32)
    rows = dict(ties=0, ties_small=1, zero=2, neg_zero=3, max_exact=4, max_above=5, m_exact=6, m_above=7, subnormal=8, clamp_lo=9,
                clamp_hi=10, max_at_clamp=11)
    return raw, rows, ties


def edge_rows_f16():
    """raw f16 rows, shared with the GPU test: the largest finite value beside the smallest subnormal, subnormals only, the smallest
    normal beside the largest subnormal, and every tie at e = 0"""
    raw16 = np.zeros((4, 128), dtype=np.uint16)
    raw16[0, 0], raw16[0, 1] = 0x7bff, 0x0001
    raw16[1, 0], raw16[1, 1], raw16[1, 2] = 0x03ff, 0x8200, 0x0001              # subnormals only: 1023, -512 and 1 times 2^-24
    raw16[2, 0], raw16[2, 1] = 0x0400, 0x03ff                                   # 2^-14 and the largest subnormal
    ties = np.array([7.5] + [(f6.GRID[c] + f6.GRID[c + 1]) / 2 for c in range(31)], dtype=np.float16)
    raw16[3, 64:96] = ties.view(np.uint16)
    raw16[3, 96:128] = (-ties).view(np.uint16)
    return raw16


# ------------------------------------------------------------------------------------------------------------ the truth helper
def test_truth_grid_is_the_32_e2m3_magnitudes():
    assert len(f6.GRID) == 32 and (np.diff(f6.GRID) > 0).all() and f6.GRID[0] == 0 and f6.GRID[31] == 7.5
    assert f6.GRID[1] == 0.125 and f6.GRID[7] == 0.875 and f6.GRID[8] == 1.0 and f6.GRID[16] == 2.0 and f6.GRID[24] == 4.0
    assert np.array_equal(f6.GRID * 8, np.round(f6.GRID * 8))                   # every value a multiple of 1/8


def test_truth_every_tie_goes_to_the_even_code():
    raw, rows, ties = edge_rows()
    codes, scales = f6.encode(raw[:2])
    assert scales.tolist() == [127, 127 - 9]
    f = f6.unpack_fields(codes)
    even = [c if c % 2 == 0 else c + 1 for c in range(31)]                       # the tie between codes c and c + 1
    assert f[0, 0] == 31 and f[0, 1:32].tolist() == even
    assert f[0, 40:71].tolist() == [0] + [32 | c for c in even[1:]]              # -1/16 rounds to code 0: the field is 0, not 32
    assert f[1, 100] == 31 and f[1, 3:34].tolist() == even
    # just off a tie, the nearer value wins
    eps = 2.0 ** -10
    x = np.zeros((1, 128))
    x[0, 0] = 7.5
    x[0, 1:32] = [t + eps for t in ties]
    x[0, 40:71] = [t - eps for t in ties]
    f = f6.unpack_fields(f6.encode_values(x)[0])
    assert f[0, 1:32].tolist() == list(range(1, 32)) and f[0, 40:71].tolist() == list(range(31))


@pytest.mark.parametrize("e", [-32, -7, 0, 3, 32])
def test_truth_exponent_at_a_maximum_of_seven_and_a_half_and_one_ulp_above(e):
    raw = np.zeros((2, 128), dtype=np.uint16)
    raw[0, 3] = _bf16(7.5 * 2.0 ** e)
    raw[1, 3] = raw[0, 3] + 1                                     # one bf16 ulp above 7.5 * 2^e: 7.53125 * 2^e
    raw[:, 4] = _bf16(2.0 ** e)
    codes, scales = f6.encode(raw)
    f = f6.unpack_fields(codes)
    assert scales[0] == e + 127 and f[0, 3] == 31 and f[0, 4] == 8             # a == 7.5 * 2^e: e, code 31; 2^e is 1.0
    if e < 32:
        assert scales[1] == e + 128 and f[1, 3] == 23 and f[1, 4] == 4         # above: e + 1, 3.765625 -> 3.75; 2^e is 0.5
    else:
        assert scales[1] == 32 + 127 and f[1, 3] == 31 and f[1, 4] == 8        # the clamp: y = min(., 7.5)


def test_truth_mantissa_threshold_zero_rows_and_the_exponent_clamps():
    raw, rows, _ = edge_rows()
    codes, scales = f6.encode(raw)
    f = f6.unpack_fields(codes)
    assert scales[rows["m_exact"]] == 127 - 4 - 2 and f[rows["m_exact"], 9] == 31 and f[rows["m_exact"], 10] == 32 | 8     # 7.5, -1.0
    assert scales[rows["m_above"]] == 127 - 4 - 1 and f[rows["m_above"], 9] == 23 and f[rows["m_above"], 10] == 32 | 4    # 3.75, -0.5
    assert scales[rows["max_exact"]] == 130 and scales[rows["max_above"]] == 131
    assert scales[rows["zero"]] == 127 and scales[rows["neg_zero"]] == 127 and not codes[[rows["zero"], rows["neg_zero"]]].any()
    assert scales[rows["subnormal"]] == 127 - 32 and not codes[rows["subnormal"]].any()
    r = rows["clamp_lo"]
    assert scales[r] == 127 - 32 and f[r, :3].tolist() == [16, 0, 1]            # 2.0; -1/16 ties to 0; 1/8
    r = rows["clamp_hi"]
    assert scales[r] == 127 + 32 and f[r, :2].tolist() == [32 | 31, 16]         # saturates at -7.5; 2^33 = 2 * 2^32
    assert scales[rows["max_at_clamp"]] == 127 + 32 and f[rows["max_at_clamp"], 5] == 31
    # f16: its largest finite value (1.999 * 2^15: e = 14, 3.998 -> 4), its smallest normal and subnormals
    raw16 = edge_rows_f16()
    c16, s16 = f6.encode(raw16, f16=True)
    f = f6.unpack_fields(c16)
    assert s16[0] == 127 + 14 and f[0, :2].tolist() == [24, 0]
    assert s16[1] == 127 - 16 and f[1, :3].tolist() == [24, 32 | 16, 0]         # 1023 * 2^-24 = 1.998 * 2^-15: e = -16, 3.996 -> 4; -2.0; 2^-8 -> 0
    assert s16[2] == 127 - 16 and f[2, :2].tolist() == [24, 24]                 # 4.0 and 3.996 -> 4.0
    even = [c if c % 2 == 0 else c + 1 for c in range(31)]
    assert s16[3] == 127 and f[3, 64:96].tolist() == [31] + even and f[3, 96:128].tolist() == [63, 0] + [32 | c for c in even[1:]]


def test_truth_pack_and_unpack_every_field_value_at_every_position():
    for k in range(128):
        fields = np.zeros((64, 128), dtype=np.uint8)
        fields[:, k] = np.arange(64)
        codes = f6.pack_fields(fields)
        assert codes.shape == (64, 96)
        np.testing.assert_array_equal(f6.unpack_fields(codes), fields)
        group = codes[:, 24 * (k // 32):24 * (k // 32) + 24]
        word = sum(group[:, b].astype(object) << (8 * b) for b in range(24))     # the little-endian 24-byte group as an integer
        assert [int(w) for w in word] == [v << (6 * (k % 32)) for v in range(64)]
        assert not np.delete(codes, np.s_[24 * (k // 32):24 * (k // 32) + 24], axis=1).any()
    rng = np.random.default_rng(0)
    fields = rng.integers(0, 64, (50, 128), dtype=np.uint8)
    np.testing.assert_array_equal(f6.unpack_fields(f6.pack_fields(fields)), fields)
    np.testing.assert_array_equal(f6.decode(f6.pack_fields(fields)), np.where(fields >> 5, -1.0, 1.0) * f6.GRID[fields & 31])


def test_truth_scores_order_clamp_and_empty_pages():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 128)) * np.exp2(rng.integers(-6, 6, (40, 1)))
    dc, ds = ft.encode_values(x)
    qc, qs = f6.encode_values(rng.standard_normal((9, 128)))
    d_off = np.array([0, 0, 7, 7, 23, 40, 40])
    q_off = np.array([0, 0, 4, 9])
    clamp0 = np.array([1, 0, 0, 1, 0, 1], dtype=np.uint8)
    M = f6.maxima(qc, qs, dc, ds, d_off, clamp0)
    vq = f6.decode(qc) * np.exp2(qs.astype(np.int64) - 127)[:, None]
    vd = ft.decode(dc) * np.exp2(ds.astype(np.int64) - 127)[:, None]
    Z = vq @ vd.T
    for c in (1, 3, 4):
        m = Z[:, d_off[c]:d_off[c + 1]].max(axis=1)
        np.testing.assert_array_equal(M[:, c].astype(np.float64), np.maximum(m, 0) if clamp0[c] else m)
    S = f6.scores(qc, qs, q_off, dc, ds, d_off, clamp0)
    assert np.isneginf(S[:, [0, 2, 5]]).all()
    assert (S[0, [1, 3, 4]] == 0).all()                           # a query without tokens
    t = np.float32(0)
    for k in range(4, 9):
        t = np.float32(t + M[k, 4])
    assert S[2, 4] == t


# ---------------------------------------------------------------------------------------------------------- contract sanity
def planted(seed=5, n_docs=300, doc_len=64, n_q=20, q_len=32):
    """tools/bench_fde.py: planted_pages, cut down: pages of rows drawn from 48 topics each, queries noisy copies of rows of a page"""
    g = torch.Generator().manual_seed(seed)
    topics = torch.randn((n_docs, 48, 128), generator=g)
    pick = torch.randint(0, 48, (n_docs, doc_len), generator=g)
    rows = torch.gather(topics, 1, pick.unsqueeze(-1).expand(n_docs, doc_len, 128)) + 0.6 * torch.randn((n_docs, doc_len, 128), generator=g)
    pages = torch.nn.functional.normalize(rows, dim=-1).to(torch.bfloat16)
    target = torch.randint(0, n_docs, (n_q,), generator=g)
    tok = torch.randint(0, doc_len, (n_q, q_len), generator=g)
    q = pages[target.unsqueeze(1), tok].float() + 0.8 * torch.randn((n_q, q_len, 128), generator=g) / 128 ** 0.5
    return pages, torch.nn.functional.normalize(q, dim=-1).to(torch.bfloat16)


def test_e2m3_queries_bring_the_first_stage_closer_to_the_exact_score():
    """An inequality between two truths, no threshold: against the float64 MaxSim of the stored bf16 values, the RMS error of the
    first stage over the same FP4 pages is strictly smaller with e2m3 query tokens than with e2m1 ones."""
    pages, q = planted()
    n_docs, doc_len = pages.shape[:2]
    d_raw = ft.raw_bits(pages.reshape(-1, 128))
    off = np.arange(n_docs + 1) * doc_len
    q_blocks = [ft.raw_bits(x) for x in q]
    D = ft.values(d_raw)
    exact = np.stack([(ft.values(b) @ D.T).reshape(-1, n_docs, doc_len).max(axis=2).sum(axis=0) for b in q_blocks])
    s4 = ft.score_blocks(q_blocks, d_raw, off).astype(np.float64)
    s6 = f6.score_blocks(q_blocks, d_raw, off).astype(np.float64)
    rms4, rms6 = np.sqrt(((s4 - exact) ** 2).mean()), np.sqrt(((s6 - exact) ** 2).mean())
    print(f"RMS stage-1 error against the exact score: e2m1 queries {rms4:.4f}, e2m3 queries {rms6:.4f}")
    assert rms6 < rms4


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    with open(os.path.join(ROOT, "include", "maxsim.h")) as f:
        header = f.read()
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    assert "msim_f6_encode_rows(" in header and "msim_f4_scores_q6(" in header

    def rows(dtype=0, x=FAKE, n=40, dim=128, codes=FAKE, scales=FAKE + 3):
        return L.msim_f6_encode_rows(dtype, x, n, dim, codes, scales, None)

    def score(q6=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90,
              dim=128, out=FAKE, ld=10):
        return L.msim_f4_scores_q6(q6, qs, qo, n_q, q_rows, maxq, d4, ds, do, c0, n_d, d_rows, dim, out, ld, None)

    assert rows(n=0) == 0 and rows(n=0, x=None, codes=None, scales=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, q6=None, d4=None, out=None) == 0
    for kw in (dict(n=-1), dict(x=None), dict(codes=None), dict(scales=None), dict(x=FAKE + 8), dict(codes=FAKE + 4)):
        assert rows(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=320), dict(dtype=2), dict(dtype=7)):
        assert rows(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q6=None), dict(qs=None),
               dict(qo=None), dict(d4=None), dict(ds=None), dict(do=None), dict(out=None), dict(q6=FAKE + 4), dict(d4=FAKE + 8),
               dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=320), dict(maxq=(1 << 20) + 1)):
        assert score(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()


# ------------------------------------------------------------------------------------------------------------ the Python layer
def _index(shard):
    from colpali_amd import Fp4Index

    codes, scales = ft.encode(ft.raw_bits(shard.blob), f16=shard.blob.dtype == torch.float16)
    return Fp4Index(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                    shard.id_base)


def _truth_fn(queries, index):
    """the e2m3 truth as a stage-1 hook: (queries, Fp4Index) -> fp32 [n_q, len(index)]"""
    qb = [ft.raw_bits(x.to(torch.bfloat16)) for x in queries]
    qc, qs = f6.encode(np.concatenate(qb))
    q_off = np.cumsum([0] + [len(x) for x in qb])
    c0 = None if index.clamp0 is None else index.clamp0.numpy()
    return torch.from_numpy(f6.scores(qc, qs, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), c0))


def _shard(n=5, rows=3, id_base=7):
    import colpali_amd

    return colpali_amd.pack_passages([torch.randn(rows, 128).to(torch.bfloat16) for _ in range(n)], torch.device("cpu"), batch_size=None,
                                     id_base=id_base)


def test_exports_and_python_refusals_without_a_gpu():
    import colpali_amd
    from colpali_amd import retrieval

    for name in ("fp6_scores", "fp6_quantize_queries", "fp4_scores_from_codes"):
        assert name in colpali_amd.__all__ and hasattr(colpali_amd, name)
    assert "fp6_scores" in colpali_amd.__doc__
    assert colpali_amd.fp6_scores in retrieval._KERNELS            # a retriever packs the queries once for it
    idx = _index(_shard())
    q = torch.randn(2, 4, 128).to(torch.bfloat16)
    off = torch.tensor([0, 4, 8], dtype=torch.int32)
    scales = torch.zeros(8, dtype=torch.uint8)
    for bad in ("e3m2", "fp6", "", None):
        with pytest.raises(ValueError, match="query_code must be"):
            colpali_amd.fp4_scores(q, idx, query_code=bad)
        with pytest.raises(ValueError, match="query_code must be"):
            colpali_amd.fp4_scores_from_codes(torch.zeros(8, 96, dtype=torch.uint8), scales, off, 4, idx, query_code=bad)
    with pytest.raises(ValueError, match=r"e2m3 query codes must be a contiguous uint8 \[tokens, 96\]"):
        colpali_amd.fp4_scores_from_codes(torch.zeros(8, 64, dtype=torch.uint8), scales, off, 4, idx, query_code="e2m3")
    with pytest.raises(ValueError, match=r"e2m1 query codes must be a contiguous uint8 \[tokens, 64\]"):
        colpali_amd.fp4_scores_from_codes(torch.zeros(8, 96, dtype=torch.uint8), scales, off, 4, idx)
    with pytest.raises(TypeError):
        colpali_amd.fp4_scores(q, idx, None, "e2m3")               # query_code is keyword-only


def test_the_hook_given_as_fp4_score_fn_is_the_stage_that_runs():
    import colpali_amd
    from oracle import topk_oracle

    shard = _shard(n=6, rows=4)
    idx = _index(shard)
    calls = []

    def stage1(q, i):
        calls.append("f6")
        return _truth_fn(q, i)

    def rerank_fn(queries, corpus, candidates):
        calls.append("rr")
        return torch.zeros(candidates.shape), candidates

    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), fp4_score_fn=stage1, rerank_fn=rerank_fn,
                                     select=topk_oracle.torch_select)
    s, i = r.search(torch.randn(2, 4, 128).to(torch.bfloat16), k=2, prefilter=idx, n_candidates=3)
    assert calls == ["f6", "rr"] and i.shape == (2, 2) and (i >= 7).all()


# ------------------------------------------------------------------------------------------------------------------ sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_docs, k, m, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    g = torch.Generator().manual_seed(11)
    lens = torch.randint(0, 40, (n_docs,), generator=g).tolist()
    docs = [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        n = full.shape[1]
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < n)
        got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0))) if n else torch.zeros(candidates.shape)
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn, fp4_score_fn=_truth_fn)
    ps, pi = r.search(q, k=k, prefilter=_index(shard), n_candidates=m)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth
        full = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None)
        _, coarse_ids = topk_oracle.topk(_truth_fn(q, _index(full)).numpy(), m)
        s, i = rerank_fn(q, full, torch.from_numpy(coarse_ids))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), ps=tps, pi=tpi)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12)])
def test_sharded_search_with_the_e2m3_stage_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
