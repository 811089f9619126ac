"""The 320-wide FP4 index without a GPU: the truth helper (tests/fp4_wide_truth.py) on its own edge cases, the ABI's argument
checks (no device work; the old 128-wide entries still refuse 320 and the new ones 128), the Python class's refusals, exports,
ShardedRetriever.search(prefilter=<Fp4WideIndex>) plumbing over gloo worlds of 2 and 3 with the truth injected as
fp4_wide_score_fn (every rank must get the unsharded answer), and a save / verify_file / range-load round trip of a hand-made
index."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fp4_wide_truth as wt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
OLD_PREFILTER_TEXT = "prefilter must be a PackedCorpus, an FdeIndex, an Int8Index, a CentroidIndex or a BinaryIndex"
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def _row(**at):
    x = np.zeros((1, 320))
    for k, v in at.items():
        x[0, int(k[1:])] = v
    return x


def _bf16(v):
    return int(wt.raw_bits(torch.tensor([[v]], dtype=torch.bfloat16))[0, 0])


# ------------------------------------------------------------------------------------------------------------ the truth helper
@pytest.mark.parametrize("at", [0, 120, 250, 300])
def test_truth_every_tie_goes_to_the_even_code(at):
    """a row whose maximum is 6 (e = 0) beside every midpoint of the grid, both signs, in every K block"""
    x = np.zeros((1, 320))
    x[0, at] = 6.0
    x[0, at + 1:at + 8] = TIES
    x[0, at + 8:at + 15] = [-t for t in TIES]
    codes, scales = wt.encode_values(x)
    assert scales[0] == 127 and codes.shape == (1, 160)
    nib = wt.unpack_nibbles(codes)[0]
    assert nib[at] == 7
    assert nib[at + 1:at + 8].tolist() == [0, 2, 2, 4, 4, 6, 6]                       # values 0, 1, 1, 2, 2, 4, 4
    assert nib[at + 8:at + 15].tolist() == [0, 8 | 2, 8 | 2, 8 | 4, 8 | 4, 8 | 6, 8 | 6]   # -0.25 rounds to code 0: nibble 0, not 8
    assert not np.delete(nib, np.arange(at, at + 15)).any()
    np.testing.assert_array_equal(wt.decode(codes)[0, at:at + 15], [6, 0, 1, 1, 2, 2, 4, 4, 0, -1, -1, -2, -2, -4, -4])
    eps = 2.0 ** -8                                                                    # just off a tie, the nearer value wins
    near = np.zeros((1, 320))
    near[0, at] = 6.0
    near[0, at + 1:at + 5] = [0.25 + eps, 0.75 - eps, 2.5 + eps, 5.0 + eps]
    assert wt.unpack_nibbles(wt.encode_values(near)[0])[0, at + 1:at + 5].tolist() == [1, 1, 5, 7]


def test_truth_codes_of_is_the_search_for_the_nearest_grid_value():
    from tests.fp4_truth import GRID, nearest_codes

    rng = np.random.default_rng(1)
    edge = np.concatenate([GRID, wt.MIDS])
    y = np.concatenate([edge, np.nextafter(edge, 7.0), np.nextafter(edge, -1.0), rng.uniform(0, 6, 20000)]).clip(0, 6)
    np.testing.assert_array_equal(wt.codes_of(y), nearest_codes(y))
    assert wt.codes_of(wt.MIDS).tolist() == [0, 2, 2, 4, 4, 6, 6] and wt.MIDS.tolist() == [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]


def test_truth_dimension_k_is_nibble_k_and_1_of_byte_k_shr_1_of_160():
    x = _row(k0=6.0, k5=-1.0, k6=0.5, k127=3.0, k128=-2.0, k255=1.5, k256=4.0, k319=-6.0)
    codes, _ = wt.encode_values(x)
    want = np.zeros((1, 160), dtype=np.uint8)
    want[0, 0] = 7                       # k = 0: low nibble of byte 0
    want[0, 2] = (8 | 2) << 4            # k = 5: high nibble of byte 2
    want[0, 3] = 1                       # k = 6: low nibble of byte 3
    want[0, 63] = 5 << 4                 # k = 127: the last nibble of K block 0
    want[0, 64] = 8 | 4                  # k = 128: the first nibble of K block 1
    want[0, 127] = 3 << 4                # k = 255
    want[0, 128] = 6                     # k = 256: the first nibble of K block 2
    want[0, 159] = (8 | 7) << 4          # k = 319
    np.testing.assert_array_equal(codes, want)
    np.testing.assert_array_equal(wt.pack_nibbles(wt.unpack_nibbles(codes)), codes)


def test_truth_one_scale_per_row_from_a_maximum_in_dimensions_256_to_319():
    """the maximum lies only in the third K block: it sets the one scale of the whole row"""
    x = np.zeros((2, 320))
    x[0, 3], x[0, 130], x[0, 300] = 1.0, -2.0, 48.0                  # 48 = 6 * 2^3
    x[1, 3], x[1, 130] = 1.0, -2.0                                   # the same row without it
    codes, scales = wt.encode_values(x)
    nib = wt.unpack_nibbles(codes)
    assert scales.tolist() == [130, 126]                             # e = 3; e = -1 (2 <= 6 * 2^-1)
    assert nib[0, 300] == 7 and nib[0, 130] == 0 and nib[0, 3] == 0   # -2 / 8 = -0.25 ties to 0 (nibble 0); 1 / 8 rounds to 0
    assert nib[1, 130] == (8 | 6) and nib[1, 3] == 4                 # 2 * 2 = 4.0 -> code 6; 1 * 2 = 2.0 -> code 4


@pytest.mark.parametrize("e", [-32, -7, 0, 3, 32])
def test_truth_exponent_at_a_maximum_of_six_and_one_ulp_above(e):
    raw = np.zeros((2, 320), dtype=np.uint16)
    raw[0, 290] = _bf16(6.0 * 2.0 ** e)
    raw[1, 290] = raw[0, 290] + 1                                    # one bf16 ulp above 6 * 2^e
    raw[:, 4] = _bf16(2.0 ** e)
    codes, scales = wt.encode(raw)
    nib = wt.unpack_nibbles(codes)
    assert scales[0] == e + 127 and nib[0, 290] == 7 and nib[0, 4] == 2         # a == 6 * 2^e: e, code 7; 2^e is 1.0
    if e < 32:
        assert scales[1] == e + 128 and nib[1, 290] == 5 and nib[1, 4] == 1     # above: e + 1, 3.0117 -> 3; 2^e is 0.5
    else:
        assert scales[1] == 32 + 127 and nib[1, 290] == 7 and nib[1, 4] == 2    # the clamp: y = min(., 6)


def test_truth_zero_rows_negative_zero_subnormals_and_the_exponent_clamps():
    raw = np.zeros((5, 320), dtype=np.uint16)
    raw[1, :] = 0x8000                                               # a row of -0.0
    raw[2, 0], raw[2, 319] = 0x0001, 0x8001                          # bf16 subnormals only: far below 6 * 2^-32
    raw[3, 200] = _bf16(2.0 ** -31)                                  # 2^-31 = 2 * 2^-32
    raw[3, 1] = _bf16(-(2.0 ** -34))                                 # 0.25 * 2^-32: the tie to 0
    raw[4, 310] = _bf16(-(2.0 ** 40))                                # above 6 * 2^32: saturates at -6
    raw[4, 1] = _bf16(2.0 ** 33)
    codes, scales = wt.encode(raw)
    nib = wt.unpack_nibbles(codes)
    assert scales.tolist() == [127, 127, 127 - 32, 127 - 32, 127 + 32]
    assert not codes[:3].any()
    assert nib[3, 200] == 4 and nib[3, 1] == 0
    assert nib[4, 310] == (8 | 7) and nib[4, 1] == 4
    raw16 = np.zeros((1, 320), dtype=np.uint16)                      # f16: its largest finite value and its smallest subnormal
    raw16[0, 300], raw16[0, 1] = 0x7bff, 0x0001
    c16, s16 = wt.encode(raw16, f16=True)
    assert s16[0] == 127 + 14 and wt.unpack_nibbles(c16)[0, [300, 1]].tolist() == [6, 0]   # 65504 = 3.998 * 2^14


def test_truth_scores_order_clamp_and_empty_pages():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 320)) * np.exp2(rng.integers(-6, 6, (40, 1)))
    dc, ds = wt.encode_values(x)
    q = rng.standard_normal((9, 320))
    qc, qs = wt.encode_values(q)
    d_off = np.array([0, 0, 7, 7, 23, 40, 40])
    q_off = np.array([0, 0, 4, 9])
    clamp0 = np.array([1, 0, 0, 1, 0, 1], dtype=np.uint8)
    M = wt.maxima(qc, qs, dc, ds, d_off, clamp0)
    vq = wt.decode(qc) * np.exp2(qs.astype(np.int64) - 127)[:, None]
    vd = wt.decode(dc) * np.exp2(ds.astype(np.int64) - 127)[:, None]
    Z = vq @ vd.T
    for c in (1, 3, 4):
        m = Z[:, d_off[c]:d_off[c + 1]].max(axis=1)
        np.testing.assert_array_equal(M[:, c].astype(np.float64), np.maximum(m, 0) if clamp0[c] else m)
    S = wt.scores(qc, qs, q_off, dc, ds, d_off, clamp0)
    assert np.isneginf(S[:, [0, 2, 5]]).all()
    assert (S[0, [1, 3, 4]] == 0).all()                              # a query without tokens
    t = np.float32(0)
    for k in range(4, 9):
        t = np.float32(t + M[k, 4])
    assert S[2, 4] == t
    # the largest sum: 320 products of 6 * 6, a float32
    full = wt.pack_nibbles(np.full((1, 320), 7))
    assert wt.maxima(full, np.array([127], np.uint8), wt.pack_nibbles(np.full((1, 320), 15)), np.array([127], np.uint8), [0, 1])[0, 0] == -11520


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def rows(dtype=0, x=FAKE, n=40, dim=320, codes=FAKE, scales=FAKE + 3):
        return L.msim_f4w_encode_rows(dtype, x, n, dim, codes, scales, None)

    def score(q4=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90,
              dim=320, out=FAKE, ld=10):
        return L.msim_f4w_scores(q4, qs, qo, n_q, q_rows, maxq, d4, ds, do, c0, n_d, d_rows, dim, out, ld, None)

    assert rows(n=0) == 0 and rows(n=0, x=None, codes=None, scales=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, q4=None, d4=None, out=None) == 0
    for kw in (dict(n=-1), dict(x=None), dict(codes=None), dict(scales=None), dict(x=FAKE + 8), dict(codes=FAKE + 4)):
        assert rows(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(dim=160), dict(dtype=2), dict(dtype=7)):
        assert rows(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q4=None), dict(qs=None),
               dict(qo=None), dict(d4=None), dict(ds=None), dict(do=None), dict(out=None), dict(q4=FAKE + 4), dict(d4=FAKE + 8),
               dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(maxq=(1 << 20) + 1)):
        assert score(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    assert L.msim_f4w_scores_plan(4, 32, 10, 90, None) == EINVAL and L.msim_f4w_scores_plan(-1, 32, 10, 90, FAKE) == EINVAL
    assert L.msim_f4w_scores_plan(4, -1, 10, 90, FAKE) == EINVAL and L.msim_f4w_scores_plan(4, 32, 10, -1, FAKE) == EINVAL


def test_the_128_wide_entries_still_refuse_width_320():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_f4_encode_rows(0, FAKE, 40, 320, FAKE, FAKE + 3, None) == EUNSUPPORTED
    assert L.msim_f6_encode_rows(0, FAKE, 40, 320, FAKE, FAKE + 3, None) == EUNSUPPORTED
    for name in ("msim_f4_scores", "msim_f4_scores_q6"):
        rc = getattr(L, name)(FAKE, FAKE + 1, FAKE, 4, 40, 32, FAKE, FAKE + 5, FAKE, None, 10, 90, 320, FAKE, 10, None)
        assert rc == EUNSUPPORTED, name
    with pytest.raises(NotImplementedError, match="the fp4 index takes bfloat16 / float16 pages of width 128"):
        colpali_amd.Fp4Index.build(_shard())


# ------------------------------------------------------------------------------------------------------------ the Python class
def _index(shard):
    from colpali_amd import Fp4WideIndex

    codes, scales = wt.encode(wt.raw_bits(shard.blob), f16=shard.blob.dtype == torch.float16)
    return Fp4WideIndex(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                        shard.id_base)


def _truth_fn(queries, index):
    qb = [wt.raw_bits(x.to(torch.bfloat16)) for x in queries]
    qc, qs = wt.encode(np.concatenate(qb))
    q_off = np.cumsum([0] + [len(x) for x in qb])
    c0 = None if index.clamp0 is None else index.clamp0.numpy()
    return torch.from_numpy(wt.scores(qc, qs, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), c0))


def _shard(n=5, rows=3, width=320, dtype=torch.bfloat16, id_base=7):
    import colpali_amd

    return colpali_amd.pack_passages([torch.randn(rows, width).to(dtype) for _ in range(n)], torch.device("cpu"), batch_size=None,
                                     id_base=id_base)


def test_class_refusals_and_exports_without_a_gpu():
    import colpali_amd
    from colpali_amd import Fp4WideIndex

    shard = _shard()
    idx = _index(shard)
    assert len(idx) == 5 and idx.device == torch.device("cpu") and idx.nbytes == 15 * 161 + 6 * 4 and idx.id_base == 7
    for name in ("Fp4WideIndex", "fp4_wide_scores", "fp4_wide_scores_from_codes", "fp4_wide_quantize_queries"):
        assert name in colpali_amd.__all__ and hasattr(colpali_amd, name)
    assert "Fp4WideIndex" in colpali_amd.__doc__
    for codes in (torch.zeros(15, 160, dtype=torch.int8), torch.zeros(15, 64, dtype=torch.uint8), torch.zeros(15, 320, dtype=torch.uint8),
                  torch.zeros(15 * 160, dtype=torch.uint8), torch.zeros(160, 15, dtype=torch.uint8).t()):
        with pytest.raises(ValueError, match="codes must be"):
            Fp4WideIndex(codes, idx.scales, shard.offsets, None, shard.lengths)
    for scales in (torch.zeros(15, dtype=torch.int8), torch.zeros(14, dtype=torch.uint8), torch.zeros(15, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="scales must be"):
            Fp4WideIndex(idx.codes, scales, shard.offsets, None, shard.lengths)
    with pytest.raises(ValueError, match="offsets must be"):
        Fp4WideIndex(idx.codes, idx.scales, shard.offsets[:-1], None, shard.lengths)
    with pytest.raises(ValueError, match="clamp0 must be"):
        Fp4WideIndex(idx.codes, idx.scales, shard.offsets, torch.zeros(4, dtype=torch.uint8), shard.lengths)
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 pages of width 320.*Fp4Index"):
        Fp4WideIndex.build(_shard(width=128))
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 pages of width 320"):
        Fp4WideIndex.build(_shard(width=64))
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 pages of width 320"):
        Fp4WideIndex.build(_shard(dtype=torch.float32))
    with pytest.raises(TypeError, match="Fp4WideIndex"):
        colpali_amd.fp4_wide_scores([torch.zeros(2, 320, dtype=torch.bfloat16)], shard)
    with pytest.raises(ValueError, match="query codes must be"):
        colpali_amd.fp4_wide_scores_from_codes(torch.zeros(4, 64, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8),
                                               torch.tensor([0, 4], dtype=torch.int32), 4, idx)


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd

    shard = _shard()
    calls = []
    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), fp4_score_fn=lambda q, i: calls.append("f4"),
                                     fp4_wide_score_fn=lambda q, i: calls.append("f4w"), rerank_fn=lambda q, c, x: calls.append("rr"))
    q = torch.randn(2, 4, 320).to(torch.bfloat16)
    for idx in (_index(_shard(n=4)), _index(_shard(id_base=6))):
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=_index(shard))
    with pytest.raises(ValueError) as exc:
        r.search(q, prefilter=torch.zeros(5, 160, dtype=torch.uint8), n_candidates=3)
    assert str(exc.value).startswith(OLD_PREFILTER_TEXT) and "Fp4WideIndex" in str(exc.value)
    assert calls == []


def test_the_wide_fp4_hook_is_the_stage_that_runs():
    import colpali_amd
    from colpali_amd import retrieval
    from oracle import topk_oracle

    assert colpali_amd.fp4_wide_scores in retrieval._KERNELS
    shard = _shard(n=6, rows=4)
    idx = _index(shard)
    calls = []

    def stage1(q, i):
        calls.append("f4w")
        return _truth_fn(q, i)

    def rerank_fn(queries, corpus, candidates):
        calls.append("rr")
        return torch.zeros(candidates.shape), candidates

    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), binary_score_fn=lambda q, i: calls.append("bin"),
                                     fp4_score_fn=lambda q, i: calls.append("f4"), fp4_wide_score_fn=stage1, rerank_fn=rerank_fn,
                                     select=topk_oracle.torch_select)
    s, i = r.search(torch.randn(2, 4, 320).to(torch.bfloat16), k=2, prefilter=idx, n_candidates=3)
    assert calls == ["f4w", "rr"] and i.shape == (2, 2) and (i >= 7).all()


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
    docs = [torch.nn.functional.normalize(torch.randn(n, 320, generator=g), dim=-1).to(torch.bfloat16) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, 320, generator=g), dim=-1).to(torch.bfloat16)

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
                                     rerank_fn=rerank_fn, fp4_wide_score_fn=_truth_fn)
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


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12), (3, 8, 10, 4)])
def test_sharded_wide_fp4_prefilter_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")


# --------------------------------------------------------------------------------------------------------------- persistence
def test_save_and_verify_file_round_trip_of_a_hand_made_index(tmp_path):
    import colpali_amd

    shard = _shard(n=6, rows=5)
    shard.clamp0 = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.uint8)
    idx = _index(shard)
    path = tmp_path / "index.msim"
    idx.save(path)
    info = colpali_amd.verify_file(path)
    assert info["kind"] == "Fp4WideIndex"
    back = colpali_amd.Fp4WideIndex.load(path, torch.device("cpu"))
    assert isinstance(back, colpali_amd.Fp4WideIndex) and back.id_base == 7
    for name in ("codes", "scales", "offsets", "clamp0", "lengths"):
        assert torch.equal(getattr(back, name), getattr(idx, name)), name
    part = colpali_amd.load(path, torch.device("cpu"), pages=(2, 5))
    assert isinstance(part, colpali_amd.Fp4WideIndex) and len(part) == 3 and part.id_base == 9
    assert torch.equal(part.codes, idx.codes[10:25]) and torch.equal(part.scales, idx.scales[10:25])
    assert part.offsets.tolist() == [0, 5, 10, 15] and torch.equal(part.clamp0, idx.clamp0[2:5])
    with pytest.raises(colpali_amd.ShardFileError, match="holds a Fp4WideIndex"):
        colpali_amd.Fp4Index.load(path, torch.device("cpu"))
