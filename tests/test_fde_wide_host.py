"""Fixed dimensional encodings at width 320 without a GPU: properties of the float64 truth (tests/fde_wide_truth.py), the parameter
draw of FdeConfig.params(width=), the argument checks of msim_fdew_* (no device work), FdeWideIndex's persistence on the CPU, the
retriever's checks with no hook called, and ShardedRetriever.search(prefilter=<FdeWideIndex>) over gloo worlds of 2 and 3 with the
truth injected as fde_wide_score_fn.  Every rank must get the unsharded answer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from colpali_amd import FdeWideIndex, fde_wide_scores  # noqa: F401  (what this module is about: nothing here runs without them)
from tests import fde_wide_truth as ft

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

W = 320
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
OLD_PREFILTER_TEXT = ("prefilter must be a PackedCorpus, an FdeIndex, an Int8Index, a CentroidIndex or a BinaryIndex, or an Fp4Index or an "
                      "Fp4WideIndex")


# ------------------------------------------------------------------------------------------------------------------ the truth
def test_projection_is_linear():
    rng = np.random.default_rng(0)
    G, S = ft.params(3, 2, 16, 1)
    assert G.shape == (3, 2, W) and S.shape == (3, 16, W)
    x, y = rng.standard_normal(W), rng.standard_normal(W)
    np.testing.assert_allclose(ft.psi(2.5 * x - 0.75 * y, S[1]), 2.5 * ft.psi(x, S[1]) - 0.75 * ft.psi(y, S[1]), rtol=1e-12, atol=1e-12)
    assert set(np.unique(S)) == {-1.0, 1.0}


def test_fill_empty_takes_the_lowest_index_nearest_row():
    rng = np.random.default_rng(1)
    G, S = ft.params(1, 3, 8, 2)
    X = rng.standard_normal((4, W))
    phi = np.array([[5], [6], [3], [4]])          # bucket 7: rows 0, 1, 2 at distance 1, row 3 at distance 2
    enc = ft.encode(X, G, S, doc=True, fill_empty=True, phi=phi).reshape(8, 8)
    np.testing.assert_allclose(enc[7], ft.psi(X[0], S[0]))
    np.testing.assert_allclose(enc[0], ft.psi(X[3], S[0]))    # bucket 0: row 3 (distance 1) beats rows 1, 2 (distance 2)
    np.testing.assert_allclose(enc[2], ft.psi(X[1], S[0]))    # bucket 2: rows 1, 2 at distance 1, row 1 first
    assert ft.nearest_row(np.array([3, 1, 1]), 0) == 1
    plain = ft.encode(X, G, S, doc=True, fill_empty=False, phi=phi).reshape(8, 8)
    assert (plain[[0, 1, 2, 7]] == 0).all()
    np.testing.assert_allclose(plain[5], ft.psi(X[0], S[0]))


def test_page_mean_and_query_sum():
    rng = np.random.default_rng(2)
    G, S = ft.params(2, 2, 8, 3)
    X = rng.standard_normal((3, W))
    phi = np.array([[1, 0], [1, 2], [3, 0]])
    d = ft.encode(X, G, S, doc=True, fill_empty=False, phi=phi).reshape(2, 4, 8)
    q = ft.encode(X, G, S, doc=False, phi=phi).reshape(2, 4, 8)
    np.testing.assert_allclose(d[0, 1], ft.psi((X[0] + X[1]) / 2, S[0]))
    np.testing.assert_allclose(q[0, 1], ft.psi(X[0] + X[1], S[0]))
    np.testing.assert_allclose(q[1, 0], ft.psi(X[0] + X[2], S[1]))
    assert (ft.encode(np.zeros((0, W)), G, S, doc=True) == 0).all()


@pytest.mark.parametrize("seed", range(4))
def test_one_token_against_one_row(seed):
    rng = np.random.default_rng(seed)
    G, S = ft.params(6, 3, 16, seed)
    q, p = rng.standard_normal(W), rng.standard_normal(W)
    cq, cp = ft.codes(q[None], G)[0], ft.codes(p[None], G)[0]
    terms = np.array([ft.psi(q, S[r]) @ ft.psi(p, S[r]) for r in range(6)])
    fq = ft.encode(q[None], G, S, doc=False)
    assert abs(fq @ ft.encode(p[None], G, S, doc=True, fill_empty=False) - (terms * (cq == cp)).sum()) < 1e-9
    assert abs(fq @ ft.encode(p[None], G, S, doc=True, fill_empty=True) - terms.sum()) < 1e-9


# ------------------------------------------------------------------------------------------------------------------ parameters
def test_wide_parameters_equal_the_truths_draw_and_the_default_is_unchanged():
    from colpali_amd import FdeConfig

    cfg = FdeConfig(reps=8, ksim=2, dproj=8, seed=9)
    G, S = cfg.params(width=320)
    tG, tS = ft.params(8, 2, 8, 9)
    assert G.dtype == torch.float32 and S.dtype == torch.float32 and G.shape == (8, 2, W) and S.shape == (8, 8, W)
    np.testing.assert_array_equal(G.double().numpy(), tG)
    np.testing.assert_array_equal(S.double().numpy(), tS)
    # the default call: width 128, the bits of the draw tests/fde_truth.py pins (restated here: G then S from one generator)
    g = torch.Generator().manual_seed(9)
    G0 = torch.randn((8, 2, 128), generator=g, dtype=torch.float32)
    S0 = torch.randint(0, 2, (8, 8, 128), generator=g, dtype=torch.int64).to(torch.float32) * 2 - 1
    for got in (cfg.params(), cfg.params(128), cfg.params(width=128)):
        assert got[0].shape == (8, 2, 128) and got[1].shape == (8, 8, 128)
        assert torch.equal(got[0].view(torch.int32), G0.view(torch.int32)) and torch.equal(got[1].view(torch.int32), S0.view(torch.int32))
    for bad in (64, 0, 321, True, None):
        with pytest.raises(ValueError):
            cfg.params(width=bad)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _enc(L, fn, dtype=0, x=FAKE, off=FAKE, n=3, rows=40, dim=W, G=FAKE, S=FAKE, reps=20, ksim=5, dproj=16, fill=1, out=FAKE,
         codes=None):
    if fn == "docs":
        return L.msim_fdew_encode_docs(dtype, x, off, n, rows, dim, G, S, reps, ksim, dproj, fill, out, codes, None)
    return L.msim_fdew_encode_queries(dtype, x, off, n, rows, dim, G, S, reps, ksim, dproj, out, codes, None)


@pytest.mark.parametrize("fn", ["docs", "queries"])
def test_wide_encoder_abi_refuses_bad_arguments_before_device_work(fn):
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    assert _enc(L, fn, n=0) == 0                                   # nothing to do: no pointer is looked at
    bad = [dict(n=-1), dict(rows=-1), dict(reps=0), dict(x=None), dict(off=None), dict(G=None), dict(S=None), dict(out=None),
           dict(x=FAKE + 8), dict(out=FAKE + 1)]
    if fn == "docs":
        bad.append(dict(fill=2))
    for kw in bad:
        assert _enc(L, fn, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=64), dict(dim=128), dict(dim=321), dict(ksim=0), dict(ksim=7), dict(dproj=12),
               dict(dproj=128), dict(reps=1, ksim=1, dproj=8), dict(reps=17, ksim=6, dproj=64), dict(reps=3, ksim=2, dproj=8)):
        assert _enc(L, fn, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    assert _enc(L, fn, dim=128, n=0) == EUNSUPPORTED               # the width is refused even where nothing would run


# ------------------------------------------------------------------------------------------------------------------ persistence
def _index(amd, n=6, id_base=11):
    cfg = amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=9, fill_empty=False)
    G, S = cfg.params(width=320)
    g = torch.Generator().manual_seed(4)
    Fd = torch.randn(n, cfg.dim, generator=g).to(torch.bfloat16)
    return amd.FdeWideIndex(Fd, id_base, cfg, params=(G + 1.0, S))             # NOT what the seed would re-draw


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8))


def test_persistence_round_trip_on_the_cpu(tmp_path):
    import colpali_amd as amd

    idx = _index(amd)
    path = str(tmp_path / "w.msim")
    idx.save(path, chunk_bytes=4096)
    header = amd.verify_file(path)
    assert header["kind"] == "FdeWideIndex" and header["abi"] == 22
    for got in (amd.load(path, "cpu"), amd.FdeWideIndex.load(path, "cpu", verify=False)):
        assert type(got) is amd.FdeWideIndex and got.id_base == 11 and got.config == idx.config and len(got) == 6
        assert _same_bits(got.Fd, idx.Fd) and _same_bits(got.params[0], idx.params[0]) and _same_bits(got.params[1], idx.params[1])
        assert not torch.equal(got.params[0], idx.config.params(width=320)[0])  # the file, not the seed
    part = amd.load(path, "cpu", pages=(1, 4))
    assert type(part) is amd.FdeWideIndex and part.id_base == 12 and len(part) == 3 and part.config == idx.config
    assert _same_bits(part.Fd, idx.Fd[1:4]) and _same_bits(part.params[0], idx.params[0]) and _same_bits(part.params[1], idx.params[1])
    for other in (amd.FdeIndex, amd.Fp4WideIndex, amd.BinaryIndex):            # the wrong class is refused, the sibling included
        with pytest.raises(amd.ShardFileError, match="not a"):
            other.load(path, "cpu")
    narrow = amd.FdeIndex(torch.zeros(2, idx.config.dim), 0, idx.config)
    narrow.save(str(tmp_path / "n.msim"))
    with pytest.raises(amd.ShardFileError, match="not a"):
        amd.FdeWideIndex.load(str(tmp_path / "n.msim"), "cpu")


def test_index_constructor_checks():
    import colpali_amd as amd

    cfg = amd.FdeConfig(reps=2, ksim=3, dproj=16)
    with pytest.raises(ValueError):
        amd.FdeWideIndex(torch.zeros(5, cfg.dim + 1), 7, cfg)
    with pytest.raises(ValueError, match="params"):
        amd.FdeWideIndex(torch.zeros(5, cfg.dim), 7, cfg, params=cfg.params())  # the 128-wide draw
    idx = amd.FdeWideIndex(torch.zeros(5, cfg.dim), 7, cfg)
    assert idx.params[0].shape == (2, 3, W) and idx.params[1].shape == (2, 16, W) and idx.count == 5 and idx.id_base == 7


# ------------------------------------------------------------------------------------------------------------------ the retriever
def _shard(amd, width, n=5, id_base=7):
    return amd.pack_passages([torch.randn(3, width).to(torch.bfloat16) for _ in range(n)], torch.device("cpu"), batch_size=None,
                             id_base=id_base)


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd as amd

    cfg = amd.FdeConfig(reps=2, ksim=3, dproj=16)
    calls = []
    hooks = dict(score_fn=lambda q, c: calls.append("score"), fde_score_fn=lambda q, i: calls.append("fde"),
                 fde_wide_score_fn=lambda q, i: calls.append("fdew"), rerank_fn=lambda q, c, x: calls.append("rr"))
    r = amd.ShardedRetriever(_shard(amd, W), **hooks)
    q = torch.randn(2, 4, W).to(torch.bfloat16)
    for idx in (amd.FdeWideIndex(torch.zeros(4, cfg.dim), 7, cfg), amd.FdeWideIndex(torch.zeros(5, cfg.dim), 6, cfg)):
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    good = amd.FdeWideIndex(torch.zeros(5, cfg.dim), 7, cfg)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=good)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=good, n_candidates=0)
    with pytest.raises(ValueError, match="not both"):
        r.search(q, prefilter=good, n_candidates=3, candidates=torch.zeros(2, 3, dtype=torch.int64))
    with pytest.raises(ValueError) as e:
        r.search(q, prefilter=torch.zeros(5, cfg.dim), n_candidates=3)
    assert str(e.value).startswith(OLD_PREFILTER_TEXT) and "FdeWideIndex" in str(e.value)[len(OLD_PREFILTER_TEXT):]
    # the other width than the shard's, both ways
    with pytest.raises(ValueError, match="320 wide"):
        r.search(q, prefilter=amd.FdeIndex(torch.zeros(5, cfg.dim), 7, cfg), n_candidates=3)
    r128 = amd.ShardedRetriever(_shard(amd, 128), **hooks)
    with pytest.raises(ValueError, match="128 wide"):
        r128.search(torch.randn(2, 4, 128).to(torch.bfloat16), prefilter=good, n_candidates=3)
    assert calls == []
    assert amd.fde_wide_scores in amd.retrieval._KERNELS


# ------------------------------------------------------------------------------------------------------------------ gloo worlds
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

    cfg = colpali_amd.FdeConfig(reps=4, ksim=3, dproj=16, seed=11)
    G, S = ft.params(cfg.reps, cfg.ksim, cfg.dproj, cfg.seed)
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(0, 40, (n_docs,), generator=g).tolist()
    docs = [torch.nn.functional.normalize(torch.randn(n, W, generator=g), dim=-1).to(torch.bfloat16) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, W, generator=g), dim=-1).to(torch.bfloat16)

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        n = full.shape[1]
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < n)
        got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0))) if n else torch.zeros(candidates.shape)
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    def index_of(corpus):
        Fd = ft.encode_all(corpus.blob.float().numpy(), corpus.offsets.numpy(), G, S, doc=True, fill_empty=cfg.fill_empty)
        return colpali_amd.FdeWideIndex(torch.from_numpy(Fd).float().contiguous(), corpus.id_base, cfg)

    def fde_wide_score_fn(queries, index):
        Fq = np.stack([ft.encode(x.float().numpy(), G, S, doc=False) for x in queries])
        return torch.from_numpy(Fq @ index.Fd.double().numpy().T).float()

    def narrow(queries, index):
        raise AssertionError("the 128-wide hook was called for an FdeWideIndex")

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn, fde_score_fn=narrow, fde_wide_score_fn=fde_wide_score_fn)
    ps, pi = r.search(q, k=k, prefilter=index_of(shard), n_candidates=m)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth
        full = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None)
        _, coarse_ids = topk_oracle.topk(fde_wide_score_fn(q, index_of(full)).numpy(), m)
        s, i = rerank_fn(q, full, torch.from_numpy(coarse_ids))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), ps=tps, pi=tpi)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12), (3, 8, 10, 4)])
def test_sharded_fde_wide_prefilter_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
