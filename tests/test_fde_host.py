"""Fixed dimensional encodings without a GPU: properties of the float64 truth (tests/fde_truth.py), the ABI's argument checks (no
device work), FdeConfig's checks, and ShardedRetriever.search(prefilter=<FdeIndex>) over gloo worlds of 2 and 3 with the truth
injected as fde_score_fn.  Every rank must get the unsharded answer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fde_truth as ft

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def test_projection_is_linear():
    rng = np.random.default_rng(0)
    _, S = ft.params(3, 2, 16, 1)
    x, y = rng.standard_normal(128), rng.standard_normal(128)
    np.testing.assert_allclose(ft.psi(2.5 * x - 0.75 * y, S[1]), 2.5 * ft.psi(x, S[1]) - 0.75 * ft.psi(y, S[1]), rtol=1e-12, atol=1e-12)
    assert set(np.unique(S)) == {-1.0, 1.0}


def test_fill_empty_takes_the_lowest_index_nearest_row():
    rng = np.random.default_rng(1)
    G, S = ft.params(1, 3, 8, 2)
    X = rng.standard_normal((4, 128))
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
    X = rng.standard_normal((3, 128))
    phi = np.array([[1, 0], [1, 2], [3, 0]])
    d = ft.encode(X, G, S, doc=True, fill_empty=False, phi=phi).reshape(2, 4, 8)
    q = ft.encode(X, G, S, doc=False, phi=phi).reshape(2, 4, 8)
    np.testing.assert_allclose(d[0, 1], ft.psi((X[0] + X[1]) / 2, S[0]))
    np.testing.assert_allclose(q[0, 1], ft.psi(X[0] + X[1], S[0]))
    np.testing.assert_allclose(q[1, 0], ft.psi(X[0] + X[2], S[1]))
    assert (ft.encode(np.zeros((0, 128)), G, S, doc=True) == 0).all()


@pytest.mark.parametrize("seed", range(4))
def test_one_token_against_one_row(seed):
    rng = np.random.default_rng(seed)
    G, S = ft.params(6, 3, 16, seed)
    q, p = rng.standard_normal(128), rng.standard_normal(128)
    cq, cp = ft.codes(q[None], G)[0], ft.codes(p[None], G)[0]
    terms = np.array([ft.psi(q, S[r]) @ ft.psi(p, S[r]) for r in range(6)])
    fq = ft.encode(q[None], G, S, doc=False)
    assert abs(fq @ ft.encode(p[None], G, S, doc=True, fill_empty=False) - (terms * (cq == cp)).sum()) < 1e-9
    assert abs(fq @ ft.encode(p[None], G, S, doc=True, fill_empty=True) - terms.sum()) < 1e-9


def test_config_checks_and_parameters():
    from colpali_amd import FdeConfig

    c = FdeConfig()
    assert (c.reps, c.ksim, c.dproj, c.seed, c.fill_empty, c.dim, c.buckets) == (20, 5, 16, 0, True, 10240, 32)
    for kw in (dict(reps=0), dict(ksim=0), dict(ksim=7), dict(dproj=12), dict(dproj=128), dict(reps=1, ksim=1, dproj=8),
               dict(reps=17, ksim=6, dproj=64), dict(reps=2.0), dict(fill_empty=1), dict(seed=None)):
        with pytest.raises(ValueError):
            FdeConfig(**kw)
    assert FdeConfig(reps=16, ksim=6, dproj=64).dim == 65536
    G, S = FdeConfig(reps=8, ksim=2, dproj=8, seed=9).params()
    tG, tS = ft.params(8, 2, 8, 9)
    assert G.dtype == torch.float32 and G.shape == (8, 2, 128) and S.shape == (8, 8, 128)
    np.testing.assert_array_equal(G.double().numpy(), tG)
    np.testing.assert_array_equal(S.double().numpy(), tS)


def _enc(L, fn, dtype=0, x=FAKE, off=FAKE, n=3, rows=40, dim=128, G=FAKE, S=FAKE, reps=20, ksim=5, dproj=16, fill=1, out=FAKE,
         codes=None):
    if fn == "docs":
        return L.msim_fde_encode_docs(dtype, x, off, n, rows, dim, G, S, reps, ksim, dproj, fill, out, codes, None)
    return L.msim_fde_encode_queries(dtype, x, off, n, rows, dim, G, S, reps, ksim, dproj, out, codes, None)


@pytest.mark.parametrize("fn", ["docs", "queries"])
def test_encoder_abi_refuses_bad_arguments_before_device_work(fn):
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
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=64), dict(dim=320), dict(ksim=0), dict(ksim=7), dict(dproj=12),
               dict(dproj=128), dict(reps=1, ksim=1, dproj=8), dict(reps=17, ksim=6, dproj=64), dict(reps=3, ksim=2, dproj=8)):
        assert _enc(L, fn, **kw) == EUNSUPPORTED, kw


def test_scorer_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def call(dtype=0, fq=FAKE, n_q=4, fd=FAKE, n_d=100, F=10240, out=FAKE, ld=100):
        return L.msim_fde_scores(dtype, fq, n_q, fd, n_d, F, out, ld, None)

    assert call(n_q=0) == 0 and call(n_d=0) == 0
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(F=-256), dict(fq=None), dict(fd=None), dict(out=None), dict(fq=FAKE + 2),
               dict(fd=FAKE + 8), dict(out=FAKE + 2), dict(ld=99)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(dtype=2), dict(dtype=5), dict(F=100), dict(F=0), dict(F=65536 + 256)):
        assert call(**kw) == EUNSUPPORTED, kw


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd
    from colpali_amd import FdeConfig, FdeIndex

    cfg = FdeConfig(reps=2, ksim=3, dproj=16)
    shard = colpali_amd.pack_passages([torch.randn(3, 128).to(torch.bfloat16) for _ in range(5)], torch.device("cpu"),
                                      batch_size=None, id_base=7)
    calls = []
    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"),
                                     fde_score_fn=lambda q, i: calls.append("fde"), rerank_fn=lambda q, c, x: calls.append("rr"))
    q = torch.randn(2, 4, 128).to(torch.bfloat16)
    for idx in (FdeIndex(torch.zeros(4, cfg.dim), 7, cfg), FdeIndex(torch.zeros(5, cfg.dim), 6, cfg)):
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=FdeIndex(torch.zeros(5, cfg.dim), 7, cfg))
    with pytest.raises(ValueError, match="prefilter must be"):
        r.search(q, prefilter=torch.zeros(5, cfg.dim), n_candidates=3)
    with pytest.raises(ValueError):
        FdeIndex(torch.zeros(5, cfg.dim + 1), 7, cfg)
    assert calls == []


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

    def index_of(corpus):
        Fd = ft.encode_all(corpus.blob.float().numpy(), corpus.offsets.numpy(), G, S, doc=True, fill_empty=cfg.fill_empty)
        return colpali_amd.FdeIndex(torch.from_numpy(Fd).float().contiguous(), corpus.id_base, cfg)

    def fde_score_fn(queries, index):
        Fq = np.stack([ft.encode(x.float().numpy(), G, S, doc=False) for x in queries])
        return torch.from_numpy(Fq @ index.Fd.double().numpy().T).float()

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn, fde_score_fn=fde_score_fn)
    ps, pi = r.search(q, k=k, prefilter=index_of(shard), n_candidates=m)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth
        full = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None)
        _, coarse_ids = topk_oracle.topk(fde_score_fn(q, index_of(full)).numpy(), m)
        s, i = rerank_fn(q, full, torch.from_numpy(coarse_ids))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), ps=tps, pi=tpi)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12), (3, 8, 10, 4)])
def test_sharded_fde_prefilter_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
