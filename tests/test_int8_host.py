"""The int8 token-level index without a GPU: the ABI's argument checks (no device work) and ShardedRetriever.search(
prefilter=<Int8Index>) plumbing, over gloo worlds of 2 and 3 with the truth (tests/int8_truth.py) injected as int8_score_fn.
Every rank must get the unsharded answer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import int8_truth as it

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def docs(dtype=0, x=FAKE, off=FAKE, n=3, rows=40, dim=128, codes=FAKE, scales=FAKE):
        return L.msim_i8_encode_docs(dtype, x, off, n, rows, dim, codes, scales, None)

    def qrys(dtype=0, x=FAKE, rows=40, dim=128, codes=FAKE, scales=FAKE):
        return L.msim_i8_encode_queries(dtype, x, rows, dim, codes, scales, None)

    def score(q8=FAKE, sq=FAKE, qo=FAKE, n_q=4, q_rows=40, maxq=32, d8=FAKE, sd=FAKE, do=FAKE, c0=None, n_d=10, d_rows=90, dim=128,
              out=FAKE, ld=10):
        return L.msim_i8_scores(q8, sq, qo, n_q, q_rows, maxq, d8, sd, do, c0, n_d, d_rows, dim, out, ld, None)

    assert docs(n=0) == 0 and docs(n=0, x=None, off=None, codes=None, scales=None) == 0
    assert qrys(rows=0) == 0 and qrys(rows=0, x=None, codes=None, scales=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, q8=None, d8=None, out=None) == 0
    for kw in (dict(n=-1), dict(rows=-1), dict(dim=64), dict(dim=320), dict(x=None), dict(off=None), dict(codes=None), dict(scales=None),
               dict(x=FAKE + 8), dict(codes=FAKE + 4), dict(off=FAKE + 2), dict(scales=FAKE + 1)):
        assert docs(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(rows=-1), dict(dim=64), dict(x=None), dict(codes=None), dict(scales=None), dict(x=FAKE + 2), dict(codes=FAKE + 8)):
        assert qrys(**kw) == EINVAL, kw
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(dim=320), dict(q8=None), dict(sq=None),
               dict(qo=None), dict(d8=None), dict(sd=None), dict(do=None), dict(out=None), dict(q8=FAKE + 4), dict(d8=FAKE + 8),
               dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
    assert docs(dtype=2) == EUNSUPPORTED and qrys(dtype=7) == EUNSUPPORTED


def _index(shard):
    from colpali_amd import Int8Index

    rows, off = shard.blob.float().numpy(), shard.offsets.numpy()
    d8, sd = it.quantize_pages(rows, off)
    return Int8Index(torch.from_numpy(d8), torch.from_numpy(sd), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                     shard.id_base)


def _truth_fn(queries, index):
    qb = [x.float().numpy() for x in queries]
    qr = np.concatenate(qb)
    q8, sq = it.quantize_tokens(qr)
    q_off = np.cumsum([0] + [len(x) for x in qb])
    c0 = None if index.clamp0 is None else index.clamp0.numpy()
    return torch.from_numpy(it.scores(q8, sq, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), c0))


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd

    shard = colpali_amd.pack_passages([torch.randn(3, 128).to(torch.bfloat16) for _ in range(5)], torch.device("cpu"),
                                      batch_size=None, id_base=7)
    calls = []
    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), int8_score_fn=lambda q, i: calls.append("i8"),
                                     rerank_fn=lambda q, c, x: calls.append("rr"))
    q = torch.randn(2, 4, 128).to(torch.bfloat16)
    short = colpali_amd.pack_passages([torch.randn(3, 128).to(torch.bfloat16) for _ in range(4)], torch.device("cpu"),
                                      batch_size=None, id_base=7)
    moved = colpali_amd.pack_passages([torch.randn(3, 128).to(torch.bfloat16) for _ in range(5)], torch.device("cpu"),
                                      batch_size=None, id_base=6)
    for idx in (_index(short), _index(moved)):
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=_index(shard))
    with pytest.raises(ValueError, match="prefilter must be"):
        r.search(q, prefilter=torch.zeros(5, 128, dtype=torch.int8), n_candidates=3)
    with pytest.raises(ValueError):
        colpali_amd.Int8Index(torch.zeros(15, 64, dtype=torch.int8), torch.zeros(5), shard.offsets, None, shard.lengths)
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

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn, int8_score_fn=_truth_fn)
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
def test_sharded_int8_prefilter_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
