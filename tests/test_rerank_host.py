"""Candidate reranking without a GPU: the ABI's argument checks (no device work) and the sharded host logic of
ShardedRetriever.search(candidates= / prefilter=) over gloo worlds of 2 and 3, with the oracle injected as score_fn / rerank_fn /
select.  Every rank must get the unsharded answer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def _call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, d=FAKE, d_off=FAKE, n_d=10, dim=128, cand=FAKE, m=4, ld_cand=4,
          out=FAKE, ld=4, flags=0, ws=FAKE):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return L.msim_fwd_candidates(dtype, qt, q_off, oh.ctypes.data, n_q, d, d_off, None, n_d, dim, cand, m, ld_cand, 0, out, ld, None,
                                 flags, ws, None)


def test_candidates_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_fwd_candidates_workspace_bytes(0, 5, 10) == 0
    assert L.msim_fwd_candidates_workspace_bytes(3, 0, 10) == 0
    assert L.msim_fwd_candidates_workspace_bytes(-1, 5, 10) == 0
    w = L.msim_fwd_candidates_workspace_bytes(1000, 100, 125000)
    assert w % 16 == 0 and w >= 125000 * 8 * 4 + 1000 * 100 * (4 + 8 + 16)
    assert L.msim_fwd_candidates_workspace_bytes(1000, 200, 125000) > w
    assert L.msim_fwd_candidates_workspace_bytes(1000, 100, 250000) > w
    assert _call(L, n_q=0) == 0 and _call(L, m=0) == 0                     # nothing to do: no pointer is looked at
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(qt=None), dict(q_off=None), dict(d_off=None), dict(cand=None),
               dict(out=None), dict(ws=None), dict(qt=FAKE + 8), dict(d=FAKE + 2), dict(ws=FAKE + 4), dict(ld_cand=3), dict(ld=3),
               dict(flags=0x2), dict(flags=1 << 8), dict(q_off_host=[1, 3, 7]), dict(q_off_host=[0, 5, 3])):
        assert _call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=320), dict(dim=64), dict(q_off_host=[0, 3, 3 + 129])):
        assert _call(L, **kw) == EUNSUPPORTED, kw


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
    lens = torch.randint(1, 40, (n_docs,), generator=g).tolist()
    docs = [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across shards
    pooled = [d[::3].contiguous() for d in docs]
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)
    cand = torch.randint(-3, n_docs + 3, (4, m), generator=g)          # -1 .. -3 and ids past the corpus: no document
    cand[1, :] = -1
    cand[2, 0] = cand[2, 1]                                            # a duplicate

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        n = full.shape[1]
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < n)
        got = torch.gather(full, 1, d.clamp(0, n - 1))
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    pshard = colpali_amd.pack_passages(pooled[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn)
    cs, ci = r.search(q, k=k, candidates=cand)
    ps, pi = r.search(q, k=k, prefilter=pshard, n_candidates=m)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), cs=cs.numpy(), ci=ci.numpy(), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth
        full = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None)
        pfull = colpali_amd.pack_passages(pooled, torch.device("cpu"), batch_size=None)
        s, i = rerank_fn(q, full, cand)
        tcs, tci = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        _, coarse_ids = topk_oracle.topk(score_fn(q, pfull).numpy(), m)
        s, i = rerank_fn(q, full, torch.from_numpy(coarse_ids))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), cs=tcs, ci=tci, ps=tps, pi=tpi)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12), (3, 8, 10, 4)])
def test_sharded_rerank_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    assert (truth["ci"][1] == -1).all()                                 # a row that lists nothing: padding only
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("ci", "cs", "pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
