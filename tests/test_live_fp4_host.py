"""The live FP4 index without a GPU: the argument checks of msim_f4_live_compact (no device work), LiveCorpus' host rules for
`fp4_index()` / `drop_fp4_index()`, the tombstone mask over an FP4 prefilter with the numpy truth (tests/fp4_truth.py,
tests/fp4_wide_truth.py) injected as the stage-1 hook, and two live shards over a gloo world of 2.  Nothing here has a tolerance."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fp4_truth as ft
from tests import fp4_wide_truth as wt
from tests import live_truth as lt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def compact(codes=FAKE, row_bytes=64, scales=FAKE + 3, bound=1000, off=FAKE, alive=FAKE, n=10, used=FAKE, ws=FAKE, bounce=FAKE,
                bounce_bytes=4096):
        return L.msim_f4_live_compact(codes, row_bytes, scales, bound, off, alive, n, used, ws, bounce, bounce_bytes, None)

    for n, b in ((0, 1 << 20), (-3, 0), (1, 16), (1024, 65), (1025, 1 << 20), (125_000, 256 << 20)):
        assert L.msim_f4_live_compact_workspace_bytes(n, b) == L.msim_live_compact_workspace_bytes(n, b), (n, b)
    assert compact(n=0) == 0
    assert compact(n=0, codes=None, scales=None, off=None, alive=None, used=None, ws=None, bounce=None) == 0
    for kw in (dict(n=-1), dict(bound=-1), dict(bounce_bytes=-1), dict(codes=None), dict(scales=None), dict(off=None), dict(alive=None),
               dict(used=None), dict(ws=None), dict(bounce=None), dict(codes=FAKE + 8), dict(bounce=FAKE + 4), dict(ws=FAKE + 8),
               dict(bounce_bytes=64), dict(bounce_bytes=0), dict(row_bytes=160, bounce_bytes=160)):
        assert compact(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(row_bytes=0), dict(row_bytes=-64), dict(row_bytes=16), dict(row_bytes=128), dict(row_bytes=65), dict(row_bytes=96),
               dict(bound=1 << 31), dict(row_bytes=160, bound=1 << 31, bounce_bytes=1 << 20)):
        assert compact(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(bounce_bytes=64), dict(row_bytes=160, bounce_bytes=160)):      # one byte short of a code row and its scale byte
        assert compact(**kw) == EINVAL and b"holds no row" in L.msim_last_error()


def _page(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def test_host_rules_of_the_fp4_index():
    import colpali_amd

    g = torch.Generator().manual_seed(3)
    for dim in (128, 320):
        live = colpali_amd.LiveCorpus(20, 4, CPU, width=dim)
        live.add([_page(g, 5, dim), _page(g, 1, dim)])
        live.drop_fp4_index()                                            # no index yet: a no-op
        with pytest.raises(RuntimeError, match="gfx950"):
            live.fp4_index()
        live.drop_fp4_index()
        assert live.rows_used == 6 and len(live) == 2
    for name in ("fp4_index", "drop_fp4_index"):
        assert name in colpali_amd.__doc__


# ------------------------------------------------------------------------------------ the tombstone mask over an FP4 prefilter
def _hooks(truth):
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        n = full.shape[1]
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < n)
        got = torch.gather(full, 1, d.clamp(0, n - 1))
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    def mask_fn(scores, alive):
        return torch.from_numpy(lt.mask(scores.numpy(), alive.numpy()))

    def stage1(queries, index):
        qb = [truth.raw_bits(x.to(torch.bfloat16)) for x in queries]
        qc, qs = truth.encode(np.concatenate(qb))
        q_off = np.cumsum([0] + [len(x) for x in qb])
        return torch.from_numpy(truth.scores(qc, qs, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), None))

    return dict(score_fn=score_fn, rerank_fn=rerank_fn, select=topk_oracle.torch_select, mask_fn=mask_fn), stage1


def _index(cls, truth, shard):
    codes, scales = truth.encode(truth.raw_bits(shard.blob))
    return cls(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), None, shard.lengths.clone(), shard.id_base)


@pytest.mark.parametrize("dim", [128, 320])
def test_deleted_pages_take_no_candidate_slot_of_an_fp4_prefilter(dim):
    import colpali_amd
    from oracle import topk_oracle

    truth, cls, kw = (ft, colpali_amd.Fp4Index, "fp4_score_fn") if dim == 128 else (wt, colpali_amd.Fp4WideIndex, "fp4_wide_score_fn")
    hooks, stage1 = _hooks(truth)
    g = torch.Generator().manual_seed(40 + dim)
    n_docs, k, m, base = 30, 3, 4, 11
    pages = [_page(g, int(n), dim) for n in torch.randint(1, 41, (n_docs,), generator=g)]
    q = torch.nn.functional.normalize(torch.randn(4, 8, dim, generator=g), dim=-1).to(torch.bfloat16)
    live = colpali_amd.LiveCorpus(sum(len(p) for p in pages) + 3, n_docs + 2, CPU, width=dim, id_base=base, **hooks, **{kw: stage1})
    live.add(pages[:17])
    live.add(pages[17:])
    idx = _index(cls, truth, live.view())                                # hand-made: not the shard's own index (there is none on the CPU)
    coarse = stage1(q, idx).numpy()
    tops = topk_oracle.topk(coarse, m, base)[1]                          # each query's m best pages by the FP4 truth ...
    deleted = sorted(set(tops.reshape(-1).tolist()))
    live.delete(deleted)                                                 # ... all deleted: unmasked, they would fill every list
    for row in tops:
        assert np.isin(row, deleted).any()
    assert n_docs - len(deleted) >= m
    got_s, got_i = live.search(q, k, prefilter=idx, n_candidates=m)

    surv = [s for s in range(n_docs) if s + base not in deleted]
    F = colpali_amd.pack_passages([pages[s] for s in surv], CPU, batch_size=None)
    cand = topk_oracle.topk(stage1(q, _index(cls, truth, F)).numpy(), m)[1]
    s, i = hooks["rerank_fn"](q, F, torch.from_numpy(cand))
    want_s, want_i = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
    np.testing.assert_array_equal(got_s.numpy().view(np.int32), want_s.view(np.int32))
    np.testing.assert_array_equal(got_i.numpy(), lt.expected_ids(want_i, surv, base))
    assert (got_i.numpy() >= 0).all() and not np.isin(got_i.numpy(), deleted).any()   # all k of m candidates were live pages


# --------------------------------------------------------------------------------------------------- two live shards over gloo
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
    from oracle import topk_oracle

    hooks, stage1 = _hooks(ft)
    g = torch.Generator().manual_seed(7)
    lens = torch.randint(1, 40, (n_docs,), generator=g).tolist()
    docs = [_page(g, n) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across pages
    docs[n_docs - 3] = docs[2].clone()        # ... and across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)
    deleted = sorted(set(torch.randint(0, n_docs, (n_docs // 3,), generator=g).tolist()) | {2})

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    live = colpali_amd.LiveCorpus(sum(lens[lo:hi]) + 5, hi - lo + 2, CPU, id_base=lo, fp4_score_fn=stage1, **hooks)
    half = (hi - lo) // 2
    live.add(docs[lo:lo + half])
    live.delete([i for i in deleted if lo <= i < lo + half])
    live.add(docs[lo + half:hi])
    live.delete([i for i in deleted if lo + half <= i < hi])
    ps, pi = live.search(q, k=k, prefilter=_index(colpali_amd.Fp4Index, ft, live.view()), n_candidates=m, world=world, rank=rank, dist=dist)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth over the surviving pages, positions mapped back to ids
        surv = [d for d in range(n_docs) if d not in deleted]
        full = colpali_amd.pack_passages([docs[d] for d in surv], CPU, batch_size=None)
        cand = topk_oracle.topk(stage1(q, _index(colpali_amd.Fp4Index, ft, full)).numpy(), m)[1]
        s, i = hooks["rerank_fn"](q, full, torch.from_numpy(cand))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), ps=tps, pi=lt.expected_ids(tpi, surv), deleted=np.asarray(deleted))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9)])
def test_two_live_shards_with_an_fp4_prefilter_give_the_unsharded_answer(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
        assert not np.isin(got["pi"], truth["deleted"]).any()
