"""The deep top-k (msim_topk_deep_f32, 1024 < k <= 8192) without a GPU: the header, the binding and the export, every refusal of
the contract (each returned before any device work), the workspace plan restated, the old entry's limits unmoved, and the routes
with the numpy order (oracle/topk_oracle.py) injected as the selection -- the sizes reach it unchanged, a gloo world of 2 merges
rows of world x k explicit ids to the unsharded answer, and the grouped route keeps its own limit.  Nothing here has a tolerance."""
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

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------- header, binding and exports
def test_header_binding_and_export():
    import colpali_amd
    from colpali_amd import retrieval

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"#define\s+MSIM_TOPK_DEEP_MAX_K\s+8192\b", header)
    assert re.search(r"size_t\s+msim_topk_deep_workspace_bytes\(int n_q, int64_t n, int k\);", header)
    assert re.search(r"int\s+msim_topk_deep_f32\(const float \*scores, const int64_t \*ids, int n_q, int64_t n, int64_t ld, int k, "
                     r"int64_t id_base,\s+float \*out_scores, int64_t \*out_ids, void \*workspace, void \*stream\);", header)
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)              # additions only
    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    for name in ("msim_topk_deep_workspace_bytes", "msim_topk_deep_f32"):
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is not None, name
    assert L.msim_topk_deep_f32.argtypes == L.msim_topk_f32.argtypes            # "word for word"
    assert colpali_amd.TOPK_MAX_K == 8192 == retrieval.TOPK_MAX_K and "TOPK_MAX_K" in colpali_amd.__all__
    assert "8192" in colpali_amd.topk.__doc__
    for cls in (colpali_amd.ShardedRetriever,):
        assert "TOPK_MAX_K" in cls.search.__doc__ and "4096" in cls.search.__doc__


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def deep(scores=FAKE, ids=None, n_q=3, n=5000, ld=5000, k=2000, id_base=0, out_s=FAKE, out_i=FAKE, ws=None):
        return L.msim_topk_deep_f32(scores, ids, n_q, n, ld, k, id_base, out_s, out_i, ws, None)

    assert deep(n_q=0) == OK                                                    # nothing launched
    assert deep(n_q=0, scores=None, out_s=None, out_i=None) == OK
    for kw in (dict(n_q=-1), dict(n=-1), dict(k=0), dict(k=-5), dict(out_s=None), dict(out_i=None), dict(scores=None), dict(ld=4999),
               dict(scores=FAKE + 2), dict(out_s=FAKE + 1), dict(out_i=FAKE + 4), dict(ids=FAKE + 4),
               dict(n_q=4, n=125000, ld=125000, k=4096, ws=None)):              # a split plan without its workspace
        assert deep(**kw) == EINVAL, kw
        assert b"msim_topk_deep_f32" in L.msim_last_error()
    assert L.msim_topk_deep_workspace_bytes(4, 125000, 4096) > 0
    for kw in (dict(k=8193), dict(k=1 << 20), dict(n=1 << 31, ld=1 << 31), dict(n=(1 << 40), ld=(1 << 40))):
        assert deep(**kw) == EUNSUPPORTED, kw
        assert b"msim_topk_deep_f32" in L.msim_last_error()
    assert deep(k=8193) == EUNSUPPORTED and b"8192" in L.msim_last_error()       # the message names the limit
    # ... through the Python layer's check it is what k > 1024 was: NotImplementedError
    with pytest.raises(NotImplementedError, match="8192"):
        colpali_amd._lib.check(deep(k=8193), "msim_topk_deep_f32")


def test_the_old_entry_keeps_its_limit_and_its_plan():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_topk_workspace_bytes(4, 125000, 5000) == 0
    assert L.msim_topk_f32(FAKE, None, 3, 5000, 5000, 1025, 0, FAKE, FAKE, None, None) == EUNSUPPORTED
    assert L.msim_last_error() == b"k=1025 > 1024"


def test_workspace_follows_the_plan():
    """Split rows -- implicit ids, fewer than 128 rows of at least 8 segments of 2048 columns -- count into the workspace: per row four
    256-bin histograms and the gather counter (1028 words, the part the call zeroes), every segment's last-digit histogram, and the
    survivors as (u32 key, u32 column).  One workgroup per row needs nothing."""
    import colpali_amd

    L = colpali_amd._lib.lib()

    def a16(x):
        return (x + 15) // 16 * 16

    def plan(n_q, n, k):
        if not (n_q < 128 and n >= 8 * 2048):
            return 0
        segs = -(-n // 2048)
        return a16(n_q * 1028 * 4) + a16(n_q * segs * 256 * 4) + 2 * a16(n_q * k * 4)

    cases = [(1, 1025, 1025), (4, 125000, 4096), (1000, 125000, 2048), (3, 65536, 8192), (1, 10, 8192)]
    for n_q, n, k in cases + [(127, 16384, 1100), (128, 16384, 1100), (5, 16383, 1100), (2, 40001, 3000)]:
        assert L.msim_topk_deep_workspace_bytes(n_q, n, k) == plan(n_q, n, k), (n_q, n, k)
    assert [L.msim_topk_deep_workspace_bytes(*c) > 0 for c in cases] == [False, True, False, True, False]      # both forms are planned
    for n_q, n, k in [(4, 125000, 8193), (4, 125000, 1 << 20), (4, 125000, 0), (0, 125000, 4096), (4, 1 << 31, 4096)]:
        assert L.msim_topk_deep_workspace_bytes(n_q, n, k) == 0, (n_q, n, k)


# ----------------------------------------------------------------------------------------------------------------- the routes
def _page(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _index(shard):
    from colpali_amd import Fp4Index

    codes, scales = ft.encode(ft.raw_bits(shard.blob))
    return Fp4Index(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                    shard.id_base)


def _gather(full, candidates, id_base):
    n = full.shape[1]
    d = candidates - id_base
    ok = (candidates >= 0) & (d >= 0) & (d < n)
    got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0)))
    return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))


def _hooks(sizes=None):
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        return _gather(score_fn(queries, corpus), candidates, corpus.id_base)

    def refine_fn(queries, index, candidates):                     # a stand-in with the hook's shape: the selection is what is tested
        return _gather(score_fn(queries, index._exact) * 0.5, candidates, index.id_base)

    def select(scores, k, id_base=0, ids=None):
        if sizes is not None:
            sizes.append((tuple(scores.shape), int(k), ids is not None))
        return topk_oracle.torch_select(scores, k, id_base, ids)

    return dict(score_fn=score_fn, rerank_fn=rerank_fn, fp4_rerank_fn=refine_fn, select=select)


def _case(seed=5, n_docs=23, id_base=7):
    import colpali_amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(n)) for n in torch.randint(1, 30, (n_docs,), generator=g)]
    pages[4] = pages[2].clone()                                     # exact ties
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)
    shard = colpali_amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    return pages, q, shard


def _refine_index(shard):
    idx = _index(shard)
    idx._exact = shard
    return idx


def test_the_routes_pass_deep_sizes_through_unchanged():
    import colpali_amd
    from oracle import topk_oracle

    pages, q, shard = _case()
    sizes = []
    hooks = _hooks(sizes)
    r = colpali_amd.ShardedRetriever(shard, **hooks)
    s, i = r.search(q, k=3000)
    assert sizes == [((4, 23), 3000, False)] and s.shape == i.shape == (4, 3000)
    want_s, want_i = topk_oracle.topk(hooks["score_fn"](q, shard).numpy(), 3000, 7)
    np.testing.assert_array_equal(i.numpy(), want_i)
    np.testing.assert_array_equal(s.numpy().view(np.int32), want_s.view(np.int32))
    assert (i[:, 23:] == -1).all() and (i[:, :23] >= 7).all()

    del sizes[:]
    pooled = colpali_amd.pack_passages([p.float().mean(0, keepdim=True).to(torch.bfloat16) for p in pages], CPU, batch_size=None, id_base=7)
    s, i = r.search(q, k=5, prefilter=pooled, n_candidates=5000, refine=_refine_index(shard), n_refine=2000)
    assert sizes == [((4, 23), 5000, False), ((4, 5000), 2000, True), ((4, 2000), 5, True)]
    want = r.search(q, k=5)                                          # every page went through both stages: the exact answer
    np.testing.assert_array_equal(i.numpy(), want[1].numpy())
    np.testing.assert_array_equal(s.numpy().view(np.int32), want[0].numpy().view(np.int32))


def test_the_grouped_route_keeps_its_own_limit():
    import colpali_amd
    from colpali_amd.group import SELECT_MAX_M

    pages, q, shard = _case()
    r = colpali_amd.ShardedRetriever(shard, **_hooks())
    groups = colpali_amd.PageGroups.from_labels(torch.arange(23, dtype=torch.int64) // 2, 7)
    assert SELECT_MAX_M == 4096 < colpali_amd.TOPK_MAX_K
    with pytest.raises(NotImplementedError, match="group_select takes at most 4096"):
        r.search(q, 3, prefilter=shard, n_candidates=SELECT_MAX_M + 1, group_by=groups)
    with pytest.raises(NotImplementedError, match="group_select takes at most 4096"):
        r.search(q, 3, prefilter=shard, n_candidates=8000, refine=_refine_index(shard), n_refine=5000, group_by=groups)


# ------------------------------------------------------------------------------------------------------------------ sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_docs, k, m1, m2, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd

    pages, q, full = _case(seed=9, n_docs=n_docs, id_base=0)
    pooled = [p.float().mean(0, keepdim=True).to(torch.bfloat16) for p in pages]

    def both(r, shard, lo, hi, sizes):
        pre = colpali_amd.pack_passages(pooled[lo:hi], CPU, batch_size=None, id_base=lo)
        a = r.search(q, k)
        b = r.search(q, 5, prefilter=pre, n_candidates=m1, refine=_refine_index(shard), n_refine=m2)
        return dict(a_s=a[0].numpy(), a_i=a[1].numpy(), b_s=b[0].numpy(), b_i=b[1].numpy(), widths=np.array([s[0][1] for s in sizes]))

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(pages[lo:hi], CPU, batch_size=None, id_base=lo)
    sizes = []
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"),
             **both(colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, **_hooks(sizes)), shard, lo, hi, sizes))
    if rank == 0:
        np.savez(os.path.join(out_dir, "truth.npz"), **both(colpali_amd.ShardedRetriever(full, **_hooks()), full, 0, n_docs, []))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m1,m2", [(2, 37, 1500, 3000, 1100)])
def test_a_world_of_two_merges_deep_lists_to_the_unsharded_answer(tmp_path, world, n_docs, k, m1, m2):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m1, m2, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("a_i", "a_s", "b_i", "b_s"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
        assert world * k in got["widths"] and world * m1 in got["widths"] and world * m2 in got["widths"]     # the merge rows
    assert truth["a_i"].shape == (4, k) and (truth["a_i"][:, :n_docs] >= 0).all() and (truth["a_i"][:, n_docs:] == -1).all()
    assert (truth["b_i"] >= 0).all()
