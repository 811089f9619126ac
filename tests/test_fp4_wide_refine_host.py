"""The wide FP4 candidate rerank and search(refine=<Fp4WideIndex>) on a 320-wide shard without a GPU: the header, binding and
exports, the argument checks of the two msim_f4w_candidates entries (no device work), and the route with the numpy truth
(tests/fp4_wide_truth.py) injected as the stage-1 and refine hooks -- the two identities the GPU test checks on the kernels,
filter= and group_by= with n_refine governing the grouped list limit, a live 320-wide shard's deleted pages, a gloo world of 2
against the unsharded answer, and the refusals of a mismatched (index, shard) pair before any hook.  Nothing here has a tolerance."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import fp4_wide_truth as wt
from tests import live_truth as lt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")
ENTRIES = ("msim_f4w_candidates_plan", "msim_f4w_candidates")
DIM = 320


# ------------------------------------------------------------------------------------------------- header, binding and exports
def test_header_binding_and_exports():
    import colpali_amd
    from colpali_amd import retrieval

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
    assert re.search(r"int msim_f4w_candidates_plan\(int n_q, int max_q_tokens, int m, int32_t \*plan", header)
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()
    for name in ENTRIES:
        assert getattr(L, name).argtypes is not None and getattr(L, name).restype is not None, name
    assert L.msim_f4w_candidates.argtypes == L.msim_f4_candidates.argtypes     # the same argument list
    assert "fp4_wide_rerank_scores" in colpali_amd.__all__ and "fp4_wide_rerank_scores" in colpali_amd.__doc__
    assert colpali_amd.fp4_wide_rerank_scores in retrieval._KERNELS
    assert "msim_f4w_candidates" in colpali_amd.fp4_wide_rerank_scores.__doc__
    for cls in (colpali_amd.ShardedRetriever, colpali_amd.LiveCorpus):
        assert "Fp4WideIndex" in cls.search.__doc__ and "fp4_wide_rerank_fn" in cls.search.__doc__


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_plan_entry():
    import colpali_amd

    L = colpali_amd._lib.lib()
    plan = torch.zeros(4, dtype=torch.int32)
    assert L.msim_f4w_candidates_plan(1000, 32, 4000, plan.data_ptr()) == 0
    assert plan[0] == 2 and plan[2] == 4 and plan[3] == 1_000_000 and 1 <= int(plan[1]) <= 4
    assert [L.msim_f4w_candidates_plan(3, t, 5, plan.data_ptr()) or int(plan[0]) for t in (1, 16, 17, 32, 33, 64, 65, 128)] == \
        [1, 1, 2, 2, 4, 4, 8, 8]
    assert L.msim_f4w_candidates_plan(3, 0, 5, plan.data_ptr()) == 0 and plan[0] == 1 and plan[3] == 4
    assert L.msim_f4w_candidates_plan(0, 32, 0, plan.data_ptr()) == 0 and plan[0] == 2 and plan[3] == 0
    for args in ((-1, 32, 5, FAKE), (3, -1, 5, FAKE), (3, 32, -1, FAKE), (3, 32, 5, None)):
        assert L.msim_f4w_candidates_plan(*args) == EINVAL, args
        assert L.msim_last_error()
    for args in ((3, 129, 5, FAKE), (1 << 30, 32, 1 << 4, FAKE)):          # a 129-token bound; 2^32 workgroups
        assert L.msim_f4w_candidates_plan(*args) == EUNSUPPORTED, args
        assert L.msim_last_error()


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def cand(q=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90,
             dim=DIM, cand=FAKE, m=6, ld_cand=6, id_base=0, out=FAKE, ld=6, ids=FAKE):
        return L.msim_f4w_candidates(q, qs, qo, n_q, q_rows, maxq, d4, ds, do, c0, n_d, d_rows, dim, cand, m, ld_cand, id_base, out, ld,
                                     ids, None)

    assert cand(n_q=0) == 0 and cand(m=0, ld_cand=0, ld=0) == 0
    assert cand(n_q=0, q=None, d4=None, cand=None, out=None) == 0 and cand(m=0, q=None, qo=None, do=None, cand=None, out=None) == 0
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(m=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q=None), dict(qs=None),
               dict(qo=None), dict(d4=None), dict(ds=None), dict(do=None), dict(cand=None), dict(out=None), dict(q=FAKE + 8),
               dict(d4=FAKE + 4), dict(qo=FAKE + 2), dict(do=FAKE + 1), dict(out=FAKE + 2), dict(cand=FAKE + 4), dict(ids=FAKE + 4),
               dict(ld_cand=5), dict(ld=5)):
        assert cand(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=128), dict(maxq=129), dict(n_q=1 << 30, m=1 << 4, ld_cand=16, ld=16)):
        assert cand(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    # the 128-wide entries keep refusing width 320
    for name in ("msim_f4_candidates", "msim_f4_candidates_q6"):
        assert getattr(L, name)(FAKE, FAKE, FAKE, 4, 40, 32, FAKE, FAKE, FAKE, None, 10, 90, DIM, FAKE, 6, 6, 0, FAKE, 6, FAKE,
                                None) == EUNSUPPORTED


# ----------------------------------------------------------------------------------------------------------------- the hooks
def _page(g, n, dim=DIM, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _index(shard):
    from colpali_amd import Fp4WideIndex

    codes, scales = wt.encode(wt.raw_bits(shard.blob))
    return Fp4WideIndex(torch.from_numpy(codes), torch.from_numpy(scales), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                        shard.id_base)


def _gather(full, candidates, id_base):
    """a score matrix over a shard's pages at a list of GLOBAL ids: (-inf, -1) off the shard"""
    n = full.shape[1]
    d = candidates - id_base
    ok = (candidates >= 0) & (d >= 0) & (d < n)
    got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0))) if n else torch.zeros(candidates.shape)
    return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))


def _hooks(calls=None):
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    def note(what):
        if calls is not None:
            calls.append(what)

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        note(("rerank", candidates.clone()))
        return _gather(score_fn(queries, corpus), candidates, corpus.id_base)

    def stage1(queries, index):
        qb = [wt.raw_bits(x.to(torch.bfloat16)) for x in queries]
        qc, qs = wt.encode(np.concatenate(qb))
        q_off = np.cumsum([0] + [len(x) for x in qb])
        return torch.from_numpy(wt.scores(qc, qs, q_off, index.codes.numpy(), index.scales.numpy(), index.offsets.numpy(), None))

    def refine_fn(queries, index, candidates):
        note(("refine", candidates.clone()))
        return _gather(stage1(queries, index), candidates, index.id_base)

    def narrow_fn(queries, index, candidates):
        note(("narrow", None))
        raise AssertionError("the 128-wide refine hook ran for an Fp4WideIndex")

    return dict(score_fn=score_fn, rerank_fn=rerank_fn, fp4_wide_score_fn=stage1, fp4_wide_rerank_fn=refine_fn, fp4_rerank_fn=narrow_fn,
                select=topk_oracle.torch_select)


def _case(seed=5, n_docs=23, id_base=7):
    import colpali_amd

    g = torch.Generator().manual_seed(seed)
    pages = [_page(g, int(n)) for n in torch.randint(1, 30, (n_docs,), generator=g)]
    pages[4] = pages[2].clone()                                     # exact ties
    q = torch.nn.functional.normalize(torch.randn(4, 8, DIM, generator=g), dim=-1).to(torch.bfloat16)
    shard = colpali_amd.pack_passages(pages, CPU, batch_size=None, id_base=id_base)
    all_ids = torch.arange(id_base, id_base + n_docs, dtype=torch.int64).expand(4, n_docs)
    return pages, q, shard, all_ids


def _pooled(pages, id_base):
    import colpali_amd

    return colpali_amd.pack_passages([p.float().mean(0, keepdim=True).to(torch.bfloat16) for p in pages], CPU, batch_size=None,
                                     id_base=id_base)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x.numpy().view(np.int32) if x.dtype == torch.float32 else x.numpy(),
                                      y.numpy().view(np.int32) if y.dtype == torch.float32 else y.numpy())


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_a_mismatched_pair_is_refused_before_any_hook():
    import colpali_amd
    from tests import fp4_truth as ft

    pages, q, shard, all_ids = _case()
    calls = []
    wide = _index(shard)
    g = torch.Generator().manual_seed(6)
    shard128 = colpali_amd.pack_passages([_page(g, 3, 128) for _ in range(23)], CPU, batch_size=None, id_base=7)
    codes, scales = ft.encode(ft.raw_bits(shard128.blob))
    narrow = colpali_amd.Fp4Index(torch.from_numpy(codes), torch.from_numpy(scales), shard128.offsets.clone(), None,
                                  shard128.lengths.clone(), 7)
    q128 = torch.zeros(4, 4, 128, dtype=torch.bfloat16)
    with pytest.raises(NotImplementedError, match="refine takes an Fp4Index of a 128-wide shard"):
        colpali_amd.ShardedRetriever(shard128, **_hooks(calls)).search(q128, candidates=all_ids, refine=wide, n_refine=3)
    r = colpali_amd.ShardedRetriever(shard, **_hooks(calls))
    with pytest.raises(NotImplementedError, match="refine takes an Fp4Index of a 128-wide shard"):
        r.search(q, candidates=all_ids, refine=narrow, n_refine=3)
    with pytest.raises(NotImplementedError, match="refine takes an Fp4Index of a 128-wide shard"):
        r.search(q, candidates=all_ids, refine=shard, n_refine=3)       # no index at all, on a wide shard
    # the rules of the route hold for the wide pair as they do at 128
    with pytest.raises(ValueError, match="exactly one of candidates= / prefilter="):
        r.search(q, refine=wide, n_refine=3)
    for bad in (None, 0, -2):
        with pytest.raises(ValueError, match="n_refine >= 1"):
            r.search(q, candidates=all_ids, refine=wide, n_refine=bad)
    with pytest.raises(ValueError, match="n_refine=6 exceeds"):
        r.search(q, prefilter=wide, n_candidates=5, refine=wide, n_refine=6)
    for other in (_index(_case(n_docs=22)[2]), _index(_case(id_base=6)[2])):
        with pytest.raises(ValueError, match="refine covers"):
            r.search(q, candidates=all_ids, refine=other, n_refine=3)
    assert calls == []                                              # every refusal came before a hook ran
    # the wrappers' own refusals need no device either
    with pytest.raises(NotImplementedError, match="Fp4Index"):
        colpali_amd.fp4_rerank_scores(q, wide, all_ids)
    with pytest.raises(NotImplementedError, match="fp4_rerank_scores"):
        colpali_amd.fp4_wide_rerank_scores(q, narrow, all_ids)
    with pytest.raises(NotImplementedError, match="Fp4WideIndex"):
        colpali_amd.fp4_wide_rerank_scores(q, shard, all_ids)


# ------------------------------------------------------------------------------------------------------------- the identities
class _OneRank:
    """the collective library of a world of one: all_gather_into_tensor copies"""

    @staticmethod
    def all_gather_into_tensor(out, mine, group=None):
        out.copy_(mine)


def test_the_two_identities_and_the_list_the_rerank_sees():
    import colpali_amd
    from oracle import topk_oracle

    pages, q, shard, all_ids = _case()
    calls = []
    hooks = _hooks(calls)
    r = colpali_amd.ShardedRetriever(shard, **hooks)
    idx = _index(shard)
    pooled = _pooled(pages, 7)
    for force in (False, True):
        r.force_collective = force
        if force:
            r.dist = _OneRank()
        for m in (1, 5, 22):
            # refining to the whole list changes nothing
            _same(r.search(q, 4, prefilter=pooled, n_candidates=m, refine=idx, n_refine=m), r.search(q, 4, prefilter=pooled, n_candidates=m))
            # refining every page is the FP4 first stage
            del calls[:]
            got = r.search(q, 4, candidates=all_ids, refine=idx, n_refine=m)
            refined = [c for what, c in calls if what == "rerank"][-1]
            _same(got, r.search(q, 4, prefilter=idx, n_candidates=m))
            want = topk_oracle.topk(hooks["fp4_wide_score_fn"](q, idx).numpy(), m, 7)[1]
            np.testing.assert_array_equal(refined.numpy(), want)      # the exact rerank saw the FP4 top m, in (score desc, id asc) order
            assert [what for what, _ in calls][:2] == ["refine", "rerank"]
    # an entry the refine stage scores -inf is not reranked: ids off the shard and -1 never reach the exact rerank
    del calls[:]
    junk = torch.tensor([[7, -1, 500, 9]] * 4, dtype=torch.int64)
    s, i = r.search(q, 4, candidates=junk, refine=idx, n_refine=4)
    seen = [c for what, c in calls if what == "rerank"][-1]
    assert sorted(seen[0].tolist()) == [-1, -1, 7, 9]
    assert (i[:, 2:] == -1).all() and torch.isinf(s[:, 2:]).all()


def test_filter_and_group_by_with_n_refine_governing_the_list_limit():
    import colpali_amd
    from colpali_amd.group import SELECT_MAX_M
    from tests import filter_truth as flt_t

    def ok(flt, n_q):
        return flt_t.allowed(flt_t.spec_of(flt, n_q), n_q, len(flt))

    def mask_fn(scores, flt, alive):
        assert alive is None
        return torch.from_numpy(flt_t.masked(scores.numpy(), ok(flt, scores.shape[0])))

    def ids_fn(ids, flt, alive):
        assert alive is None
        return torch.from_numpy(flt_t.ids_truth(ids.numpy(), ok(flt, ids.shape[0]), flt.id_base))

    pages, q, shard, all_ids = _case()
    idx = _index(shard)
    hooks = _hooks()
    # filter=: only even local pages are allowed, on both routes; with n_refine = every allowed page the answer is the FP4 first
    # stage's under the same filter
    allowed = torch.arange(23) % 2 == 0
    flt = colpali_amd.PageFilter.from_mask(allowed, 7, pack_fn=lambda m2: torch.from_numpy(flt_t.pack(m2.numpy()).view(np.int32)))
    r = colpali_amd.ShardedRetriever(shard, filter_mask_fn=mask_fn, filter_ids_fn=ids_fn, **hooks)
    n_ok = int(allowed.sum())
    a = r.search(q, 4, candidates=all_ids, filter=flt, refine=idx, n_refine=n_ok)
    b = r.search(q, 4, prefilter=idx, n_candidates=n_ok, filter=flt)
    _same(a, b)
    assert ((a[1] - 7) % 2 == 0).all()
    c = r.search(q, 4, prefilter=_pooled(pages, 7), n_candidates=n_ok, filter=flt, refine=idx, n_refine=5)
    assert ((c[1] - 7) % 2 == 0).all() and (c[1] >= 0).all()

    # group_by=: n_refine counts pages and governs group_select's list limit
    picked = []

    def group_select_fn(scores, gids, page_ids, k):
        picked.append(int(scores.shape[1]))
        return scores[:, :k], gids[:, :k], page_ids[:, :k]

    r = colpali_amd.ShardedRetriever(shard, group_select_fn=group_select_fn, **hooks)
    groups = colpali_amd.PageGroups.from_labels(torch.arange(23, dtype=torch.int64) // 2, 7)
    long_list = (7 + torch.arange(SELECT_MAX_M + 5, dtype=torch.int64) % 23).expand(4, SELECT_MAX_M + 5)
    with pytest.raises(NotImplementedError, match="group_select takes at most"):
        r.search(q, 3, candidates=long_list, group_by=groups)
    out = r.search(q, 3, candidates=long_list, group_by=groups, refine=idx, n_refine=9)
    assert picked == [9] and len(out) == 3
    with pytest.raises(NotImplementedError, match="group_select takes at most"):
        r.search(q, 3, candidates=long_list, group_by=groups, refine=idx, n_refine=SELECT_MAX_M + 1)
    r.search(q, 3, prefilter=idx, n_candidates=SELECT_MAX_M + 1, group_by=groups, refine=idx, n_refine=SELECT_MAX_M)
    assert picked == [9, SELECT_MAX_M]


# ------------------------------------------------------------------------------------------------------------------------ live
def test_a_deleted_page_of_a_live_wide_shard_never_leaves_the_refine_hook():
    import colpali_amd

    pages, q, _, _ = _case(n_docs=20, id_base=11)
    seen = []
    hooks = _hooks()
    inner = hooks.pop("fp4_wide_rerank_fn")

    def refine_fn(queries, index, candidates):
        s, i = inner(queries, index, candidates)
        seen.append(i.clone())
        return s, i

    live = colpali_amd.LiveCorpus(sum(len(p) for p in pages) + 3, 22, CPU, width=DIM, id_base=11, fp4_wide_rerank_fn=refine_fn,
                                  mask_fn=lambda scores, alive: torch.from_numpy(lt.mask(scores.numpy(), alive.numpy())), **hooks)
    live.add(pages)
    idx = _index(live.view())
    deleted = [11 + c for c in range(1, 20, 3)]
    live.delete(deleted)
    all_ids = torch.arange(11, 31, dtype=torch.int64).expand(4, 20)
    surv = [c for c in range(20) if 11 + c not in deleted]
    fresh = colpali_amd.pack_passages([pages[c] for c in surv], CPU, batch_size=None)
    r = colpali_amd.ShardedRetriever(fresh, **_hooks())
    for m in (1, 6, len(surv)):
        got_s, got_i = live.search(q, 5, candidates=all_ids, refine=idx, n_refine=m)
        assert not np.isin(seen[-1].numpy(), deleted).any()           # the hook's output names no deleted page ...
        assert not np.isin(got_i.numpy(), deleted).any()              # ... and neither does the answer
        want_s, want_i = r.search(q, 5, candidates=torch.arange(len(surv), dtype=torch.int64).expand(4, len(surv)), refine=_index(fresh),
                                  n_refine=m)
        np.testing.assert_array_equal(got_s.numpy().view(np.int32), want_s.numpy().view(np.int32))
        np.testing.assert_array_equal(got_i.numpy(), lt.expected_ids(want_i.numpy(), surv, 11))
    with pytest.raises(ValueError, match="n_refine goes with refine="):
        live.search(q, 5, candidates=all_ids, n_refine=3)


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

    pages, q, full, all_ids = _case(seed=9, n_docs=n_docs, id_base=0)

    def both(r, shard, lo, hi):
        pre = _pooled(pages[lo:hi], lo)
        a = r.search(q, k, prefilter=pre, n_candidates=m1, refine=_index(shard), n_refine=m2)
        b = r.search(q, k, candidates=all_ids, refine=_index(shard), n_refine=m2)
        return dict(a_s=a[0].numpy(), a_i=a[1].numpy(), b_s=b[0].numpy(), b_i=b[1].numpy())

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(pages[lo:hi], CPU, batch_size=None, id_base=lo)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"),
             **both(colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, **_hooks()), shard, lo, hi))
    if rank == 0:
        np.savez(os.path.join(out_dir, "truth.npz"), **both(colpali_amd.ShardedRetriever(full, **_hooks()), full, 0, n_docs))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m1,m2", [(2, 37, 5, 20, 9)])
def test_a_world_of_two_refines_to_the_unsharded_answer(tmp_path, world, n_docs, k, m1, m2):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m1, m2, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("a_i", "a_s", "b_i", "b_s"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
    assert (truth["a_i"] >= 0).all() and (truth["b_i"] >= 0).all()
