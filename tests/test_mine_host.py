"""Hard-negative mining without a GPU: the numpy restatement (tests/mine_truth.py) against a brute-force loop, the C ABI's argument
checks (refused before any device work), the argument errors of the public entries, `LiveCorpus.mine` with deleted slots and
`ShardedRetriever.mine` over gloo worlds of 2 and 3 with the restatement injected as score / bounds / mask functions: a positive
held by another rank must bound this rank's selection, and every rank must get the single-shard truth."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import mine_truth as mt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")
NINF = -float("inf")


# ------------------------------------------------------------------------------------------------------------ the restatement
def _brute(s, pos_list, n_neg, id_base, max_ratio, skip_top, alive):
    """The rule of the issue, written as plainly as possible: one query, one column at a time."""
    n_q, n = s.shape
    out_s, out_i = [], []
    for q in range(n_q):
        mine_pos = [i - id_base for i in pos_list[q] if id_base <= i < id_base + n]
        live_pos = [c for c in mine_pos if alive is None or alive[c] != 0]
        pos = np.float32(np.inf)
        if live_pos:
            pos = max(np.float32(s[q, c]) for c in live_pos)
        cand = []
        for c in range(n):
            if c in mine_pos:
                continue
            if alive is not None and alive[c] == 0:
                continue
            if s[q, c] == -np.inf:
                continue
            if max_ratio is not None:
                with np.errstate(invalid="ignore"):
                    if np.float32(s[q, c]) > np.float32(np.float32(max_ratio) * pos):
                        continue
            cand.append((-float(s[q, c]), c + id_base))
        cand.sort()
        cand = cand[skip_top:skip_top + n_neg]
        out_s.append([-a for a, _ in cand] + [-np.inf] * (n_neg - len(cand)))
        out_i.append([i for _, i in cand] + [-1] * (n_neg - len(cand)))
    return np.asarray(out_s, dtype=np.float32), np.asarray(out_i, dtype=np.int64)


@pytest.mark.parametrize("seed,n_q,n,id_base,max_ratio,skip_top,n_neg,negative", [
    (0, 5, 23, 0, None, 0, 4, False), (1, 6, 40, 1000, 0.95, 0, 8, False), (2, 4, 17, 7, 0.95, 3, 5, False),
    (3, 5, 30, 0, 0.95, 2, 6, True), (4, 3, 6, 0, 0.5, 1, 9, False), (5, 4, 12, 100, 1.25, 0, 3, True),
])
def test_truth_equals_a_brute_force_loop(seed, n_q, n, id_base, max_ratio, skip_top, n_neg, negative):
    r = np.random.default_rng(seed)
    s = r.integers(-6, 7, size=(n_q, n)).astype(np.float32) / 4          # a coarse grid: many exact ties
    if negative:
        s = -np.abs(s) - 1
    s[r.random((n_q, n)) < 0.1] = -np.inf                                # pages of 0 rows
    alive = (r.random(n) > 0.25).astype(np.uint8) if seed % 2 else None
    pos_list = [[int(x) for x in r.integers(id_base - 2, id_base + n + 2, size=r.integers(0, 4))] for _ in range(n_q)]
    pos_list[0] = []                                                     # a query without positives
    pos_list[1] = [id_base - 1, id_base + n, -1]                         # ... and one whose positives all lie outside the shard
    pos_list[2] = pos_list[2] + pos_list[2]                              # duplicates
    want_s, want_i = _brute(s, pos_list, n_neg, id_base, max_ratio, skip_top, alive)
    got_s, got_i = mt.mine(s, pos_list, n_neg, id_base, max_ratio, skip_top, alive)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_s, want_s)
    m = mt.masked(s, pos_list, id_base, max_ratio, alive)
    ok = mt.eligible(s, pos_list, id_base, max_ratio, alive)
    assert np.isneginf(m[~ok]).all() and (m[ok] == s[ok]).all()
    b = mt.bounds(s, pos_list, id_base, alive)
    assert b[0] == np.inf and b[1] == np.inf and b.dtype == np.float32
    assert (mt.bounds(s, pos_list, id_base, alive, none=-np.inf)[:2] == -np.inf).all()


def test_truth_hand_written_cases_and_the_sign_quirk():
    s = np.asarray([[10.0, 9.6, 9.4, 3.0, -np.inf, 9.4], [-10.0, -9.4, -9.6, -12.0, -9.5, -30.0]], dtype=np.float32)
    pos = [[0], [0]]
    # positive scores: the bound lies BELOW the positive (9.5): 9.6 is dropped, 9.4 kept; the tie 9.4 / 9.4 is id-ascending
    # negative scores: the bound lies ABOVE the positive (-9.5): -9.4 (better than the positive!) is dropped, -9.5 itself is kept
    gs, gi = mt.mine(s, pos, 4, max_ratio=0.95)
    assert gi.tolist() == [[2, 5, 3, -1], [4, 2, 3, 5]]
    assert gs[0].tolist() == [np.float32(9.4), np.float32(9.4), 3.0, -np.inf]
    assert mt.mine(s, pos, 2, max_ratio=0.95, skip_top=1)[1].tolist() == [[5, 3], [2, 3]]
    assert mt.mine(s, pos, 3)[1].tolist() == [[1, 2, 5], [1, 4, 2]]                          # no ratio: only the positive leaves
    assert mt.mine(s, [[], []], 2, max_ratio=0.95)[1].tolist() == [[0, 1], [1, 4]]           # no positive: +inf, nothing dropped
    assert mt.mine(s, pos, 3, alive=[1, 1, 0, 1, 1, 1])[1].tolist() == [[1, 5, 3], [1, 4, 3]]
    assert mt.as_lists(np.asarray([3, -1]), 2) == [[3], [-1]]
    assert mt.as_lists(np.asarray([[3, 4], [-1, -1]]), 2) == [[3, 4], [-1, -1]]
    assert mt.as_lists((np.asarray([3, 4, 9]), np.asarray([0, 2, 3])), 2) == [[3, 4], [9]]
    box, lens = mt.gather(np.arange(12).reshape(6, 2), [0, 1, 4, 4, 6], np.asarray([[11, 12], [9, 13]]), 2, id_base=10)
    assert lens.tolist() == [[2, 0], [0, 2]] and box[0, 0].tolist() == [[2, 3], [4, 5]] and not box[0, 1].any() and not box[1, 0].any()


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_the_header_declares_the_entries_and_the_library_exports_them():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    L = colpali_amd._lib.lib()
    for name in ("msim_mine_bounds", "msim_mine_mask", "msim_gather_pages"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header) and hasattr(L, name)
    assert colpali_amd._lib.ABI_VERSION == L.msim_abi_version()
    assert colpali_amd.mine_hard_negatives is colpali_amd.mine.mine_hard_negatives
    assert colpali_amd.gather_pages is colpali_amd.mine.gather_pages
    assert "mine_hard_negatives" in colpali_amd.__all__ and "gather_pages" in colpali_amd.__all__


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def bounds(scores=FAKE, ld=10, n_q=4, n=10, ids=FAKE, off=FAKE, nnz=5, alive=None, out=FAKE):
        return L.msim_mine_bounds(scores, ld, n_q, n, ids, off, nnz, 0, alive, 0, out, None)

    def mask(scores=FAKE, ld=10, n_q=4, n=10, b=FAKE, ratio=0.95, alive=None, ids=FAKE, off=FAKE, nnz=5):
        return L.msim_mine_mask(scores, ld, n_q, n, b, ratio, alive, ids, off, nnz, 0, None)

    def gather(rows=FAKE, row_bytes=256, d_rows=100, off=FAKE, n_d=10, ids=FAKE, n_slots=6, pad=8, out=FAKE, lens=FAKE):
        return L.msim_gather_pages(rows, row_bytes, d_rows, off, n_d, 0, ids, n_slots, pad, out, lens, None)

    assert bounds(n_q=0, scores=None, ids=None, off=None, out=None) == 0 and mask(n_q=0, scores=None, ids=None, off=None, b=None) == 0
    assert mask(n=0, scores=None) == 0 and gather(n_slots=0, rows=None, off=None, ids=None, out=None, lens=None) == 0
    for kw in (dict(n_q=-1), dict(n=-1), dict(nnz=-1), dict(scores=None), dict(off=None), dict(ids=None), dict(out=None),
               dict(scores=FAKE + 2), dict(off=FAKE + 2), dict(ids=FAKE + 4), dict(out=FAKE + 1), dict(ld=9)):
        assert bounds(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(n=-1), dict(nnz=-1), dict(scores=None), dict(off=None), dict(ids=None), dict(scores=FAKE + 2),
               dict(off=FAKE + 2), dict(ids=FAKE + 4), dict(b=FAKE + 2), dict(ld=9), dict(ratio=float("nan"))):
        assert mask(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(n_slots=-1), dict(n_d=-1), dict(d_rows=-1), dict(pad=-1), dict(row_bytes=0), dict(row_bytes=-16), dict(row_bytes=100),
               dict(row_bytes=24), dict(rows=None), dict(off=None), dict(ids=None), dict(out=None), dict(lens=None), dict(rows=FAKE + 8),
               dict(out=FAKE + 8), dict(ids=FAKE + 4), dict(off=FAKE + 2), dict(lens=FAKE + 2)):
        assert gather(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(row_bytes=1 << 20), dict(d_rows=1 << 31), dict(pad=1 << 31), dict(n_slots=1 << 31)):
        assert gather(**kw) == EUNSUPPORTED, kw


# ------------------------------------------------------------------------------------------ injected stand-ins for the kernels
def _page(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _score_fn(queries, corpus):
    from oracle import maxsim_oracle as mo

    return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))


def _lists(csr, n_q):
    return mt.as_lists((csr[0].numpy(), csr[1].numpy()), n_q)


def _bounds_fn(scores, csr, id_base=0, *, local=False, alive=None):
    return torch.from_numpy(mt.bounds(scores.numpy(), _lists(csr, scores.shape[0]), id_base, None if alive is None else alive.numpy(),
                                      none=-np.inf if local else np.inf))


def _mask_fn(scores, csr, id_base=0, bounds=None, max_ratio=None, alive=None):
    m = mt.masked(scores.numpy(), _lists(csr, scores.shape[0]), id_base, max_ratio, None if alive is None else alive.numpy(),
                  None if bounds is None else bounds.numpy())
    scores.copy_(torch.from_numpy(m))                                    # in place, as the kernel
    return scores


def _hooks():
    from oracle import topk_oracle

    return dict(score_fn=_score_fn, select=topk_oracle.torch_select, mine_bounds_fn=_bounds_fn, mine_mask_fn=_mask_fn)


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors():
    import colpali_amd as amd
    from colpali_amd.mine import positives_csr

    g = torch.Generator().manual_seed(0)
    corpus = amd.pack_passages([_page(g, 5) for _ in range(6)], CPU, batch_size=None)
    q = torch.stack([_page(g, 4) for _ in range(3)])
    pos = torch.tensor([0, 1, -1])
    r = amd.ShardedRetriever(corpus, **_hooks())
    assert r.mine(q, pos, 2)[1].shape == (3, 2)
    for kw in (dict(n_neg=0), dict(n_neg=-3), dict(n_neg=2, skip_top=-1), dict(n_neg=2, max_ratio=0.0), dict(n_neg=2, max_ratio=-0.95),
               dict(n_neg=2, max_ratio=float("inf")), dict(n_neg=2, max_ratio=float("nan"))):
        with pytest.raises(ValueError):
            r.mine(q, pos, **kw)
    for bad in (pos.to(torch.int32), pos.float(), pos[:2], torch.zeros((2, 3), dtype=torch.int64), torch.zeros((3, 2, 2), dtype=torch.int64),
                [0, 1, 2], (torch.tensor([0, 1]), torch.tensor([0, 1, 2, 2])),                     # offsets of the wrong dtype
                (torch.tensor([0, 1]), torch.tensor([0, 1, 2], dtype=torch.int32)),               # ... and of the wrong length
                (torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0, 1, 2, 2], dtype=torch.int32)),
                (torch.tensor([0, 1]),)):
        with pytest.raises(ValueError):
            r.mine(q, bad, 2)
    ids, off = positives_csr(torch.tensor([[4, -1], [5, 6], [-1, -1]]), 3, CPU)
    assert ids.tolist() == [4, -1, 5, 6, -1, -1] and off.tolist() == [0, 2, 4, 6] and off.dtype == torch.int32
    ids, off = positives_csr(pos, 3, CPU)
    assert ids.tolist() == [0, 1, -1] and off.tolist() == [0, 1, 2, 3]
    ids, off = positives_csr(torch.zeros((3, 0), dtype=torch.int64), 3, CPU)
    assert ids.numel() == 0 and off.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError):                                    # a CPU corpus: the GPU-only error, as rerank and align
        amd.mine_hard_negatives(q, corpus, pos, 2)
    with pytest.raises(RuntimeError):
        amd.gather_pages(corpus, torch.zeros((2, 2), dtype=torch.int64))
    with pytest.raises(ValueError):                                      # the kernels have no CPU fallback
        amd.mine.mine_mask(torch.zeros(3, 6), positives_csr(pos, 3, CPU))
    with pytest.raises(ValueError):
        amd.mine.mine_bounds(torch.zeros(3, 6), positives_csr(pos, 3, CPU))


# ------------------------------------------------------------------------------------------------- LiveCorpus.mine, host logic
def test_live_corpus_mine_skips_deleted_slots():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(5)
    pages = [_page(g, n) for n in (4, 1, 6, 3, 9, 2, 5, 7, 3, 4)]
    pages[6] = pages[2].clone()                                          # an exact tie
    live = amd.LiveCorpus(80, 12, CPU, id_base=50, **_hooks())
    live.add(pages)
    q = torch.stack([_page(g, 6) for _ in range(4)])
    pos = torch.tensor([[50, 53], [54, -1], [-1, -1], [57, 51]])
    live.delete([53, 55, 58])                                            # a positive of query 0 among them
    got_s, got_i = live.mine(q, pos, 5, max_ratio=0.95, skip_top=1)
    surv = [c for c in range(10) if c not in (3, 5, 8)]
    fresh = amd.pack_passages([pages[c] for c in surv], CPU, batch_size=None)
    s = _score_fn(q, fresh).numpy()
    where = {50 + c: p for p, c in enumerate(surv)}
    pos_fresh = [[where[i] for i in row if i in where] for row in pos.tolist()]
    want_s, want_i = mt.mine(s, pos_fresh, 5, 0, 0.95, 1)
    want_i = np.where(want_i >= 0, np.asarray(surv + [0])[np.clip(want_i, 0, None)] + 50, -1)
    np.testing.assert_array_equal(got_i.numpy(), want_i)
    np.testing.assert_array_equal(got_s.numpy(), want_s)
    assert not np.isin(got_i.numpy(), [53, 55, 58]).any()
    starved_s, starved_i = live.mine(q, pos, 9)                          # 7 live pages, at most 2 of them positives
    assert (starved_i[:, -1] == -1).all() and torch.isneginf(starved_s[:, -1]).all() and (starved_i[2, :7] >= 0).all()


# ------------------------------------------------------------------------------------------- ShardedRetriever.mine over gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_docs, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd

    g = torch.Generator().manual_seed(21)
    docs = [_page(g, n) for n in torch.randint(1, 30, (n_docs,), generator=g).tolist()]
    q = torch.stack([_page(g, 8) for _ in range(5)])
    docs[1] = torch.cat([q[0], _page(g, 3)])                             # query 0: its positive (page 1, rank 0) holds the query's own
    near = q[0].float()                                                  # tokens, and a near-duplicate of it lives on the LAST rank:
    near[7] = torch.nn.functional.normalize(near[7] + 0.6 * _page(g, 1)[0].float(), dim=-1)      # 7 + ~0.86 of 8 > 0.95 x 8
    docs[n_docs - 2] = torch.cat([near.to(torch.bfloat16), _page(g, 2)])
    docs[4] = docs[n_docs - 3].clone()                                   # an exact tie across shards
    pos = torch.tensor([[1, -1], [n_docs - 1, 0], [-1, -1], [3, 3], [n_docs + 5, 2]])
    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], CPU, batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, **_hooks())
    out = {}
    for name, kw in (("plain", dict(n_neg=6)), ("ratio", dict(n_neg=6, max_ratio=0.95)), ("window", dict(n_neg=4, max_ratio=0.95, skip_top=3)),
                     ("starved", dict(n_neg=n_docs + 2))):
        s, i = r.mine(q, pos, **kw)
        out[name + "_s"], out[name + "_i"] = s.numpy(), i.numpy()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
    if rank == 0:                                                        # the single-shard truth
        full = colpali_amd.pack_passages(docs, CPU, batch_size=None)
        sc = _score_fn(q, full).numpy()
        pl = mt.as_lists(pos.numpy(), 5)
        truth = {}
        for name, kw in (("plain", dict(n_neg=6)), ("ratio", dict(n_neg=6, max_ratio=0.95)),
                         ("window", dict(n_neg=4, max_ratio=0.95, skip_top=3)), ("starved", dict(n_neg=n_docs + 2))):
            truth[name + "_s"], truth[name + "_i"] = mt.mine(sc, pl, **kw)
        # the planted near-duplicate scores above 0.95 x the positive's score: only a bound that crossed the ranks can drop it
        truth["planted"] = np.asarray([sc[0, n_docs - 2] > np.float32(0.95) * sc[0, 1], sc[0, 1] == sc[0].max()])
        np.savez(os.path.join(out_dir, "truth.npz"), **truth)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs", [(2, 23), (3, 31)])
def test_sharded_mine_equals_the_single_shard_truth(tmp_path, world, n_docs):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    assert truth["planted"].all()
    assert n_docs - 2 in truth["plain_i"][0] and n_docs - 2 not in truth["ratio_i"][0]       # dropped by the other rank's positive
    assert (truth["starved_i"][:, -1] == -1).all() and np.isneginf(truth["starved_s"][:, -1]).all()
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in truth.files:
            if key != "planted":
                np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
