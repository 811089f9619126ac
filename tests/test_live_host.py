"""The live corpus without a GPU: the ABI's argument checks (no device work), the numpy restatement (tests/live_truth.py) on
hand-written cases, LiveCorpus' host rules, and two live shards over a gloo world of 2 with the oracle injected: every rank must get
the unsharded answer over the surviving pages, with deleted pages absent."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import live_truth as lt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def compact(rows=FAKE, row_bytes=256, bound=1000, off=FAKE, alive=FAKE, n=10, used=FAKE, ws=FAKE, bounce=FAKE, bounce_bytes=4096):
        return L.msim_live_compact(rows, row_bytes, bound, off, alive, n, used, ws, bounce, bounce_bytes, None)

    def mask(scores=FAKE, ld=10, n_q=4, n=10, alive=FAKE):
        return L.msim_live_mask_scores(scores, ld, n_q, n, alive, None)

    assert L.msim_live_compact_workspace_bytes(0, 1 << 20) == 0 and L.msim_live_compact_workspace_bytes(-3, 0) == 0
    w = L.msim_live_compact_workspace_bytes(125_000, 256 << 20)
    assert w % 16 == 0 and w >= 4 * 125_001 and L.msim_live_compact_workspace_bytes(250_000, 256 << 20) > w
    assert compact(n=0) == 0 and compact(n=0, rows=None, off=None, alive=None, used=None, ws=None, bounce=None) == 0
    assert mask(n_q=0) == 0 and mask(n=0, scores=None, alive=None) == 0 and mask(n_q=0, n=0, ld=0) == 0
    for kw in (dict(n=-1), dict(bound=-1), dict(bounce_bytes=-1), dict(row_bytes=0), dict(row_bytes=-16), dict(row_bytes=100),
               dict(row_bytes=24), dict(rows=None), dict(off=None), dict(alive=None), dict(used=None), dict(ws=None), dict(bounce=None),
               dict(rows=FAKE + 8), dict(bounce=FAKE + 4), dict(ws=FAKE + 8), dict(off=FAKE + 2), dict(used=FAKE + 4),
               dict(bounce_bytes=255), dict(bounce_bytes=0), dict(row_bytes=512, bounce_bytes=256)):
        assert compact(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(row_bytes=1 << 20, bounce_bytes=1 << 21), dict(bound=1 << 31), dict(bound=1 << 24, bounce_bytes=256)):
        assert compact(**kw) == EUNSUPPORTED, kw
    for kw in (dict(n_q=-1), dict(n=-1), dict(scores=None), dict(alive=None), dict(scores=FAKE + 2), dict(ld=9)):
        assert mask(**kw) == EINVAL, kw
        assert L.msim_last_error()


# ------------------------------------------------------------------------------------------------------------ the restatement
OFF = [0, 3, 4, 9, 9, 12, 20]         # six slots of 3, 1, 5, 0 (compacted away earlier), 3 and 8 rows


@pytest.mark.parametrize("alive,new_off,moves", [
    ([1, 1, 1, 0, 1, 1], [0, 3, 4, 9, 9, 12, 20], []),                                         # nothing to hand back
    ([0, 1, 1, 0, 1, 1], [0, 0, 1, 6, 6, 9, 17], [(3, 0, 1), (4, 1, 5), (9, 6, 3), (12, 9, 8)]),  # the first page
    ([1, 1, 1, 0, 1, 0], [0, 3, 4, 9, 9, 12, 12], []),                                         # the last page: nothing moves
    ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0], []),                                           # every page
    ([1, 0, 0, 0, 1, 1], [0, 3, 3, 3, 3, 6, 14], [(9, 3, 3), (12, 6, 8)]),                     # adjacent dead slots
    ([1, 0, 1, 0, 0, 1], [0, 3, 3, 8, 8, 8, 16], [(4, 3, 5), (12, 8, 8)]),
])
def test_truth_on_hand_written_cases(alive, new_off, moves):
    assert lt.compact_offsets(OFF, alive).tolist() == new_off
    assert lt.move_list(OFF, alive) == moves
    assert lt.moved_bytes(OFF, alive, 256) == 4 * 256 * sum(m[2] for m in moves)
    rows = np.arange(20 * 2).reshape(20, 2)
    out = lt.compact_rows(rows, OFF, alive)
    want = np.concatenate([rows[OFF[c]:OFF[c + 1]] for c in range(6) if alive[c]] + [rows[:0]])
    np.testing.assert_array_equal(out[:new_off[-1]], want)
    first = min([m[1] for m in moves], default=20)
    np.testing.assert_array_equal(out[:first], rows[:first])            # rows below the first move are untouched
    # compaction twice is a no-op the second time
    assert lt.compact_offsets(new_off, alive).tolist() == new_off and lt.move_list(new_off, alive) == []
    np.testing.assert_array_equal(lt.compact_rows(out, new_off, alive), out)


def test_truth_mask_ids_and_slot_table():
    s = np.arange(12, dtype=np.float32).reshape(2, 6)
    m = lt.mask(s, [1, 0, 1, 1, 0, 0])
    assert np.isneginf(m[:, [1, 4, 5]]).all() and (m[:, [0, 2, 3]] == s[:, [0, 2, 3]]).all()
    assert lt.expected_ids([[1, 0, -1], [2, -1, -1]], [0, 2, 3], id_base=10).tolist() == [[12, 10, -1], [13, -1, -1]]
    t = lt.SlotTable(id_base=5)
    assert t.add([3, 1, 5]) == [5, 6, 7] and t.add([2]) == [8]
    t.delete([6, 8])
    for bad in ([6], [4], [9], [5, 5]):
        with pytest.raises(KeyError):
            t.delete(bad)
    assert t.survivors() == [0, 2] and t.rows_used == 11 and t.offsets().tolist() == [0, 3, 4, 9, 11]
    t.compact()
    assert t.rows_used == 8 and t.offsets().tolist() == [0, 3, 3, 8, 8]
    assert t.add([4]) == [9] and t.survivors() == [0, 2, 4]             # ids are never reused
    with pytest.raises(ValueError):
        t.add([0])


# ------------------------------------------------------------------------------------------------------- LiveCorpus' host rules
def _page(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _state(live):
    return (live.n_slots, live.rows_used, live.offsets.clone(), live.alive.clone(), live.blob.clone())


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))


def test_live_corpus_host_rules():
    import colpali_amd

    g = torch.Generator().manual_seed(3)
    live = colpali_amd.LiveCorpus(20, 4, CPU, id_base=100)
    assert len(live) == 0 and live.rows_used == 0 and len(live.view()) == 0
    ids = live.add([_page(g, 5), _page(g, 1), _page(g, 7)])
    assert ids.tolist() == [100, 101, 102] and ids.dtype == torch.int64
    assert live.rows_used == 13 and live.offsets.tolist() == [0, 5, 6, 13, 0] and live.alive.tolist() == [1, 1, 1, 0, 0]
    before = _state(live)
    with pytest.raises(RuntimeError, match="capacity_rows=20"):
        live.add([_page(g, 8)])
    with pytest.raises(RuntimeError, match="capacity_docs=4"):
        live.add([_page(g, 1), _page(g, 1)])
    with pytest.raises(ValueError, match="0 rows"):
        live.add([_page(g, 2), _page(g, 0)])
    with pytest.raises(ValueError, match="0 rows"):
        live.add(torch.zeros(2, 0, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="width"):
        live.add([_page(g, 2, dim=64)])
    with pytest.raises(RuntimeError, match="width"):
        live.add([_page(g, 2, dtype=torch.float16)])
    for bad in ([99], [103], [104], [-1], [100, 100], [101, 7]):
        with pytest.raises(KeyError):
            live.delete(bad)
    assert _same(before, _state(live))                                   # every refusal left the corpus as it was
    live.delete([101])
    with pytest.raises(KeyError):
        live.delete([101])                                               # already deleted
    with pytest.raises(KeyError):
        live.delete(torch.tensor([102, 101]))                            # a host tensor follows the host rules; 102 stays
    assert live.alive.tolist() == [1, 0, 1, 0, 0] and live.n_live == 2 and len(live) == 3
    with pytest.raises(RuntimeError, match="capacity_docs=4"):
        live.add(_page(g, 6).reshape(2, 3, 128))                         # a [n, rows, width] tensor of two pages: one slot is left
    assert live.add(_page(g, 3).reshape(1, 3, 128)).tolist() == [103]    # the deleted page's id is not handed out again
    assert live.rows_used == 16 and live.view().lengths.tolist() == [5, 1, 7, 3] and live.add([]).numel() == 0


def test_live_corpus_views_and_from_packed():
    import colpali_amd

    g = torch.Generator().manual_seed(4)
    pages = [_page(g, n) for n in (4, 1, 6)]
    packed = colpali_amd.pack_passages(pages, CPU, batch_size=None, id_base=7)
    live = colpali_amd.LiveCorpus.from_packed(packed, spare_rows=10, spare_docs=3)
    assert (live.capacity_rows, live.capacity_docs, live.id_base, live.rows_used, len(live)) == (21, 6, 7, 11, 3)
    v = live.view()
    assert torch.equal(v.blob, packed.blob) and torch.equal(v.offsets, packed.offsets) and v.clamp0 is None
    assert v.lengths.tolist() == [4, 1, 6] and v.id_base == 7 and v.blob.data_ptr() == live.blob.data_ptr()
    assert live.add(torch.stack([_page(g, 3), _page(g, 3)])).tolist() == [10, 11]
    assert live.view().offsets.tolist() == [0, 4, 5, 11, 14, 17] and live.rows_used == 17
    with pytest.raises(ValueError, match="clamp0"):
        colpali_amd.LiveCorpus.from_packed(colpali_amd.pack_passages(pages, CPU, batch_size=2), 1, 1)
    with pytest.raises(ValueError, match="0 rows"):
        colpali_amd.LiveCorpus.from_packed(colpali_amd.pack_passages(pages + [_page(g, 0)], CPU, batch_size=None), 1, 1)
    with pytest.raises(RuntimeError, match="gfx950"):
        live.delete([8])
        live.compact()                                                   # compaction is a kernel: no CPU fallback
    with pytest.raises(ValueError):
        colpali_amd.live.mask_scores(torch.zeros(2, 5), live.alive)      # so is the mask
    with pytest.raises(ValueError):
        colpali_amd.LiveCorpus(0, 4, CPU)
    f32 = colpali_amd.LiveCorpus(8, 2, CPU, dtype=torch.float32, width=100)
    assert f32.blob.shape == (8, 104)                                    # the generic kernels' padded width
    f32.add([torch.ones(2, 100)])
    assert f32.blob[:2, :100].eq(1).all() and f32.blob[:2, 100:].eq(0).all()


# ------------------------------------------------------------------------------------------------- two live shards over gloo
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
    docs = [_page(g, n) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across pages
    docs[n_docs - 3] = docs[2].clone()        # ... and across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)
    cand = torch.randint(-3, n_docs + 3, (4, m), generator=g)
    cand[2, 0] = cand[2, 1]
    deleted = sorted(set(torch.randint(0, n_docs, (n_docs // 3,), generator=g).tolist()) | {2})

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
        from tests import live_truth

        return torch.from_numpy(live_truth.mask(scores.numpy(), alive.numpy()))

    hooks = dict(score_fn=score_fn, rerank_fn=rerank_fn, select=topk_oracle.torch_select, mask_fn=mask_fn)
    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    live = colpali_amd.LiveCorpus(sum(lens[lo:hi]) + 5, hi - lo + 2, CPU, id_base=lo, **hooks)
    half = (hi - lo) // 2
    live.add(docs[lo:lo + half])                                          # two arrivals; ids follow the arrival order
    live.delete([i for i in deleted if lo <= i < lo + half])
    assert live.add(docs[lo + half:hi]).tolist() == list(range(lo + half, hi))
    live.delete([i for i in deleted if lo + half <= i < hi])
    s, i = live.search(q, k=k, world=world, rank=rank, dist=dist)
    cs, ci = live.search(q, k=k, candidates=cand, world=world, rank=rank, dist=dist)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), s=s.numpy(), i=i.numpy(), cs=cs.numpy(), ci=ci.numpy())

    if rank == 0:                             # unsharded truth over the surviving pages, positions mapped back to ids
        from tests import live_truth

        surv = [d for d in range(n_docs) if d not in deleted]
        full = colpali_amd.pack_passages([docs[d] for d in surv], CPU, batch_size=None)
        ts, ti = topk_oracle.topk(score_fn(q, full).numpy(), k)
        pos = {d: p for p, d in enumerate(surv)}
        tcand = torch.tensor([[pos.get(int(c), -1) for c in row] for row in cand])
        rs, ri = rerank_fn(q, full, tcand)
        tcs, tci = topk_oracle.topk(rs.numpy(), k, 0, ri.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), s=ts, i=live_truth.expected_ids(ti, surv), cs=tcs, ci=live_truth.expected_ids(tci, surv),
                 deleted=np.asarray(deleted))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (2, 12, 10, 6)])
def test_two_live_shards_give_the_unsharded_answer(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("i", "s", "ci", "cs"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
        assert not np.isin(got["i"], truth["deleted"]).any() and not np.isin(got["ci"], truth["deleted"]).any()
    if k > n_docs - len(truth["deleted"]):                                # fewer live pages than k: the tail is (-inf, -1)
        assert (truth["i"][:, -1] == -1).all() and np.isneginf(truth["s"][:, -1]).all()
