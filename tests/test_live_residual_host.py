"""The live compressed shard without a GPU (colpali_amd.LiveResidualCorpus, include/maxsim.h: msim_res_append,
msim_res_live_compact): the ABI's argument checks (refused before any device work), the binding and the header, and the class' host
logic over a seeded history with every kernel replaced by its numpy truth -- `encode_fn` from tests/centroid_truth.py: codes +
tests/residual_truth.py: encode, `compact_fn` from tests/live_truth.py, numpy scorers -- checked against those truths applied to the
surviving pages."""
import os
import re

import numpy as np
import pytest
import torch

from tests import centroid_truth as ct
from tests import live_truth as lt
from tests import residual_truth as rt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------------------------ the ABI
def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def append(dtype=0, d=FAKE, off=FAKE, n_d=3, n_rows=10, dim=128, longest=5, C=FAKE, K=256, cut=FAKE, bits=2, codes=FAKE, res=FAKE,
               row0=7, dst_rows=17, status=FAKE):
        return L.msim_res_append(dtype, d, off, n_d, n_rows, dim, longest, C, K, cut, bits, codes, res, row0, dst_rows, status, None)

    def compact(codes=FAKE, res=FAKE, bits=2, bound=1000, off=FAKE, alive=FAKE, n=10, used=FAKE, ws=FAKE, bounce=FAKE, bounce_bytes=4096):
        return L.msim_res_live_compact(codes, res, bits, bound, off, alive, n, used, ws, bounce, bounce_bytes, None)

    assert append(n_d=0) == 0 and append(longest=0) == 0 and append(n_d=0, d=None, off=None, C=None, cut=None, codes=None, res=None) == 0
    for kw in (dict(n_d=-1), dict(n_rows=-1), dict(longest=-1), dict(row0=-1), dict(dst_rows=-1), dict(row0=8), dict(dst_rows=16),
               dict(dim=320), dict(dim=64), dict(K=100), dict(K=4096), dict(d=None), dict(off=None), dict(C=None), dict(cut=None),
               dict(codes=None), dict(res=None), dict(d=FAKE + 8), dict(C=FAKE + 2), dict(codes=FAKE + 2), dict(res=FAKE + 4),
               dict(off=FAKE + 2), dict(status=FAKE + 2), dict(cut=FAKE + 2)):
        assert append(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(bits=3), dict(bits=0), dict(longest=65536 * 256, n_rows=1 << 25, dst_rows=1 << 26)):
        assert append(**kw) == EUNSUPPORTED, kw

    wsq = L.msim_res_live_compact_workspace_bytes
    assert wsq(0, 1 << 20) == 0 and wsq(-3, 0) == 0
    w = wsq(125_000, 256 << 20)
    assert w % 16 == 0 and w >= 4 * 125_001 and wsq(250_000, 256 << 20) > w
    assert compact(n=0) == 0 and compact(n=0, codes=None, res=None, off=None, alive=None, used=None, ws=None, bounce=None) == 0
    for kw in (dict(n=-1), dict(bound=-1), dict(bounce_bytes=-1), dict(codes=None), dict(res=None), dict(off=None), dict(alive=None),
               dict(used=None), dict(ws=None), dict(bounce=None), dict(codes=FAKE + 2), dict(res=FAKE + 8), dict(bounce=FAKE + 4),
               dict(ws=FAKE + 8), dict(off=FAKE + 2), dict(used=FAKE + 4), dict(bounce_bytes=33), dict(bounce_bytes=0),
               dict(bits=4, bounce_bytes=65)):
        assert compact(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(bits=3), dict(bits=8), dict(bound=1 << 31), dict(bound=1 << 24, bounce_bytes=34)):
        assert compact(**kw) == EUNSUPPORTED, kw
    # msim_live_compact keeps its contract: rows that are no multiple of 16 bytes are not its business
    assert L.msim_live_compact(FAKE, 2, 1000, FAKE, FAKE, 10, FAKE, FAKE, FAKE, 4096, None) == EINVAL


def test_binding_and_header_declare_the_new_entries():
    import colpali_amd

    L = colpali_amd._lib.lib()
    for name, n_args in (("msim_res_append", 17), ("msim_res_live_compact", 12), ("msim_res_live_compact_workspace_bytes", 2)):
        assert len(getattr(L, name).argtypes) == n_args
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    for name in ("msim_res_append", "msim_res_live_compact"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert re.search(r"\bsize_t\s+msim_res_live_compact_workspace_bytes\s*\(\s*int n_slots,\s*int64_t bounce_bytes\s*\)\s*;", header)
    assert "floor(bounce_bytes / (16 * bits + 2))" in header and "dst_row0 + r" in header
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)


# ------------------------------------------------------------------------------------------------------- numpy stand-ins (hooks)
def _f32(t):
    return t.float().numpy()


def _u16(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def _page(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _decoded(rc):
    kind = "f16" if rc.dtype == torch.float16 else "bf16"
    bits16 = rt.decode(_f32(rc.centroids), _u16(rc.codes), rc.residuals.numpy(), rc.weights.numpy(), rc.bits, kind)
    return rt.from_bits(bits16, kind)


def _maxsim(queries, xhat, off):
    out = np.full((len(queries), len(off) - 1), -np.inf, dtype=np.float32)
    for i, q in enumerate(queries):
        for c in range(len(off) - 1):
            if off[c + 1] > off[c]:
                out[i, c] = np.float32((_f32(q).astype(np.float64) @ xhat[off[c]:off[c + 1]].astype(np.float64).T).max(axis=1).sum())
    return out


def score_fn(queries, rc):
    return torch.from_numpy(_maxsim(queries, _decoded(rc), rc.offsets.numpy().astype(np.int64)))


def rerank_fn(queries, rc, candidates):
    full = score_fn(queries, rc)
    n = full.shape[1]
    d = candidates - rc.id_base
    ok = (candidates >= 0) & (d >= 0) & (d < n)
    got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0)))
    return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))


def centroid_score_fn(queries, index):
    q_off = np.concatenate([[0], np.cumsum([len(q) for q in queries])])
    table = ct.table(np.concatenate([_f32(q) for q in queries]), _f32(index.centroids))
    return torch.from_numpy(ct.scores(table, q_off, _u16(index.codes), index.offsets.numpy()))


def mask_fn(scores, alive):
    return torch.from_numpy(lt.mask(scores.numpy(), alive.numpy()))


CALLS = {"encode": 0}


def encode_fn(live, rows, offsets, n_pages, max_rows, dst_row0):
    CALLS["encode"] += 1
    off = offsets.numpy()
    assert off[0] == 0 and off[-1] == rows.shape[0] and len(off) == n_pages + 1 and (np.diff(off) <= max_rows).all() and (np.diff(off) > 0).all()
    x, C = _f32(rows), _f32(live.centroids)
    codes = ct.codes(x, C)
    n = len(codes)
    _u16(live.codes)[dst_row0:dst_row0 + n] = codes
    live.residuals.numpy()[dst_row0:dst_row0 + n] = rt.encode(x, C, codes, live.cutoffs.numpy(), live.bits)


def compact_fn(live, rows_bound):
    n = live.n_slots
    off, alive = live.offsets.numpy()[:n + 1].copy(), live.alive.numpy()[:n]
    assert off[-1] == rows_bound
    _u16(live.codes)[:] = lt.compact_rows(_u16(live.codes), off, alive)
    live.residuals.numpy()[:] = lt.compact_rows(live.residuals.numpy(), off, alive)
    live.offsets.numpy()[:n + 1] = lt.compact_offsets(off, alive)


def _hooks():
    from oracle import topk_oracle

    return dict(rerank_fn=rerank_fn, centroid_score_fn=centroid_score_fn, select=topk_oracle.torch_select, mask_fn=mask_fn,
                encode_fn=encode_fn, compact_fn=compact_fn)


def _codec(g, bits, k=256, dtype=torch.bfloat16):
    C = _page(g, k, dtype)
    cut = torch.sort(torch.randn((1 << bits) - 1, generator=g) * 0.05).values.contiguous()
    w = torch.sort(torch.randn(1 << bits, generator=g) * 0.08).values.contiguous()
    return C, cut, w


class Truth:
    """The pages by slot and the truth of what the shard holds."""

    def __init__(self, amd, live):
        self.amd, self.live, self.pages, self.table = amd, live, [], lt.SlotTable(live.id_base)

    def add(self, pages, as_tensor=False):
        got = self.live.add(torch.stack(pages) if as_tensor else pages)
        assert got.tolist() == self.table.add([len(p) for p in pages]) and got.dtype == torch.int64
        self.pages += pages

    def expected(self, slots):
        """(codes, residuals, offsets) of the truth encode over the pages of `slots`, back to back"""
        live = self.live
        C = _f32(live.centroids)
        x = np.concatenate([_f32(self.pages[s]) for s in slots] + [np.zeros((0, 128), np.float32)])
        codes = ct.codes(x, C) if len(x) else np.zeros(0, np.uint16)
        res = rt.encode(x, C, codes, live.cutoffs.numpy(), live.bits) if len(x) else np.zeros((0, 16 * live.bits), np.uint8)
        return codes, res, np.concatenate([[0], np.cumsum([len(self.pages[s]) for s in slots])]).astype(np.int64)

    def check(self, queries, k, cand):
        amd, live, table = self.amd, self.live, self.table
        holders = [s for s, n in enumerate(table.lengths) if n > 0]                    # slots that own rows now, deleted or not
        codes, res, _ = self.expected(holders)
        v = live.view()
        assert live.rows_used == table.rows_used == len(codes) and len(live) == len(self.pages) == len(v)
        np.testing.assert_array_equal(v.offsets.numpy(), table.offsets())
        np.testing.assert_array_equal(_u16(v.codes)[:len(codes)], codes)
        np.testing.assert_array_equal(v.residuals.numpy()[:len(codes)], res)
        np.testing.assert_array_equal(live.alive[:len(live)].numpy(), np.asarray(table.alive, dtype=np.uint8))
        assert v.lengths.tolist() == table.lengths and v.codes.data_ptr() == live.codes.data_ptr() and v.clamp0 is None
        surv = table.survivors()
        s_codes, s_res, s_off = self.expected(surv)
        if not surv:
            got_s, got_i = live.search(queries, k, candidates=cand)
            assert np.isneginf(got_s.numpy()).all() and (got_i.numpy() == -1).all()
            return
        R = amd.ResidualCorpus(live.centroids, torch.from_numpy(s_codes.view(np.int16).copy()).view(torch.uint16), torch.from_numpy(s_res.copy()),
                               live.cutoffs, live.weights, torch.from_numpy(s_off.astype(np.int32)), None,
                               torch.from_numpy(np.diff(s_off)), 0, live.bits)
        hooks = {k_: f for k_, f in _hooks().items() if k_ in ("rerank_fn", "centroid_score_fn", "select")}
        ref = amd.ShardedRetriever(R, score_fn=score_fn, **hooks)
        pos = {s + live.id_base: p for p, s in enumerate(surv)}
        tcand = torch.tensor([[pos.get(int(c), -1) for c in row] for row in cand.tolist()], dtype=torch.int64)
        for got, want in ((live.search(queries, k, candidates=cand), ref.search(queries, k, candidates=tcand)),
                          (live.search(queries, k, prefilter=live.index, n_candidates=6), ref.search(queries, k, prefilter=R.index, n_candidates=6)),
                          (live.search(queries, k), ref.search(queries, k))):
            np.testing.assert_array_equal(got[0].numpy().view(np.int32), want[0].numpy().view(np.int32))
            np.testing.assert_array_equal(got[1].numpy(), lt.expected_ids(want[1].numpy(), surv, live.id_base))


@pytest.mark.parametrize("bits,dtype,ingest_rows", [(2, torch.bfloat16, 7), (4, torch.float16, None)])
def test_a_history_with_injected_truths(bits, dtype, ingest_rows):
    import colpali_amd as amd

    g = torch.Generator().manual_seed(40 + bits)
    C, cut, w = _codec(g, bits, dtype=dtype)
    live = amd.LiveResidualCorpus(C, cut, w, bits, 400, 30, id_base=20, ingest_rows=ingest_rows, score_fn=score_fn, **_hooks())
    assert live.ingest_rows == (7 if ingest_rows else 400) and live.device == CPU and live.dtype == dtype and len(live.view()) == 0
    t = Truth(amd, live)
    queries = [_page(g, n, dtype) for n in (5, 1, 9)]
    cand = torch.randint(15, 45, (3, 8), generator=g)                                 # ids below, inside and above the shard
    cand[1, :] = -1
    lens = [3, 1, 20, 7, 2, 11]
    CALLS["encode"] = 0
    t.add([_page(g, n, dtype) for n in lens])
    assert CALLS["encode"] == (-(-sum(lens) // 7) if ingest_rows else 1)              # rounds of ingest_rows rows; a page straddles them
    t.check(queries, 4, cand)
    t.add([_page(g, 4, dtype) for _ in range(3)], as_tensor=True)                      # a [n, rows, 128] tensor: one call, never the ingest buffer
    t.check(queries, 4, cand)
    live.delete([20, 23])
    t.table.delete([20, 23])
    t.check(queries, 4, cand)
    old_view, old_index = live.view(), live.index
    live.compact()
    t.table.compact()
    t.check(queries, 4, cand)
    # a view made before add / compact keeps the page count and lengths of its time: it is no longer the shard
    assert old_view.lengths.tolist() != live.view().lengths.tolist() and old_index.codes.data_ptr() == live.index.codes.data_ptr()
    before = (_u16(live.codes).copy(), live.offsets.clone())
    live.compact()                                                                    # nothing to hand back
    assert (before[0] == _u16(live.codes)).all() and torch.equal(before[1], live.offsets)
    live.delete(torch.tensor([28, 21]))                                               # a host tensor follows the host rules
    t.table.delete([28, 21])
    t.add([_page(g, n, dtype) for n in (6, 1)])                                        # ids are not reused, rows go to the tail
    assert len(live.view()) == len(old_view) + 2
    t.check(queries, 40, cand)                                                        # k above the number of live pages
    live.compact()
    t.table.compact()
    t.check(queries, 4, cand)
    live.delete([s + 20 for s in t.table.survivors()])
    t.table.delete([s + 20 for s in t.table.survivors()])
    t.check(queries, 4, cand)
    live.compact()
    t.table.compact()
    assert live.rows_used == 0 and live.n_live == 0
    t.add([_page(g, 5, dtype)])
    assert live.view().offsets[-2].item() == 0
    t.check(queries, 4, cand)


def _state(live):
    return (live.n_slots, live.rows_used, live.offsets.clone(), live.alive.clone(), live.codes.view(torch.int16).clone(), live.residuals.clone())


def _same(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))


def test_host_rules_and_refusals():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(3)
    C, cut, w = _codec(g, 2)
    live = amd.LiveResidualCorpus(C, cut, w, 2, 20, 4, id_base=100, **_hooks())
    assert live.add([_page(g, 5), _page(g, 1), _page(g, 7)]).tolist() == [100, 101, 102]
    assert live.rows_used == 13 and live.offsets.tolist() == [0, 5, 6, 13, 0] and live.alive.tolist() == [1, 1, 1, 0, 0]
    before = _state(live)
    with pytest.raises(RuntimeError, match="capacity_rows=20"):
        live.add([_page(g, 8)])
    with pytest.raises(RuntimeError, match="capacity_docs=4"):
        live.add([_page(g, 1), _page(g, 1)])
    with pytest.raises(RuntimeError, match="capacity_docs=4"):
        live.add(_page(g, 6).reshape(2, 3, 128))
    with pytest.raises(ValueError, match="0 rows"):
        live.add([_page(g, 2), _page(g, 0)])
    with pytest.raises(ValueError, match="0 rows"):
        live.add(torch.zeros(2, 0, 128, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="width"):
        live.add([torch.zeros(2, 64, dtype=torch.bfloat16)])
    with pytest.raises(RuntimeError, match="width"):
        live.add([_page(g, 2, torch.float16)])
    with pytest.raises(ValueError, match="3-D"):
        live.add(_page(g, 2))
    for bad in ([99], [103], [-1], [100, 100], [101, 7]):
        with pytest.raises(KeyError):
            live.delete(bad)
    assert _same(before, _state(live))                                    # every refusal left the shard as it was
    # a default instance scans on request only: ShardedRetriever's refusal, on every route that reads every row
    q = [_page(g, 4)]
    for kw in (dict(), dict(group_by=object()), dict(filter=object())):
        with pytest.raises(NotImplementedError, match="score_fn=residual_scores"):
            live.search(q, 2, **kw)
    with pytest.raises(NotImplementedError, match="score_fn=residual_scores"):
        live.mine(q, [[100]], 2)
    live.delete([101])
    s, i = live.search(q, 3, candidates=torch.tensor([[101, 102, 100, 7]]))
    assert sorted(i[0].tolist()) == [-1, 100, 102] and np.isneginf(s[0, 2].item())
    assert live.add(_page(g, 3).reshape(1, 3, 128)).tolist() == [103] and live.n_live == 3 and len(live) == 4
    # the default hooks are gfx950 kernels: no CPU fallback
    plain = amd.LiveResidualCorpus(C, cut, w, 2, 20, 4)
    with pytest.raises(RuntimeError, match="gfx950"):
        plain.add([_page(g, 2)])
    plain._lengths[:1], plain._alive_h[:1], plain.n_slots, plain._rows_used = 2, False, 1, 2
    with pytest.raises(RuntimeError, match="gfx950"):
        plain.compact()
    # the formats of ResidualCorpus, with its exceptions
    with pytest.raises(ValueError, match="bits"):
        amd.LiveResidualCorpus(C, cut, w, 3, 20, 4)
    with pytest.raises(ValueError, match="cutoffs"):
        amd.LiveResidualCorpus(C, cut, w, 4, 20, 4)
    with pytest.raises(ValueError):
        amd.LiveResidualCorpus(C[:100], cut, w, 2, 20, 4)
    with pytest.raises(NotImplementedError):
        amd.LiveResidualCorpus(C.float(), cut, w, 2, 20, 4)
    with pytest.raises(ValueError, match="positive"):
        amd.LiveResidualCorpus(C, cut, w, 2, 0, 4)
    with pytest.raises(ValueError, match="bounce_bytes"):
        amd.LiveResidualCorpus(C, cut, w, 2, 20, 4, bounce_bytes=33)


def test_like_and_from_residual():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(4)
    C, cut, w = _codec(g, 4)
    src = amd.LiveResidualCorpus(C, cut, w, 4, 30, 5, id_base=7, **_hooks())
    src.add([_page(g, n) for n in (4, 1, 6)])
    rc = src.view()
    empty = amd.LiveResidualCorpus.like(rc, 50, 9, **_hooks())
    assert (len(empty), empty.rows_used, empty.bits, empty.id_base, empty.capacity_rows) == (0, 0, 4, 0, 50)
    assert empty.centroids.data_ptr() == C.data_ptr() and empty.residuals.shape == (50, 64)
    live = amd.LiveResidualCorpus.from_residual(rc, spare_rows=10, spare_docs=3, **_hooks())
    assert (live.capacity_rows, live.capacity_docs, live.id_base, live.rows_used, len(live)) == (21, 6, 7, 11, 3)
    v = live.view()
    assert torch.equal(v.codes.view(torch.int16), rc.codes.view(torch.int16)) and torch.equal(v.residuals, rc.residuals)
    assert torch.equal(v.offsets, rc.offsets) and v.lengths.tolist() == [4, 1, 6] and v.codes.data_ptr() != rc.codes.data_ptr()
    assert live.add(torch.stack([_page(g, 3), _page(g, 3)])).tolist() == [10, 11] and live.view().offsets.tolist() == [0, 4, 5, 11, 14, 17]
    clamped = amd.ResidualCorpus(C, rc.codes, rc.residuals, cut, w, rc.offsets, torch.zeros(3, dtype=torch.uint8), rc.lengths, 0, 4)
    with pytest.raises(ValueError, match="clamp0"):
        amd.LiveResidualCorpus.from_residual(clamped, 1, 1)
    with pytest.raises(ValueError, match="ResidualCorpus"):
        amd.LiveResidualCorpus.like(object(), 1, 1)
