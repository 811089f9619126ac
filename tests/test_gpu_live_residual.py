"""The live compressed shard on the MI355X (colpali_amd.LiveResidualCorpus, msim_res_append, msim_res_live_compact).

Everything here is bit for bit, nothing has a tolerance:
  * the fused append-encode against the two entries it fuses (msim_cent_encode_docs, then msim_res_encode_docs) on the same inputs,
    at the tile, wave and workgroup edges of the encode mapping, written at an odd row of sentinel-filled arrays;
  * the compaction of both arrays against tests/live_truth.py, with a bounce buffer of 5 rows and with one that holds everything;
  * the class over a history of add / delete / compact: after every step `view()` holds the bits of `ResidualCorpus.build` over the
    packed survivors and `search` returns what `ShardedRetriever` returns over that corpus, positions mapped back to slots.
"""
import numpy as np
import pytest
import torch

from tests import live_truth as lt
from tests.test_gpu_live import Model

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EINVAL, EUNSUPPORTED = -1, -2
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _rows(g, n, dtype):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _u16(t):
    return t.detach().cpu().view(torch.int16).numpy().view(np.uint16)


def _codec(g, bits, k, dtype):
    """unit centroids with two identical rows (3 and 5), cutoffs with one that is exactly 0.0, sorted weights"""
    C = _rows(g, k, dtype)
    C[5] = C[3]
    nb = 1 << bits
    cut = torch.sort(torch.randn(nb - 1, generator=g) * 0.05).values
    cut[(nb - 1) // 2] = 0.0
    cut = torch.sort(cut).values.contiguous()
    w = torch.sort(torch.randn(nb, generator=g) * 0.08).values.contiguous()
    return C, cut, w


# ------------------------------------------------------------------------------------------------------------- 1. the fused encode
LENS = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("K", [256, 512])
def test_fused_append_has_the_bits_of_the_two_entries_it_fuses(amd, dtype, bits, K):
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(100 * bits + K + (dtype == torch.float16))
    C, cut, _ = _codec(g, bits, K, dtype)
    # pages: the edge lengths, one page longer than max_doc_rows in the middle, and a last page whose offsets run past n_rows
    lens = LENS[:6] + [301] + LENS[6:] + [40]
    max_doc_rows = 300
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    n_rows = int(off[-1]) - 5                                             # the array ends 5 rows before the last page does
    bad_pages = [6, len(lens) - 1]
    D = _rows(g, n_rows, dtype)
    copies = torch.randperm(n_rows, generator=g)[:200]
    D[copies] = C[torch.randint(0, K, (200,), generator=g)]               # exact copies of a centroid: residual 0 == a cutoff
    D[copies[:20]] = C[5]                                                 # ... of the doubled centroid: the lower k must win
    dtc = amd._lib.dtype_code(dtype)
    dD, dC, dcut, doff = D.to(DEV), C.to(DEV), cut.to(DEV), torch.from_numpy(off).to(DEV)
    st = None

    # the composition, at row 0 of arrays of its own
    ref_codes = torch.full((2 * n_rows,), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.int16)
    ref_res = torch.full((n_rows, 16 * bits), SENTINEL, dtype=torch.uint8, device=DEV)
    ref_status = torch.full((len(lens),), 7, dtype=torch.int32, device=DEV)
    assert L.msim_cent_encode_docs(dtc, dD.data_ptr(), doff.data_ptr(), len(lens), n_rows, 128, max_doc_rows, dC.data_ptr(), K,
                                   ref_codes.data_ptr(), ref_status.data_ptr(), st) == 0, L.msim_last_error()
    assert L.msim_res_encode_docs(dtc, dD.data_ptr(), n_rows, 128, ref_codes.data_ptr(), dC.data_ptr(), K, dcut.data_ptr(), bits,
                                  ref_res.data_ptr(), st) == 0, L.msim_last_error()

    # the fused entry, at an odd row of larger sentinel-filled arrays with guard rows on both sides
    row0, guard = 37, 64
    dst_rows = row0 + n_rows + guard
    codes = torch.full((2 * dst_rows,), SENTINEL, dtype=torch.uint8, device=DEV).view(torch.int16)
    res = torch.full((dst_rows, 16 * bits), SENTINEL, dtype=torch.uint8, device=DEV)
    status = torch.full((len(lens),), 7, dtype=torch.int32, device=DEV)

    def append(**kw):
        a = dict(dtype=dtc, D=dD.data_ptr(), n_rows=n_rows, dim=128, codes=codes.data_ptr(), row0=row0, dst_rows=dst_rows)
        a.update(kw)
        return L.msim_res_append(a["dtype"], a["D"], doff.data_ptr(), len(lens), a["n_rows"], a["dim"], max_doc_rows, dC.data_ptr(), K,
                                 dcut.data_ptr(), bits, a["codes"], res.data_ptr(), a["row0"], a["dst_rows"], status.data_ptr(), st)

    assert append(row0=guard + row0 + 1) == EINVAL and append(dst_rows=row0 + n_rows - 1) == EINVAL      # dst_row0 + n_rows > dst_rows
    assert append(codes=codes.data_ptr() + 2) == EINVAL and append(dim=320) == EINVAL and append(dim=64) == EINVAL
    assert append(dtype=amd._lib.dtype_code(torch.float32)) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (_u16(codes) == SENTINEL * 257).all() and (res.cpu().numpy() == SENTINEL).all()               # a refused call wrote nothing
    assert append() == 0, L.msim_last_error()
    torch.cuda.synchronize()

    want_status = np.zeros(len(lens), dtype=np.int32)
    want_status[bad_pages] = 1
    np.testing.assert_array_equal(ref_status.cpu().numpy(), want_status)
    np.testing.assert_array_equal(status.cpu().numpy(), want_status)
    good = np.ones(n_rows, dtype=bool)
    for p in bad_pages:
        good[off[p]:min(off[p + 1], n_rows)] = False
    want_codes = np.full(dst_rows, SENTINEL * 257, dtype=np.uint16)
    want_res = np.full((dst_rows, 16 * bits), SENTINEL, dtype=np.uint8)
    want_codes[row0:row0 + n_rows][good] = _u16(ref_codes)[good]
    want_res[row0:row0 + n_rows][good] = ref_res.cpu().numpy()[good]
    np.testing.assert_array_equal(_u16(codes), want_codes)               # the good rows, and the sentinel everywhere else
    np.testing.assert_array_equal(res.cpu().numpy(), want_res)
    # the two rules the inputs were built to exercise were exercised
    got = _u16(codes)[row0:row0 + n_rows]
    tie_rows = [int(r) for r in copies[:20] if good[int(r)]]
    assert tie_rows and (got[tie_rows] == 3).all() and not (got[good] == 5).any()
    zero_bucket = int((cut <= 0.0).sum())                                 # a residual of exactly 0.0 sits on a cutoff: the upper bucket
    field = res.cpu().numpy()[row0 + tie_rows[0]]
    assert all(((int(b) >> s) & ((1 << bits) - 1)) == zero_bucket for b in field for s in range(0, 8, bits))


# --------------------------------------------------------------------------------------------------------------- 2. compaction
C_LENS = [3, 51, 1, 1, 17, 5, 33, 7, 9, 1]                               # odd lengths: codes land on odd 2-byte positions
PATTERNS = {"first": [0, 1, 1, 1, 1, 1, 1, 1, 1, 1], "last": [1, 1, 1, 1, 1, 1, 1, 1, 1, 0], "two runs": [1, 0, 0, 1, 1, 0, 0, 0, 1, 1],
            "none": [1] * 10, "all": [0] * 10}


@pytest.mark.parametrize("bits", [2, 4])
@pytest.mark.parametrize("bounce_rows", [5, None], ids=["bounce of 5 rows", "bounce holds everything"])
def test_compaction_moves_both_arrays_against_one_plan(amd, bits, bounce_rows):
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(5 + bits)
    off = np.concatenate([[0], np.cumsum(C_LENS)]).astype(np.int32)
    bound, n = int(off[-1]), len(C_LENS)
    row_bytes = 16 * bits + 2
    bounce = torch.zeros(((bounce_rows or bound) * row_bytes,), dtype=torch.uint8, device=DEV)
    ws = torch.zeros(L.msim_res_live_compact_workspace_bytes(n, bounce.numel()), dtype=torch.uint8, device=DEV)
    used = torch.zeros(1, dtype=torch.int64, device=DEV)
    for name, alive in PATTERNS.items():
        codes = torch.randint(0, 2048, (bound + 6,), generator=g, dtype=torch.int32).to(torch.int16)
        res = torch.randint(0, 255, (bound + 6, 16 * bits), generator=g, dtype=torch.uint8)
        d_codes, d_res = codes.to(DEV).view(torch.uint16), res.to(DEV)
        d_off, d_alive = torch.from_numpy(off).to(DEV), torch.tensor(alive, dtype=torch.uint8, device=DEV)
        new_off = lt.compact_offsets(off, alive)
        want_codes = lt.compact_rows(codes.numpy().view(np.uint16), off, alive)
        want_res = lt.compact_rows(res.numpy(), off, alive)
        for _ in range(2):                                                # the second call changes nothing
            used.fill_(-1)
            rc = L.msim_res_live_compact(d_codes.data_ptr(), d_res.data_ptr(), bits, bound, d_off.data_ptr(), d_alive.data_ptr(), n,
                                         used.data_ptr(), ws.data_ptr(), bounce.data_ptr(), bounce.numel(), None)
            assert rc == 0, L.msim_last_error()
            torch.cuda.synchronize()
            assert int(ws[:4].view(torch.int32)[0]) == 0 and int(used[0]) == new_off[-1], name
            np.testing.assert_array_equal(d_off.cpu().numpy(), new_off, err_msg=name)
            t = int(new_off[-1])
            np.testing.assert_array_equal(_u16(d_codes)[:t], want_codes[:t], err_msg=name)
            np.testing.assert_array_equal(d_res.cpu().numpy()[:t], want_res[:t], err_msg=name)
            np.testing.assert_array_equal(_u16(d_codes)[bound:], codes.numpy().view(np.uint16)[bound:])     # nothing past the bound
            np.testing.assert_array_equal(d_res.cpu().numpy()[bound:], res.numpy()[bound:])
            first = min([m[1] for m in lt.move_list(off, alive)], default=bound)
            np.testing.assert_array_equal(_u16(d_codes)[:first], codes.numpy().view(np.uint16)[:first])     # nothing below the first move
    # offsets that are not monotonic: the status bit, no move, the old row count
    bad = torch.tensor([0, 5, 3, 9], dtype=torch.int32, device=DEV)
    keep = d_codes.view(torch.int16).clone(), d_res.clone()
    rc = L.msim_res_live_compact(d_codes.data_ptr(), d_res.data_ptr(), bits, 9, bad.data_ptr(), d_alive.data_ptr(), 3, used.data_ptr(),
                                 ws.data_ptr(), bounce.data_ptr(), bounce.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(ws[:4].view(torch.int32)[0]) == 1 and int(used[0]) == 9
    assert torch.equal(keep[0], d_codes.view(torch.int16)) and torch.equal(keep[1], d_res) and bad.tolist() == [0, 5, 3, 9]


# ------------------------------------------------------------------------------------------------------------------ 3. the class
def _same(got, want, surv, id_base):
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
    if len(got) == 3:                                                     # group_by: (scores, document ids, best pages)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
    np.testing.assert_array_equal(got[-1].cpu().numpy(), lt.expected_ids(want[-1].cpu().numpy(), surv, id_base))


def _check(amd, m, plain, codec, queries, cand, slot_mask, slot_labels, k=5):
    """`m.live` (score_fn=residual_scores, 100 ingest rows, a bounce buffer of 5 rows) and `plain` (all defaults) against the build
    over the packed survivors"""
    C, cut, w, bits = codec
    live = m.live
    F, surv = m.packed()
    for x in (live, plain):
        assert x.rows_used == m.table.rows_used and len(x) == len(m.pages)
        np.testing.assert_array_equal(x.view().offsets.cpu().numpy(), m.table.offsets())
        np.testing.assert_array_equal(x.alive[:len(x)].cpu().numpy(), np.asarray(m.table.alive, dtype=np.uint8))
        x.check()
    assert torch.equal(live.codes.view(torch.int16)[:live.rows_used], plain.codes.view(torch.int16)[:live.rows_used])
    assert torch.equal(live.residuals[:live.rows_used], plain.residuals[:live.rows_used])       # ingest rounds do not change a bit
    if F is None:
        got_s, got_i = live.search(queries[0], k)
        assert np.isneginf(got_s.cpu().numpy()).all() and (got_i.cpu().numpy() == -1).all()
        return
    R = amd.ResidualCorpus.build(F, index=amd.CentroidIndex.build(F, centroids=C), bits=bits, cutoffs=cut, weights=w)
    v = live.view()
    if live.rows_used == int(F.blob.shape[0]):                            # right after a compaction: the arrays are R's, byte for byte
        assert torch.equal(v.codes.view(torch.int16), R.codes.view(torch.int16)) and torch.equal(v.residuals, R.residuals)
    v_off, r_off = v.offsets.cpu().numpy(), R.offsets.cpu().numpy()
    v_codes, v_res, r_codes, r_res = _u16(v.codes), v.residuals.cpu().numpy(), _u16(R.codes), R.residuals.cpu().numpy()
    for p, s in enumerate(surv):                                          # the live slots hold R's pages
        assert v_off[s + 1] - v_off[s] == r_off[p + 1] - r_off[p]
        np.testing.assert_array_equal(v_codes[v_off[s]:v_off[s + 1]], r_codes[r_off[p]:r_off[p + 1]])
        np.testing.assert_array_equal(v_res[v_off[s]:v_off[s + 1]], r_res[r_off[p]:r_off[p + 1]])
    ref = amd.ShardedRetriever(R, score_fn=amd.residual_scores)
    base = live.id_base
    pos = {s + base: p for p, s in enumerate(surv)}
    n = len(live)
    flt = amd.PageFilter.from_mask(slot_mask[:n].to(DEV), base)
    ref_flt = amd.PageFilter.from_mask(slot_mask[surv].to(DEV), 0)
    grp = amd.PageGroups.from_labels(slot_labels[:n].to(DEV), base)
    ref_grp = amd.PageGroups.from_labels(slot_labels[surv].to(DEV), 0)
    for q in queries:
        c = cand[:len(q)]
        tc = torch.tensor([[pos.get(int(i), -1) for i in row] for row in c.tolist()], dtype=torch.int64, device=DEV)
        for x in (live, plain):
            _same(x.search(q, k, candidates=c), ref.search(q, k, candidates=tc), surv, base)
            _same(x.search(q, k, prefilter=x.index, n_candidates=7), ref.search(q, k, prefilter=R.index, n_candidates=7), surv, base)
        _same(live.search(q, k), ref.search(q, k), surv, base)
        for route in ("mask", "list"):
            _same(live.search(q, k, filter=flt, filter_route=route), ref.search(q, k, filter=ref_flt, filter_route=route), surv, base)
        _same(live.search(q, k, group_by=grp), ref.search(q, k, group_by=ref_grp), surv, base)
        _same(live.mine(q, c[:, :2].contiguous(), 6, max_ratio=0.95), ref.mine(q, tc[:, :2].contiguous(), 6, max_ratio=0.95), surv, base)   # deleted positives among them
        with pytest.raises(NotImplementedError, match="score_fn=residual_scores"):
            plain.mine(q, c[:, :2].contiguous(), 6)
        with pytest.raises(NotImplementedError, match="score_fn=residual_scores"):
            plain.search(q, k)


@pytest.mark.parametrize("dtype,bits", [(torch.bfloat16, 2), (torch.float16, 4)], ids=["bf16-2", "f16-4"])
def test_a_history_matches_the_build_over_the_packed_survivors(amd, dtype, bits):
    g = torch.Generator().manual_seed(2000 + bits)
    C, cut, w = (t.to(DEV) for t in _codec(g, bits, 256, dtype))
    codec = (C, cut, w, bits)
    live = amd.LiveResidualCorpus(C, cut, w, bits, 9000, 60, id_base=50, ingest_rows=100, bounce_bytes=5 * (16 * bits + 2),
                                  score_fn=amd.residual_scores)
    plain = amd.LiveResidualCorpus(C, cut, w, bits, 9000, 60, id_base=50)
    m = Model(amd, live, 128, dtype)
    queries = [amd.pack_queries([_rows(g, int(t), dtype) for t in torch.randint(1, 33, (n_q,), generator=g)], DEV) for n_q in (1, 4, 9)]
    cand = torch.randint(40, 120, (9, 10), generator=g).to(DEV)           # ids below, inside and above the shard
    cand[1, :] = -1
    cand[2, 0] = cand[2, 1] = 55                                          # a duplicate
    slot_mask = torch.rand(60, generator=g) > 0.4
    slot_labels = torch.randint(0, 6, (60,), generator=g) * 7 + 3

    def step(op, *a, **kw):
        getattr(m, op)(*a, **kw)
        x = a[0] if a else None
        if op == "add":
            assert plain.add(torch.stack(x).to(DEV) if kw.get("on_device") else x).tolist() == list(range(50 + len(m.pages) - len(x), 50 + len(m.pages)))
        elif op == "delete":
            plain.delete(torch.tensor(x, dtype=torch.int64, device=DEV) if kw.get("on_device") else [i for i in x])
        else:
            plain.compact()
        _check(amd, m, plain, codec, queries, cand, slot_mask, slot_labels)

    lens = [1, 300, 17, 64, 257] + [int(x) for x in torch.randint(1, 200, (20,), generator=g)]
    step("add", [_rows(g, n, dtype) for n in lens])                       # a host list: 100 rows a round, pages straddle rounds
    step("add", [_rows(g, 40, dtype) for _ in range(3)], on_device=True)  # a [n, rows, 128] device tensor
    step("delete", [50, 53, 54, 60, 77])                                  # the first page, an adjacent run, the last page
    step("compact")
    step("delete", [51, 70])
    # an add that does not fit raises and leaves bits, ids and rows_used as they were
    before = (live.rows_used, len(live), live.codes.view(torch.int16).clone(), live.residuals.clone(), live.offsets.clone())
    with pytest.raises(RuntimeError, match="capacity_rows"):
        live.add([_rows(g, 2000, dtype) for _ in range(5)])
    with pytest.raises(RuntimeError, match="capacity_docs"):
        live.add([_rows(g, 1, dtype) for _ in range(40)])
    assert (live.rows_used, len(live)) == before[:2] and torch.equal(before[2], live.codes.view(torch.int16))
    assert torch.equal(before[3], live.residuals) and torch.equal(before[4], live.offsets)
    step("add", [_rows(g, int(n), dtype) for n in torch.randint(1, 300, (12,), generator=g)])    # rows go behind the dead ones
    step("delete", [52, 79, 7, 10_000, 52], on_device=True)               # ids outside the shard and a repeat: ignored
    step("compact")
    keep = live.codes.view(torch.int16).clone(), live.residuals.clone(), live.offsets.clone()
    live.compact()                                                        # nothing to hand back: a no-op
    assert torch.equal(keep[0], live.codes.view(torch.int16)) and torch.equal(keep[1], live.residuals) and torch.equal(keep[2], live.offsets)
    step("delete", [s + 50 for s in m.table.survivors()])                 # delete everything ...
    step("compact")
    assert live.rows_used == 0
    step("add", [_rows(g, n, dtype) for n in (5, 130)])                   # ... then add again: new ids, rows from 0
    assert live.view().offsets[-3].item() == 0
    # from_residual starts from the frozen shard: the same bits, room to grow
    F, surv = m.packed()
    R = amd.ResidualCorpus.build(F, index=amd.CentroidIndex.build(F, centroids=C), bits=bits, cutoffs=cut, weights=w)
    grown = amd.LiveResidualCorpus.from_residual(R, 500, 4)
    assert grown.add([_rows(g, 9, dtype)]).tolist() == [2] and grown.rows_used == 144
    assert torch.equal(grown.view().codes.view(torch.int16)[:135], R.codes.view(torch.int16)[:135])


def test_captured_compact_and_search_replay_the_same_result(amd):
    """compact() and both candidate routes in one hipGraph: the second and third replay find nothing to move and give the same bits"""
    g = torch.Generator().manual_seed(8)
    dtype, bits = torch.bfloat16, 2
    C, cut, w = (t.to(DEV) for t in _codec(g, bits, 256, dtype))
    pages = [_rows(g, int(n), dtype) for n in torch.randint(1, 120, (60,), generator=g)]
    pq = amd.pack_queries([_rows(g, n, dtype) for n in (32, 9, 20)], DEV)
    cand = torch.randint(0, 64, (3, 12), generator=g).to(DEV)
    gone = [3, 4, 17, 40, 59]

    def fresh():
        live = amd.LiveResidualCorpus(C, cut, w, bits, 8000, 64, bounce_bytes=64 * 34)
        live.add(pages)
        live.delete(gone)
        return live

    def both(live):
        return live.search(pq, 10, candidates=cand) + live.search(pq, 10, prefilter=live.index, n_candidates=8)

    warm = fresh()                                                                       # loads every kernel outside the capture
    warm.compact()
    eager = [t.clone() for t in both(warm)]
    live = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live.compact()
        captured = both(live)
    for _ in range(3):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    live.check()
    assert torch.equal(live.view().codes.view(torch.int16), warm.view().codes.view(torch.int16))
    assert torch.equal(live.view().residuals, warm.view().residuals) and torch.equal(live.view().offsets, warm.view().offsets)
