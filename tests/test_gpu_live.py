"""The live corpus on the MI355X (colpali_amd.LiveCorpus, msim_live_compact, msim_live_mask_scores).

The contract, checked bit for bit after every step of a seeded history of add / delete / compact: with S the surviving pages in
slot order and F = pack_passages(S, batch_size=None), live.search returns the scores of ShardedRetriever(F).search and the ids of F
mapped back to slots (tests/live_truth.py: expected_ids) -- for the full scan, for candidates= and for prefilter=int8_index().
Nothing here has a tolerance.
"""
import numpy as np
import pytest
import torch

from tests import live_truth as lt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _rows(g, n, dim, dtype):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


class Model:
    """What the live corpus must be equal to: the pages by slot, and who survives."""

    def __init__(self, amd, live, dim, dtype):
        self.amd, self.live, self.dim, self.dtype = amd, live, dim, dtype
        self.pages, self.table = [], lt.SlotTable(live.id_base)

    def add(self, pages, on_device=False):
        got = self.live.add(torch.stack(pages).to(DEV) if on_device else pages)
        assert got.tolist() == self.table.add([len(p) for p in pages])
        self.pages += pages

    def delete(self, ids, on_device=False):
        self.live.delete(torch.tensor(ids, dtype=torch.int64, device=DEV) if on_device else ids)
        known = [i for i in dict.fromkeys(ids) if 0 <= i - self.live.id_base < len(self.pages)]     # the device form ignores the rest
        self.table.delete([i for i in known if self.table.alive[i - self.live.id_base]])

    def compact(self):
        self.live.compact()
        self.table.compact()

    def packed(self):
        surv = self.table.survivors()
        return (self.amd.pack_passages([self.pages[s] for s in surv], DEV, batch_size=None) if surv else None), surv

    def check(self, queries, k, candidates=None, n_candidates=None):
        amd, live = self.amd, self.live
        F, surv = self.packed()
        for q in queries:
            n_q = len(q)
            got_s, got_i = live.search(q, k)
            if F is None:
                assert np.isneginf(got_s.cpu().numpy()).all() and (got_i.cpu().numpy() == -1).all()
                continue
            ref = amd.ShardedRetriever(F)
            want_s, want_i = ref.search(q, k)
            np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
            np.testing.assert_array_equal(got_i.cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv, live.id_base))
            if candidates is not None:
                cand = candidates[:n_q]
                pos = {s + live.id_base: p for p, s in enumerate(surv)}
                tcand = torch.tensor([[pos.get(int(c), -1) for c in row] for row in cand.tolist()], dtype=torch.int64, device=DEV)
                got_s, got_i = live.search(q, k, candidates=cand)
                want_s, want_i = ref.search(q, k, candidates=tcand)
                np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
                np.testing.assert_array_equal(got_i.cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv, live.id_base))
            if n_candidates is not None:
                idx = live.int8_index()
                want_idx = amd.Int8Index.build(live.view())
                assert torch.equal(idx.codes[:live.rows_used], want_idx.codes[:live.rows_used])
                np.testing.assert_array_equal(_bits(idx.scales), _bits(want_idx.scales))
                got_s, got_i = live.search(q, k, prefilter=idx, n_candidates=n_candidates)
                want_s, want_i = ref.search(q, k, prefilter=amd.Int8Index.build(F), n_candidates=n_candidates)
                np.testing.assert_array_equal(_bits(got_s), _bits(want_s))
                np.testing.assert_array_equal(got_i.cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv, live.id_base))
        assert live.rows_used == self.table.rows_used and len(live) == len(self.pages)
        np.testing.assert_array_equal(live.view().offsets.cpu().numpy(), self.table.offsets())
        np.testing.assert_array_equal(live.alive[:len(live)].cpu().numpy(), np.asarray(self.table.alive, dtype=np.uint8))
        live.check()


@pytest.mark.parametrize("dtype,dim,bounce_rows", [(torch.bfloat16, 128, None), (torch.float16, 128, 7), (torch.bfloat16, 320, 5),
                                                  (torch.float32, 100, 3)])
def test_a_random_history_matches_the_packed_survivors_after_every_step(amd, dtype, dim, bounce_rows):
    g = torch.Generator().manual_seed(1000 + dim + (0 if dtype == torch.bfloat16 else 1))
    width = amd._lib.kernel_width(dim, dtype)
    row_bytes = width * (4 if dtype == torch.float32 else 2)
    tuned = dim == 128
    live = amd.LiveCorpus(9000, 400, DEV, dtype=dtype, width=dim, id_base=50,
                          bounce_bytes=None if bounce_rows is None else bounce_rows * row_bytes)
    m = Model(amd, live, dim, dtype)
    qs4 = [_rows(g, n, dim, dtype) for n in (32, 5, 17, 32)]                              # K1s
    qs40 = [_rows(g, int(n), dim, dtype) for n in torch.randint(1, 40, (40,), generator=g)]   # K1b
    queries = [amd.pack_queries(qs4, DEV), amd.pack_queries(qs40, DEV)] if dim in (128, 320) and dtype != torch.float32 else [qs4, qs40]
    cand = torch.randint(40, 200, (40, 12), generator=g).to(DEV) if tuned else None      # ids below, inside and above the corpus
    if tuned:
        cand[1, :] = -1
        cand[2, 0] = cand[2, 1] = 55                                                      # a duplicate

    def lens(n):
        return [int(x) for x in torch.randint(1, 90, (n,), generator=g)]

    m.add([_rows(g, n, dim, dtype) for n in [1, 40, 1, 2100 if tuned else 300] + lens(8)])   # 1-row pages, one page above 2048 rows
    m.check(queries, 10, cand, 6 if tuned else None)
    steps = 0
    while steps < 40:
        steps += 1
        op = int(torch.randint(0, 10, (1,), generator=g))
        alive_ids = [s + live.id_base for s in m.table.survivors()]
        if op < 3 and len(m.pages) < 380 and live.rows_used < 6000:
            if op == 0:
                per = int(torch.randint(1, 30, (1,), generator=g))
                m.add([_rows(g, per, dim, dtype) for _ in range(3)], on_device=True)      # a [n, rows, width] device tensor
            else:
                m.add([_rows(g, n, dim, dtype) for n in lens(int(torch.randint(1, 6, (1,), generator=g)))])
        elif op < 7 and alive_ids:
            pick = torch.randperm(len(alive_ids), generator=g)[:int(torch.randint(1, 5, (1,), generator=g))].tolist()
            ids = [alive_ids[p] for p in pick]
            if op == 6:
                m.delete(ids + [7, 10_000, ids[0]], on_device=True)                       # ids outside the corpus and a repeat: ignored
            else:
                m.delete(ids)
        else:
            m.compact()
            F, _ = m.packed()
            if F is not None:                                                             # the blob is the packed survivors, byte for byte
                assert torch.equal(live.view().blob.view(torch.uint8), F.blob.view(torch.uint8))
        m.check(queries, 10, cand, 6 if tuned else None)
    m.compact()
    before = live.view().blob.clone(), live.view().offsets.clone()
    live.compact()                                                                        # nothing to hand back: a no-op
    assert torch.equal(before[0], live.view().blob) and torch.equal(before[1], live.view().offsets)
    m.check(queries, 500, cand, 6 if tuned else None)                                     # k above the number of live pages
    if m.table.survivors():
        m.delete([s + live.id_base for s in m.table.survivors()])                         # delete everything ...
    m.check(queries, 10, cand, 6 if tuned else None)
    m.compact()
    assert live.rows_used == 0
    m.check(queries, 10, cand, 6 if tuned else None)
    m.add([_rows(g, n, dim, dtype) for n in lens(4)])                                     # ... then add again: new ids, rows from 0
    assert live.view().offsets[-5].item() == 0
    m.check(queries, 10, cand, 6 if tuned else None)


def test_small_chunks_a_page_across_chunks_and_raw_abi(amd):
    """The multi-chunk path directly: a bounce buffer of 4 rows under pages of up to 50 rows, for 256-byte and 128-byte rows."""
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(5)
    lens = [3, 50, 1, 1, 17, 4, 33, 2, 9, 1]
    alive = [1, 0, 1, 0, 0, 1, 1, 0, 1, 1]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    for row_bytes in (256, 128, 16, 640):
        rows = torch.randint(0, 255, (int(off[-1]) + 5, row_bytes), generator=g, dtype=torch.uint8)
        d_rows, d_off = rows.to(DEV), torch.from_numpy(off).to(DEV)
        d_alive = torch.tensor(alive, dtype=torch.uint8, device=DEV)
        used = torch.zeros(1, dtype=torch.int64, device=DEV)
        bounce = torch.zeros(4 * row_bytes, dtype=torch.uint8, device=DEV)
        ws = torch.zeros(L.msim_live_compact_workspace_bytes(len(lens), bounce.numel()), dtype=torch.uint8, device=DEV)
        for _ in range(2):                                                               # the second call changes nothing
            rc = L.msim_live_compact(d_rows.data_ptr(), row_bytes, int(off[-1]), d_off.data_ptr(), d_alive.data_ptr(), len(lens),
                                     used.data_ptr(), ws.data_ptr(), bounce.data_ptr(), bounce.numel(), None)
            assert rc == 0, L.msim_last_error()
            torch.cuda.synchronize()
            new_off = lt.compact_offsets(off, alive)
            assert int(ws[:4].view(torch.int32)[0]) == 0 and int(used[0]) == new_off[-1]
            np.testing.assert_array_equal(d_off.cpu().numpy(), new_off)
            want = lt.compact_rows(rows.numpy(), off, alive)
            np.testing.assert_array_equal(d_rows.cpu().numpy()[:new_off[-1]], want[:new_off[-1]])
            np.testing.assert_array_equal(d_rows.cpu().numpy()[int(off[-1]):], rows.numpy()[int(off[-1]):])   # nothing past the bound
    # offsets that are not monotonic: a status word, no move, the old row count
    bad = torch.tensor([0, 5, 3, 9], dtype=torch.int32, device=DEV)
    keep = d_rows.clone()
    rc = L.msim_live_compact(d_rows.data_ptr(), 640, 9, bad.data_ptr(), d_alive.data_ptr(), 3, used.data_ptr(), ws.data_ptr(),
                             bounce.data_ptr(), bounce.numel(), None)
    torch.cuda.synchronize()
    assert rc == 0 and int(ws[:4].view(torch.int32)[0]) == 1 and int(used[0]) == 9
    assert torch.equal(keep, d_rows) and bad.tolist() == [0, 5, 3, 9]


def test_mask_scores_writes_dead_columns_only(amd):
    g = torch.Generator().manual_seed(6)
    for n_q, n, pad in ((1, 1, 0), (3, 1027, 0), (70, 4100, 3), (5, 64, 4), (9, 2048, 0)):
        base = torch.randn(n_q, n + pad, generator=g).to(DEV)
        alive = (torch.rand(n, generator=g) > 0.4).to(torch.uint8)
        alive[: min(n, 8)] = 0                                                            # a whole 16-byte group of dead columns
        s = base.clone()[:, :n]
        amd.live.mask_scores(s, alive.to(DEV))
        np.testing.assert_array_equal(_bits(s), lt.mask(base[:, :n].cpu().numpy(), alive.numpy()).view(np.int32))


def test_captured_compact_and_search_replay_the_same_result(amd):
    g = torch.Generator().manual_seed(8)
    pages = [_rows(g, int(n), 128, torch.bfloat16) for n in torch.randint(1, 120, (60,), generator=g)]
    pq = amd.pack_queries([_rows(g, n, 128, torch.bfloat16) for n in (32, 9, 20)], DEV)
    gone = [3, 4, 17, 40, 59]

    def fresh():
        live = amd.LiveCorpus(8000, 64, DEV, bounce_bytes=64 * 256)
        live.add(pages)
        live.int8_index()
        live.delete(gone)
        return live

    warm = fresh()                                                                       # loads every kernel outside the capture
    warm.compact()
    eager = [t.clone() for t in warm.search(pq, 10) + warm.search(pq, 10, prefilter=warm.int8_index(), n_candidates=8)]
    live = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        live.compact()
        captured = live.search(pq, 10) + live.search(pq, 10, prefilter=live.int8_index(), n_candidates=8)
    for _ in range(3):                                                                   # the second and third compaction find nothing to move
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    live.check()
    surv = [s for s in range(60) if s not in gone]
    F = amd.pack_passages([pages[s] for s in surv], DEV, batch_size=None)
    assert torch.equal(live.view().blob, F.blob)
    want_s, want_i = amd.ShardedRetriever(F).search(pq, 10)
    np.testing.assert_array_equal(_bits(captured[0]), _bits(want_s))
    np.testing.assert_array_equal(captured[1].cpu().numpy(), lt.expected_ids(want_i.cpu().numpy(), surv))
