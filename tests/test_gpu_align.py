"""Token-to-patch alignment on the MI355X: msim_align_candidates (kernel K1a), colpali_amd.align, ShardedRetriever.align,
LiveCorpus.align and Alignment.similarity_maps.

Truth: helpers.maxsim_truth (float64 M, first-max A, gap G) and the float64 product S = Q D^T of the packed inputs.
Tolerance, derived: the kernel accumulates dim products in fp32 in one chain, so for any summation order
    |got - truth| <= dim * 2^-24 * sum_k |q_k d_k|                                   (the bound B_ij of one similarity)
with the sum taken in float64 from the inputs.  A reported maximum is the similarity of the reported row, so best_sim is held to the
same bound at that row, and to B_i = max_j B_ij against M.  best_row must equal A wherever G exceeds 2 B_i (two values that far apart
cannot swap under errors of B_i each); elsewhere any row whose truth similarity is within B_i of M is accepted.  No token is left
out.  What the kernel promises bit for bit (best_sim = the maximum of its row of sims, first column = best_row, the same bits for
the same (query, page) anywhere) is compared bit for bit.
"""
import functools

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NEG_INF = -float("inf")
PAGE_LENS = [0, 1, 15, 16, 17, 31, 33, 100, 257]
QUERY_LENS = [1, 15, 16, 17, 33, 128]
ID_BASE = 50
FORMATS = [(128, torch.bfloat16), (128, torch.float16), (320, torch.bfloat16), (320, torch.float16)]


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dim, dtype):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


class Case:
    """Packed inputs on the device plus their float64 truth, computed once."""

    def __init__(self, amd, qs, ps, flags, id_base=ID_BASE):
        self.qs, self.ps, self.id_base = qs, ps, id_base
        self.dim = int(qs[0].shape[1])
        self.flags = [bool(f) for f in flags] if flags is not None else [False] * len(ps)
        self.corpus = amd.pack_passages(ps, DEV, batch_size=None, id_base=id_base)
        if flags is not None:
            self.corpus.clamp0 = torch.tensor([int(f) for f in self.flags], dtype=torch.uint8, device=DEV)
        self.pq = amd.pack_queries(qs, DEV, layout="flat")
        self.q_lens = [int(q.shape[0]) for q in qs]
        self.p_lens = [int(p.shape[0]) for p in ps]
        self.q_off = np.concatenate([[0], np.cumsum(self.q_lens)])
        self.d_off = np.concatenate([[0], np.cumsum(self.p_lens)])
        Q = torch.cat(qs).double()
        D = torch.cat(ps).double() if sum(self.p_lens) else torch.zeros((0, self.dim), dtype=torch.float64)
        self.M, self.A, self.G = (t.numpy() for t in helpers.maxsim_truth(Q, D, self.d_off))
        self.S = (Q @ D.T).numpy()                                         # [tokens, rows]
        self.B = self.dim * 2.0**-24 * (Q.abs() @ D.abs().T).numpy()       # the bound of every similarity
        self.T = max(self.q_lens)
        self.R = max(self.p_lens)


def verify(case, al, ids, R=None, maps=True):
    """Every entry and every token slot of an Alignment against the truth of `case`; `ids` the host list the call was given."""
    R = case.R if R is None else R
    bs, br = al.best_sim.cpu().numpy(), al.best_row.cpu().numpy()
    sims = al.sims.cpu().numpy() if maps else None
    n_q, m = ids.shape
    assert bs.shape == (n_q, m, case.T) and br.shape == bs.shape and bs.dtype == np.float32 and br.dtype == np.int32
    if maps:
        assert sims.shape == (n_q, m, case.T, R)
    out_ids = al.ids.cpu().numpy()
    checked = 0
    for q in range(n_q):
        a, b = case.q_off[q], case.q_off[q + 1]
        L = b - a
        for j in range(m):
            where = f"entry ({q}, {j}) id {int(ids[q, j])}"
            c = int(ids[q, j]) - case.id_base
            has_page = int(ids[q, j]) >= 0 and 0 <= c < len(case.ps)
            assert out_ids[q, j] == (int(ids[q, j]) if has_page else -1), where
            gs, gr = bs[q, j], br[q, j]
            assert (gs[L:] == 0.0).all() and (gr[L:] == -1).all(), where + ": padding token slots are (0, -1)"
            if maps:
                assert (sims[q, j, L:] == NEG_INF).all(), where + ": padding token slots of the map are -inf"
            n = case.p_lens[c] if has_page else 0
            flagged = has_page and case.flags[c]
            if maps:
                assert (sims[q, j, :, n:] == NEG_INF).all(), where + ": columns past the page's end are -inf"
            if n == 0:
                assert (gr[:L] == -1).all(), where
                assert (gs[:L] == (0.0 if flagged else NEG_INF)).all(), where
                checked += L
                continue
            r0 = case.d_off[c]
            S, B = case.S[a:b, r0:r0 + n], case.B[a:b, r0:r0 + n]
            M, A, G = case.M[a:b, c], case.A[a:b, c], case.G[a:b, c]
            Bi = B.max(axis=1)
            if maps:
                got = sims[q, j, :L, :n].astype(np.float64)
                assert (np.abs(got - S) <= B).all(), where + f": map error {np.abs(got - S).max():.3e}"
                rowmax = sims[q, j, :L, :n].max(axis=1)
                first = (sims[q, j, :L, :n] == rowmax[:, None]).argmax(axis=1)
            for i in range(L):
                tok = where + f" token {i}"
                v, r = float(gs[i]), int(gr[i])
                if r == -1:                                               # the zero padding row won: only under the flag, only
                    assert flagged and v == 0.0 and M[i] <= Bi[i], tok    # where the truth maximum is not clearly positive
                    if maps:
                        assert not rowmax[i] >= 0.0, tok
                else:
                    assert 0 <= r < n, tok
                    assert not (flagged and M[i] < -Bi[i]), tok + ": a clearly negative maximum under the flag must report (0, -1)"
                    assert abs(v - S[i, r]) <= B[i, r], tok + f": best_sim is not the similarity of row {r}"
                    assert abs(v - M[i]) <= Bi[i], tok + f": best_sim {v} vs {M[i]}"
                    if G[i] > 2 * Bi[i]:
                        assert r == A[i], tok + f": row {r}, truth {A[i]} (gap {G[i]:.3e})"
                    else:
                        assert M[i] - S[i, r] <= Bi[i], tok + f": row {r} is not within the bound of the maximum"
                    if maps:                                              # bit for bit: the maximum of its row, its first column
                        assert np.float32(v).view(np.int32) == rowmax[i].view(np.int32) and r == first[i], tok
                checked += 1
    assert checked == sum(case.q_off[q + 1] - case.q_off[q] for q in range(n_q)) * m       # no token was left out


def _id_lists(n_pages, n_q, seed):
    """[n_q, 7]: four listed pages (every page of the corpus is listed by some query), -1, an id outside the range (below: 49 and 3,
    above: the first id past the corpus and 10^12) and, in column 5, column 0 again."""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_pages, generator=g).tolist()
    outside = [ID_BASE - 1, ID_BASE + n_pages, 3, 10**12]
    rows = []
    for q in range(n_q):
        p = [ID_BASE + perm[(4 * q + t) % n_pages] for t in range(4)]
        rows.append([p[0], p[1], -1, outside[q % 4], p[2], p[0], p[3]])
    assert {c - ID_BASE for r in rows for c in (r[0], r[1], r[4], r[6])} == set(range(n_pages)) or n_q * 4 < n_pages
    return torch.tensor(rows, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _ragged(amd, dim, dtype):
    g = torch.Generator().manual_seed(dim + (7 if dtype == torch.float16 else 0))
    lens = PAGE_LENS * 2
    lens = [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]
    flags = torch.zeros(len(lens), dtype=torch.bool)
    flags[torch.randperm(len(lens), generator=g)[: len(lens) // 2]] = True           # a random half
    ps = [_unit(g, n, dim, dtype) for n in lens]
    qs = [_unit(g, n, dim, dtype) for n in QUERY_LENS]
    case = Case(amd, qs, ps, flags.tolist())
    ids = _id_lists(len(ps), len(qs), seed=dim)
    return case, ids


@pytest.mark.parametrize("dim,dtype", FORMATS)
def test_every_entry_against_the_float64_truth(amd, dim, dtype):
    case, ids = _ragged(amd, dim, dtype)
    assert set(case.p_lens) == set(PAGE_LENS) and case.q_lens == QUERY_LENS
    al = amd.align(case.pq, case.corpus, ids.to(DEV), maps=True)
    verify(case, al, ids)
    # the same entries without the map, under m = 1, in a permuted list, at a repeated position: the same bits
    lean = amd.align(case.pq, case.corpus, ids.to(DEV))
    assert lean.sims is None
    np.testing.assert_array_equal(_bits(lean.best_sim), _bits(al.best_sim))
    np.testing.assert_array_equal(lean.best_row.cpu().numpy(), al.best_row.cpu().numpy())
    np.testing.assert_array_equal(_bits(al.best_sim[:, 5]), _bits(al.best_sim[:, 0]))
    np.testing.assert_array_equal(_bits(al.sims[:, 5]), _bits(al.sims[:, 0]))
    np.testing.assert_array_equal(al.best_row[:, 5].cpu().numpy(), al.best_row[:, 0].cpu().numpy())
    one = amd.align(case.pq, case.corpus, ids[:, :1].to(DEV), maps=True)
    verify(case, one, ids[:, :1])
    np.testing.assert_array_equal(_bits(one.best_sim), _bits(al.best_sim[:, :1]))
    np.testing.assert_array_equal(_bits(one.sims), _bits(al.sims[:, :1]))
    perm = torch.randperm(7, generator=torch.Generator().manual_seed(1))
    shuffled = amd.align(case.pq, case.corpus, ids[:, perm].to(DEV), maps=True)
    np.testing.assert_array_equal(_bits(shuffled.best_sim), _bits(al.best_sim[:, perm.to(DEV)]))
    np.testing.assert_array_equal(_bits(shuffled.sims), _bits(al.sims[:, perm.to(DEV)]))
    np.testing.assert_array_equal(shuffled.best_row.cpu().numpy(), al.best_row[:, perm.to(DEV)].cpu().numpy())
    # the same queries in another batch (other positions, another longest query: another T)
    sub = [4, 1, 3]
    pq2 = amd.pack_queries([case.qs[i] for i in sub], DEV, layout="flat")
    other = amd.align(pq2, case.corpus, ids[sub].to(DEV), maps=True)
    T2 = max(case.q_lens[i] for i in sub)
    assert other.best_sim.shape[2] == T2
    np.testing.assert_array_equal(_bits(other.best_sim), _bits(al.best_sim[sub][:, :, :T2]))
    np.testing.assert_array_equal(_bits(other.sims), _bits(al.sims[sub][:, :, :T2]))
    # host lists and a dense device box are packed as rerank packs them
    box = torch.zeros((2, 40, dim), dtype=dtype)
    box[0, :33], box[1, :17] = case.qs[4], case.qs[3]
    dense = amd.align(box.to(DEV), case.corpus, ids[[4, 3]].to(DEV))
    np.testing.assert_array_equal(_bits(dense.best_sim[0, :, :33]), _bits(al.best_sim[4, :, :33]))
    np.testing.assert_array_equal(_bits(dense.best_sim[1, :, :17]), _bits(al.best_sim[3, :, :17]))


@pytest.mark.parametrize("dim,dtype", [(128, torch.bfloat16), (320, torch.float16)])
def test_token_sums_agree_with_rerank(amd, dim, dtype):
    """sum_i best_sim[q, j, i] in float64 vs rerank: every token is within its bound B_i, rerank within its documented
    1e-5 * max(|score|, 1) of the truth."""
    case, ids = _ragged(amd, dim, dtype)
    al = amd.align(case.pq, case.corpus, ids.to(DEV))
    scores = amd.rerank(case.pq, case.corpus, ids.to(DEV)).cpu().numpy().astype(np.float64)
    bs = al.best_sim.cpu().numpy().astype(np.float64)
    for q in range(ids.shape[0]):
        a, b = case.q_off[q], case.q_off[q + 1]
        for j in range(ids.shape[1]):
            total = bs[q, j, :b - a].sum()
            c = int(ids[q, j]) - case.id_base
            if not (int(ids[q, j]) >= 0 and 0 <= c < len(case.ps)) or (case.p_lens[c] == 0 and not case.flags[c]):
                assert total == NEG_INF and scores[q, j] == NEG_INF
                continue
            r0, n = case.d_off[c], case.p_lens[c]
            margin = (case.B[a:b, r0:r0 + n].max(axis=1).sum() if n else 0.0) + 1e-5 * max(abs(scores[q, j]), 1.0)
            assert abs(total - scores[q, j]) <= margin, (q, j, total, scores[q, j], margin)


@pytest.mark.parametrize("dim,dtype", [(128, torch.bfloat16), (320, torch.bfloat16), (128, torch.float16)])
def test_exact_ties_report_the_lower_row(amd, dim, dtype):
    g = torch.Generator().manual_seed(5)
    u = _unit(g, 1, dim, torch.float32)[0]
    qs = [torch.nn.functional.normalize(u + 0.05 * torch.randn(n, dim, generator=g), dim=-1).to(dtype) for n in (17, 33, 5)]
    twin = u.to(dtype)
    ps, want = [], []
    for n, (lo, hi) in ((33, (0, 5)), (40, (15, 16)), (257, (3, 256)), (20, (3, 19))):
        p = _unit(g, n, dim, dtype)
        p[lo] = twin
        p[hi] = twin                                                       # the same row bit for bit
        ps.append(p)
        want.append(lo)
    case = Case(amd, qs, ps, None)
    ids = torch.tensor([[ID_BASE + c for c in range(4)]] * 3, dtype=torch.int64)
    al = amd.align(case.pq, case.corpus, ids.to(DEV), maps=True)
    verify(case, al, ids)
    sims, br = al.sims.cpu(), al.best_row.cpu()
    for c, (lo, hi) in enumerate(((0, 5), (15, 16), (3, 256), (3, 19))):
        for q, L in enumerate(case.q_lens):
            assert (case.A[case.q_off[q]:case.q_off[q + 1], c] == lo).all()       # the twin rows are the maximum of every token
            assert torch.equal(sims[q, c, :L, lo].view(torch.int32), sims[q, c, :L, hi].view(torch.int32))
            assert (br[q, c, :L] == want[c]).all(), (c, q)


@pytest.mark.parametrize("dim", [128, 320])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sign_tier_all_negative_pages(amd, dim, dtype):
    """Every similarity is negative: a zero that leaks into a maximum (a row past the page's end that was not masked, a clamp on
    the wrong page) moves a result by at least the margin asserted on the truth."""
    g = torch.Generator().manual_seed(dim)
    d_lens = helpers.far_side_doc_lens(g, copies=1, n_empty=2, max_len=257)
    q_lens = [1, 17, 40]
    for planted in (False, True):
        qs, ps, rows = helpers.far_side_case(3 + planted, q_lens, d_lens, dim, dtype, planted=planted)
        ids = torch.arange(ID_BASE, ID_BASE + len(ps), dtype=torch.int64).repeat(len(qs), 1)
        for flagged in (False, True):
            case = Case(amd, qs, ps, [flagged] * len(ps))
            nonempty = np.array(case.p_lens) > 0
            if not planted:                                               # the tier's precondition, asserted on the truth
                assert (case.M[:, nonempty] <= -helpers.SIGN_MARGIN).all()
            else:
                assert (case.M[:, nonempty] >= helpers.SIGN_MARGIN).all() and (case.G[:, nonempty] >= helpers.SIGN_MARGIN).all()
            al = amd.align(case.pq, case.corpus, ids.to(DEV), maps=True)
            verify(case, al, ids)
            bs, br = al.best_sim.cpu().numpy(), al.best_row.cpu().numpy()
            for q, L in enumerate(q_lens):
                for c, n in enumerate(case.p_lens):
                    if planted and n:
                        assert (br[q, c, :L] == rows[c]).all(), (q, c)
                        assert (bs[q, c, :L] >= helpers.SIGN_MARGIN / 2).all()
                    elif flagged:
                        assert (bs[q, c, :L] == 0.0).all() and (br[q, c, :L] == -1).all(), (q, c)
                    elif n:
                        assert (bs[q, c, :L] <= -helpers.SIGN_MARGIN / 2).all() and (br[q, c, :L] >= 0).all(), (q, c)
                    else:
                        assert (bs[q, c, :L] == NEG_INF).all() and (br[q, c, :L] == -1).all(), (q, c)


def test_sign_edge_lengths_are_covered():
    lens = helpers.far_side_doc_lens(torch.Generator().manual_seed(0), copies=1, n_empty=2, max_len=257)
    assert sorted(lens) == [0, 0] + [n for n in helpers.SIGN_EDGE_LENS if n <= 257]


def test_live_corpus_align(amd):
    dim, dtype = 128, torch.bfloat16
    g = torch.Generator().manual_seed(21)
    pages = [_unit(g, n, dim, dtype) for n in (5, 33, 100, 16, 1, 64, 17)]
    live = amd.LiveCorpus(2000, 40, DEV, dtype=dtype, width=dim, id_base=ID_BASE)
    live.add(pages)
    qs = [_unit(g, n, dim, dtype) for n in (7, 33)]
    pq = amd.pack_queries(qs, DEV, layout="flat")
    ids = torch.tensor([[50, 51, 52, 53, 54, 55, 56, -1, 57], [56, 55, 54, 53, 52, 51, 50, 49, 51]], dtype=torch.int64, device=DEV)
    before = amd.align(pq, live.view(), ids, maps=True)
    live.delete([51, 54])
    dead = (ids == 51) | (ids == 54)
    for compacted in (False, True):
        if compacted:
            live.compact()
            live.add([_unit(g, 9, dim, dtype)])                          # id 57 now exists
        got = live.align(pq, ids, maps=True)
        want = amd.align(pq, live.view(), ids, maps=True)
        for q, L in enumerate((7, 33)):
            assert bool((got.best_sim[q, dead[q], :L] == NEG_INF).all()) and bool((got.best_row[q, dead[q]] == -1).all())
            assert bool((got.sims[q, dead[q]] == NEG_INF).all()) and bool((got.ids[q, dead[q]] == -1).all())
        keep = ~dead
        R = min(got.sims.shape[3], before.sims.shape[3])
        np.testing.assert_array_equal(_bits(got.best_sim[keep]), _bits(want.best_sim[keep]))          # a survivor: the bits of align
        np.testing.assert_array_equal(_bits(got.sims[keep]), _bits(want.sims[keep]))                  # on the view
        np.testing.assert_array_equal(got.best_row[keep].cpu().numpy(), want.best_row[keep].cpu().numpy())
        old = keep & (ids != 57)
        np.testing.assert_array_equal(_bits(got.best_sim[old]), _bits(before.best_sim[old]))          # ... and of before the deletes
        np.testing.assert_array_equal(_bits(got.sims[old][..., :R]), _bits(before.sims[old][..., :R]))
    assert bool((got.best_row[0, 8, :7] >= 0).all())                     # the page added after the compaction is found


@pytest.mark.parametrize("dim,dtype", [(128, torch.bfloat16), (320, torch.float16)])
def test_two_shards_combined_by_max_equal_one(amd, dim, dtype):
    case, ids = _ragged(amd, dim, dtype)
    one = amd.ShardedRetriever(case.corpus).align(case.pq, ids.to(DEV))
    direct = amd.align(case.pq, case.corpus, ids.to(DEV))
    np.testing.assert_array_equal(_bits(one.best_sim), _bits(direct.best_sim))
    cut = 7
    parts = []
    for lo, hi in ((0, cut), (cut, len(case.ps))):
        shard = amd.pack_passages(case.ps[lo:hi], DEV, batch_size=None, id_base=ID_BASE + lo)
        shard.clamp0 = case.corpus.clamp0[lo:hi].contiguous()
        parts.append(amd.ShardedRetriever(shard).align(case.pq, ids.to(DEV)))
    np.testing.assert_array_equal(_bits(torch.maximum(parts[0].best_sim, parts[1].best_sim)), _bits(one.best_sim))
    np.testing.assert_array_equal(torch.maximum(parts[0].best_row, parts[1].best_row).cpu().numpy(), one.best_row.cpu().numpy())
    np.testing.assert_array_equal(torch.maximum(parts[0].ids, parts[1].ids).cpu().numpy(), one.ids.cpu().numpy())
    with pytest.raises(ValueError):
        amd.ShardedRetriever(case.corpus, world=2, rank=0, dist=object()).align(case.pq, ids.to(DEV), maps=True)


def test_the_c_abi_directly(amd):
    """sims = NULL, a list row stride > m, max_rows smaller than one listed page: that entry is NaN / -1, its neighbours and the
    memory behind the outputs are untouched."""
    from colpali_amd import _lib

    case, ids = _ragged(amd, 128, torch.bfloat16)
    L = _lib.lib()
    n_q, m, ld, T = len(case.qs), 7, 9, case.T
    R = 100                                                              # the 257-row pages do not fit
    dids = torch.cat([ids, torch.full((n_q, ld - m), ID_BASE + 1, dtype=torch.int64)], dim=1).to(DEV)    # row stride 9 > m
    bs = torch.full((n_q * m * T + 64,), 7.0, dtype=torch.float32, device=DEV)
    br = torch.full((n_q * m * T + 64,), 7, dtype=torch.int32, device=DEV)

    def call(dtype=0, dim=128, t=T, sims=None):
        return L.msim_align_candidates(dtype, _lib.ptr(case.pq.tokens), _lib.ptr(case.pq.offsets), n_q, case.pq.tokens.shape[0], t,
                                       _lib.ptr(case.corpus.blob), _lib.ptr(case.corpus.offsets), _lib.ptr(case.corpus.clamp0),
                                       len(case.corpus), case.corpus.blob.shape[0], dim, _lib.ptr(dids), m, ld, ID_BASE, _lib.ptr(bs),
                                       _lib.ptr(br), _lib.ptr(sims), R, _lib.current_stream_handle(DEV))

    assert call() == 0, L.msim_last_error()
    torch.cuda.synchronize()
    want = amd.align(case.pq, case.corpus, dids[:, :m].contiguous())
    got_s, got_r = bs[:n_q * m * T].view(n_q, m, T), br[:n_q * m * T].view(n_q, m, T)
    too_long = torch.tensor([[int(c) - ID_BASE in range(len(case.ps)) and case.p_lens[int(c) - ID_BASE] > R for c in row[:m]]
                             for row in ids.tolist()])
    assert bool(too_long.any()) and not bool(too_long.all())
    assert bool(torch.isnan(got_s[too_long.to(DEV)]).all()) and bool((got_r[too_long.to(DEV)] == -1).all())
    ok = (~too_long).to(DEV)
    np.testing.assert_array_equal(_bits(got_s[ok]), _bits(want.best_sim[ok]))
    np.testing.assert_array_equal(got_r[ok].cpu().numpy(), want.best_row[ok].cpu().numpy())
    assert bool((bs[n_q * m * T:] == 7.0).all()) and bool((br[n_q * m * T:] == 7).all())
    # the same bound with maps through the binding: the long page's map is NaN in full, max_rows that is no multiple of 4
    short = amd.align(case.pq, case.corpus, dids[:, :m].contiguous(), maps=True, max_rows=R + 1)
    assert bool(torch.isnan(short.sims[too_long.to(DEV)]).all()) and bool(torch.isnan(short.best_sim[too_long.to(DEV)]).all())
    np.testing.assert_array_equal(_bits(short.best_sim[ok]), _bits(want.best_sim[ok]))
    full = amd.align(case.pq, case.corpus, dids[:, :m].contiguous(), maps=True)
    np.testing.assert_array_equal(_bits(short.sims[ok][..., :R + 1]), _bits(full.sims[ok][..., :R + 1]))
    # refused formats
    assert call(dtype=2) == -2 and call(dim=96) == -2 and call(t=129) == -2
    assert L.msim_align_candidates(0, None, None, 0, 0, 4, None, None, None, 0, 0, 128, None, 3, 3, 0, None, None, None, 4, None) == 0


def test_similarity_maps_match_the_dense_entry(amd):
    """Alignment.similarity_maps vs get_similarity_maps_from_embeddings on the same page.  The dense entry returns its map rounded to
    the embeddings' dtype: both fp32 values are within B of the truth, so they differ by at most 2 B plus half a bf16 ulp of the
    dense value (8 significand bits: at most 2^-8 relative)."""
    dim, dtype = 128, torch.bfloat16
    g = torch.Generator().manual_seed(31)
    nx, ny = 6, 9
    lead = 3                                                             # rows in front of the image patches (text tokens)
    ps = [_unit(g, 40, dim, dtype), _unit(g, lead + nx * ny + 2, dim, dtype), _unit(g, nx * ny, dim, dtype)]
    qs = [_unit(g, 13, dim, dtype), _unit(g, 20, dim, dtype)]
    case = Case(amd, qs, ps, None)
    ids = torch.tensor([[52, 51], [51, 52]], dtype=torch.int64)
    al = amd.align(case.pq, case.corpus, ids.to(DEV), maps=True)
    verify(case, al, ids)
    for q, j, c, rows in ((0, 0, 2, None), (0, 1, 1, slice(lead, lead + nx * ny)), (1, 0, 1, slice(lead, lead + nx * ny))):
        got = al.similarity_maps(q, j, (nx, ny), rows=rows)
        assert got.shape == (case.q_lens[q], nx, ny) and got.dtype == torch.float32
        mask = torch.zeros((1, case.p_lens[c]), dtype=torch.bool)
        mask[0, rows if rows is not None else slice(None)] = True
        ref = amd.get_similarity_maps_from_embeddings(ps[c].unsqueeze(0).to(DEV), qs[q].unsqueeze(0).to(DEV), (nx, ny), mask.to(DEV))[0]
        assert ref.shape == got.shape
        ref = ref.float().cpu().numpy().astype(np.float64)
        a, r0 = case.q_off[q], case.d_off[c] + (lead if rows is not None else 0)
        B = case.B[a:a + case.q_lens[q], r0:r0 + nx * ny].reshape(-1, ny, nx).transpose(0, 2, 1)
        S = case.S[a:a + case.q_lens[q], r0:r0 + nx * ny].reshape(-1, ny, nx).transpose(0, 2, 1)
        mine = got.cpu().numpy().astype(np.float64)
        assert (np.abs(mine - S) <= B).all()                             # the axis order, against the truth
        assert (np.abs(mine - ref) <= 2 * B + np.abs(ref) * 2.0**-8).all()
    with pytest.raises(ValueError, match="does not match the number of non-padded image tokens"):
        al.similarity_maps(0, 1, (nx, ny))


def test_broken_device_offsets_give_nan_and_no_fault(amd):
    dim, dtype = 320, torch.bfloat16
    g = torch.Generator().manual_seed(41)
    corpus = amd.pack_passages([_unit(g, int(n), dim, dtype) for n in torch.randint(1, 200, (30,), generator=g)], DEV, batch_size=None)
    pq = amd.pack_queries([_unit(g, 20, dim, dtype) for _ in range(3)], DEV, layout="flat")
    ids = torch.randint(0, 30, (3, 9), generator=g)
    ids[0, 0], ids[1, 1] = 4, 9
    ids = ids.to(DEV)
    good = amd.align(pq, corpus, ids, maps=True)
    # query 2 claims tokens 40 .. 299 of a 60-token matrix
    bad = amd.PackedQueries(tokens=pq.tokens, offsets=torch.tensor([0, 20, 40, 300], dtype=torch.int32, device=DEV),
                            offsets_host=pq.offsets_host)
    al = amd.align(bad, corpus, ids, maps=True)
    assert bool(torch.isnan(al.best_sim[2]).all()) and bool((al.best_row[2] == -1).all()) and bool(torch.isnan(al.sims[2]).all())
    np.testing.assert_array_equal(_bits(al.best_sim[:2]), _bits(good.best_sim[:2]))
    np.testing.assert_array_equal(_bits(al.sims[:2]), _bits(good.sims[:2]))
    # offsets that run backwards, and a query longer than the bound the call was given
    for off in ([0, 20, 10, 60], [0, 45, 50, 60]):
        al = amd.align(amd.PackedQueries(tokens=pq.tokens, offsets=torch.tensor(off, dtype=torch.int32, device=DEV),
                                         offsets_host=pq.offsets_host), corpus, ids)
        assert bool(torch.isnan(al.best_sim).any()) and bool((al.best_row[torch.isnan(al.best_sim)] == -1).all())
    # page offsets: page 4 ends past the blob, page 9 runs backwards; every entry that lists them is NaN, the others are untouched
    off = corpus.offsets.clone()
    off[5] = corpus.blob.shape[0] + 1000
    off[10] = off[9] - 1
    broken = amd.PackedCorpus(blob=corpus.blob, offsets=off, clamp0=None, lengths=corpus.lengths)
    al = amd.align(pq, broken, ids, maps=True)
    hit = (ids == 4) | (ids == 5) | (ids == 9) | (ids == 10)             # the neighbours' starts or ends moved too
    assert bool(torch.isnan(al.best_sim[(ids == 4) | (ids == 9)]).all())
    np.testing.assert_array_equal(_bits(al.best_sim[~hit]), _bits(good.best_sim[~hit]))
    np.testing.assert_array_equal(_bits(al.sims[~hit]), _bits(good.sims[~hit]))


def test_captured_call_equals_eager(amd):
    case, ids = _ragged(amd, 320, torch.bfloat16)
    dids = ids.to(DEV)

    def fn():
        al = amd.align(case.pq, case.corpus, dids, maps=True)
        return al.best_sim, al.best_row, al.sims

    eager = [t.clone() for t in fn()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up on a side stream, as torch.cuda.graph expects
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = fn()
    for _ in range(2):
        for t in captured:
            t.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(captured, eager):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.int32), want.cpu().numpy().view(np.int32))


def test_error_paths(amd):
    dim = 128
    g = torch.Generator().manual_seed(9)
    corpus = amd.pack_passages([_unit(g, 5, dim, torch.bfloat16) for _ in range(10)], DEV, batch_size=None)
    ids = torch.randint(0, 10, (2, 4), generator=g).to(DEV)
    with pytest.raises(RuntimeError):                                  # dtype mismatch
        amd.align([_unit(g, 8, dim, torch.float16)] * 2, corpus, ids)
    with pytest.raises(NotImplementedError):                           # fp32
        c32 = amd.pack_passages([torch.randn(5, dim)] * 10, DEV, batch_size=None)
        amd.align([torch.randn(8, dim)] * 2, c32, ids)
    with pytest.raises(NotImplementedError):                           # neither 128 nor 320
        cw = amd.pack_passages([_unit(g, 5, 96, torch.bfloat16)] * 10, DEV, batch_size=None)
        amd.align([_unit(g, 8, 96, torch.bfloat16)] * 2, cw, ids)
    with pytest.raises(NotImplementedError):                           # width-320 queries against a width-128 corpus
        amd.align([_unit(g, 8, 320, torch.bfloat16)] * 2, corpus, ids)
    with pytest.raises(NotImplementedError):                           # a query over 128 tokens
        amd.align([_unit(g, 129, dim, torch.bfloat16), _unit(g, 4, dim, torch.bfloat16)], corpus, ids)
    for wrong in (ids.cpu(), ids.to(torch.int32), ids[0], ids[:1]):    # device, dtype, rank, number of rows
        with pytest.raises(ValueError):
            amd.align([_unit(g, 8, dim, torch.bfloat16)] * 2, corpus, wrong)
    with pytest.raises(ValueError):
        amd.align([_unit(g, 8, dim, torch.bfloat16)] * 2, corpus, ids, max_rows=-1)
    empty = amd.align([_unit(g, 8, dim, torch.bfloat16)] * 2, corpus, ids[:, :0])
    assert empty.best_sim.shape == (2, 0, 8) and empty.sims is None
