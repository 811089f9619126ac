"""Filtered search on the MI355X (colpali_amd.PageFilter, msim_filter_pack / _mask / _list / _ids, `search(filter=)`).

Every comparison is exact (bits, ids): the scores are those of the unchanged scan and rerank kernels, fetched to the host and fed
to the numpy restatement in tests/filter_truth.py; the filter kernels only move bits and ids.  The one tolerance is the width-320
corner include/maxsim.h states for msim_fwd_candidates_wide.  The shapes are the edges of the kernels: rows around the 32-bit word,
the 64-column ballot and the 4-column lane group, matrices whose rows are not 16-byte aligned, rows around the list kernel's pass
span S, words whose bits at positions >= n are dirty.
"""
import numpy as np
import pytest
import torch

from tests import filter_truth as ft

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.0
S = 8192                  # the list kernel's pass span (include/maxsim.h)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _filter(amd, spec, id_base=0, dirty=False):
    """the PageFilter of a tests/filter_truth.py SPEC; dirty: the bits at positions >= n of every last word are set afterwards"""
    if spec[0] == "labels":
        return amd.PageFilter.from_labels(torch.from_numpy(np.asarray(spec[1], dtype=np.int32)).to(DEV),
                                          torch.from_numpy(np.asarray(spec[2], dtype=np.int32)).to(DEV), id_base)
    flt = amd.PageFilter.from_mask(torch.from_numpy(np.asarray(spec[1]).astype(bool)).to(DEV), id_base)
    n = len(flt)
    if dirty and n % 32:
        high = np.array([(0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)
        flt.words[:, -1] |= torch.from_numpy(high).to(DEV)
    return flt


def _specs(r, n_q, n, density=0.3):
    shared = r.random(n) < density
    per = r.random((n_q, n)) < density
    if n_q > 1:
        per[1] = False                                                   # a query with no allowed page
    labels = (r.integers(0, 4, n).astype(np.int32), r.integers(0, 4, n_q).astype(np.int32))
    labels[1][0] = 99                                                    # a label no page carries
    return [("shared", shared), ("per_query", per), ("labels", *labels)]


# ----------------------------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 2049])
def test_pack_equals_numpy(amd, n):
    r = np.random.default_rng(n)
    for rows in (1, 5):
        m = (r.random((rows, n)) < 0.5)
        m[0, n - 1] = True
        want = ft.pack(m)
        views = []
        views.append(torch.from_numpy(m).to(DEV))                                        # bool, contiguous
        views.append(torch.from_numpy(m.astype(np.uint8) * 200).to(DEV))                 # uint8: any non-zero byte is allowed
        for ld, shift in ((n + 12, 0), (n + 13, 0), (n + 11, 1)):                        # a row stride above n (rows 4-byte aligned or
            buf = torch.ones((rows * ld + shift,), dtype=torch.uint8, device=DEV)        # not), a base one byte off
            v = buf[shift:].view(rows, ld)[:, :n]
            v.copy_(torch.from_numpy(m.astype(np.uint8)))
            assert v.data_ptr() % 4 == shift and v.stride(0) == ld
            views.append(v)
        for v in views:
            words = amd.filter.filter_pack(v)
            assert words.shape == want.shape and words.dtype == torch.int32
            np.testing.assert_array_equal(words.cpu().numpy().view(np.uint32), want, err_msg=f"rows={rows} stride={v.stride(0)}")
        if n % 32:                                                                       # the bits at positions >= n are 0
            assert not (want[:, -1] >> np.uint32(n % 32)).any()
    f = amd.PageFilter.from_mask(torch.from_numpy(m).to(DEV), 3)
    assert f.prepare().max_allowed == int(m.sum(1).max()) and f.rows == 5
    assert amd.PageFilter.from_mask(torch.from_numpy(m[2]).to(DEV)).prepare().max_allowed == int(m[2].sum())


# ----------------------------------------------------------------------------------------------------------------------- mask
def _mask_case(amd, n, ld, seed, kind, with_alive, n_q=5, shift=0):
    r = np.random.default_rng(seed)
    s = (r.standard_normal((n_q, n)) * 4 + 6).astype(np.float32)
    s[r.random((n_q, n)) < 0.1] = -np.inf
    s[r.random((n_q, n)) < 0.1] = np.nan
    s[r.random((n_q, n)) < 0.1] = -0.0
    spec = {sp[0]: sp for sp in _specs(r, n_q, n, 0.5)}[kind]
    alive = (r.random(n) > 0.3).astype(np.uint8) if with_alive else None
    buf = torch.full((n_q * ld + shift,), SENTINEL, dtype=torch.float32, device=DEV)
    view = buf[shift:].view(n_q, ld)[:, :n]
    view.copy_(torch.from_numpy(s))
    alive_d = None if alive is None else torch.from_numpy(alive).to(DEV)
    out = amd.filter.filter_mask(view, _filter(amd, spec, 0, dirty=True), alive_d)
    assert out.data_ptr() == view.data_ptr()
    ok = ft.with_alive(ft.allowed(spec, n_q, n), alive)
    want = np.full((n_q, ld), SENTINEL, dtype=np.float32)
    want[:, :n] = ft.masked(s, ok)
    np.testing.assert_array_equal(_bits(buf[shift:].view(n_q, ld)), want.view(np.int32), err_msg=f"n={n} ld={ld} {kind} alive={with_alive}")
    assert (buf[:shift] == SENTINEL).all()
    return ok


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 1027])
def test_mask_writes_minus_inf_into_disallowed_columns_and_nothing_else(amd, n):
    seen = np.zeros((2,), dtype=np.int64)
    seed = 100 * n
    for kind in ("shared", "per_query", "labels"):
        for with_alive in (False, True):
            ld = (n + 4 + 3) // 4 * 4                                    # rows 16-byte aligned: the vector path, with slack behind n
            ok = _mask_case(amd, n, ld, seed, kind, with_alive)
            seen += [ok.sum(), (~ok).sum()]
            odd = n + 3 if (n + 3) % 2 else n + 4                        # every row starts at another alignment
            _mask_case(amd, n, odd, seed + 1, kind, with_alive)
            _mask_case(amd, n, ld, seed + 2, kind, with_alive, shift=1)  # ld a multiple of 4, the matrix itself 4 bytes off
            _mask_case(amd, n, ld, seed + 3, kind, with_alive, n_q=1)
            seed += 4
    assert seen.min() > 0                                                # both kinds of column occurred


# ----------------------------------------------------------------------------------------------------------------------- list
def _patterns(r, n):
    empty, full = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    first, last, alt = empty.copy(), empty.copy(), empty.copy()
    first[0], last[n - 1] = True, True
    alt[::2] = True
    return [empty, full, first, last, alt, r.random(n) < 0.01, r.random(n) < 0.5]


def _list_check(amd, spec, n_q, n, id_base, m_cap, alive=None, dirty=True):
    ok = ft.with_alive(ft.allowed(spec, n_q, n), alive)
    alive_d = None if alive is None else torch.from_numpy(alive).to(DEV)
    cand, counts, status = amd.filter.filter_list(_filter(amd, spec, id_base, dirty), n_q, m_cap, alive_d)
    want_c, want_n, want_st = ft.list_truth(ok, m_cap, id_base)
    assert cand.shape == (n_q, m_cap) and cand.dtype == torch.int64 and counts.dtype == torch.int32
    np.testing.assert_array_equal(counts.cpu().numpy(), want_n, err_msg=f"{spec[0]} n={n} m_cap={m_cap}")
    np.testing.assert_array_equal(cand.cpu().numpy(), want_c, err_msg=f"{spec[0]} n={n} m_cap={m_cap} id_base={id_base}")
    assert int(status.item()) == want_st
    return want_n, want_st


@pytest.mark.parametrize("n", [1, 33, S - 1, S, S + 1, 3 * S + 5])
def test_list_is_ascending_exact_and_padded(amd, n):
    r = np.random.default_rng(n)
    pats = _patterns(r, n)
    for id_base in (0, 1000):
        for p in pats:                                                   # shared: the same list in every row
            count = int(p.sum())
            for m_cap in (count, count + 7):
                _, st = _list_check(amd, ("shared", p), 3, n, id_base, m_cap)
                assert st == 0
        per = np.stack(pats)                                             # one row per pattern
        top = int(per.sum(1).max())
        for m_cap in (top, top + 7):
            _, st = _list_check(amd, ("per_query", per), len(pats), n, id_base, m_cap)
            assert st == 0
        labels = (r.integers(0, 3, n).astype(np.int32), np.asarray([0, 1, 2, 99, 1], dtype=np.int32))      # 99: no page carries it
        top = int(np.bincount(labels[0], minlength=3).max())
        for m_cap in (top, top + 7):
            counts, st = _list_check(amd, ("labels", *labels), 5, n, id_base, m_cap)
            assert st == 0 and counts[3] == 0
    alive = (r.random(n) > 0.3).astype(np.uint8)
    for spec, n_q in ((("shared", pats[6]), 2), (("per_query", per), len(pats)), (("labels", *labels), 5)):
        _list_check(amd, spec, n_q, n, 1000, n, alive=alive)
        _list_check(amd, spec, n_q, n, 0, n, dirty=False)


def test_list_overflow_keeps_the_first_ids_and_reports_it(amd):
    n = S + 70
    r = np.random.default_rng(9)
    per = np.stack([r.random(n) < 0.5, r.random(n) < 0.1, np.ones(n, dtype=bool)])
    top = int(per.sum(1).max())
    counts, st = _list_check(amd, ("per_query", per), 3, n, 1000, top - 1)
    assert st == 1 and counts.tolist() == per.sum(1).tolist() and counts[2] == n
    _, st = _list_check(amd, ("shared", per[0]), 2, n, 0, int(per[0].sum()) - 1)
    assert st == 1
    labels = (r.integers(0, 2, n).astype(np.int32), np.asarray([0, 1], dtype=np.int32))
    _, st = _list_check(amd, ("labels", *labels), 2, n, 0, int(np.bincount(labels[0]).max()) - 1)
    assert st == 1


# ------------------------------------------------------------------------------------------------------------------------ ids
@pytest.mark.parametrize("n,m", [(1, 1), (70, 9), (1000, 300)])
def test_ids_become_minus_one_only_where_disallowed_in_the_shard(amd, n, m):
    r = np.random.default_rng(n)
    n_q, base = 4, 500
    for spec in _specs(r, n_q, n):
        for alive in (None, (r.random(n) > 0.3).astype(np.uint8)):
            ids = r.integers(base - 5, base + n + 5, size=(n_q, m))
            ids[0, 0] = -1
            ids[-1, -1] = 7                                              # another rank's
            ok = ft.with_alive(ft.allowed(spec, n_q, n), alive)
            want = ft.ids_truth(ids, ok, base)
            ld = m + 3
            buf = torch.full((n_q, ld), -77, dtype=torch.int64, device=DEV)
            view = buf[:, :m]
            view.copy_(torch.from_numpy(ids))
            out = amd.filter.filter_ids(view, _filter(amd, spec, base, dirty=True), None if alive is None else torch.from_numpy(alive).to(DEV))
            assert out.data_ptr() == view.data_ptr() and (buf[:, m:] == -77).all()
            np.testing.assert_array_equal(view.cpu().numpy(), want)
            inside = (ids >= base) & (ids < base + n)
            assert (want[~inside] == ids[~inside]).all() and ((want == -1) | (want == ids)).all()


# --------------------------------------------------------------------------------------------------------------------- search
class _FakeDist:
    """Stands in for torch.distributed inside one process: rank r's message is whatever virtual shard r produced."""

    def __init__(self, messages, me):
        self.messages, self.me = messages, me

    def all_gather_into_tensor(self, out, mine, group=None):
        self.messages[self.me] = mine.clone()
        out.copy_(torch.cat([m.reshape(-1) for m in self.messages]))


def _search_case(dtype, dim=128, seed=1, q_lens=None):
    g = torch.Generator().manual_seed(seed)
    pages = [_unit(g, int(k), dim, dtype) for k in torch.randint(1, 41, (301,), generator=g)]
    for at in (10, 150, 303):                                            # three 0-row pages
        pages.insert(at, _unit(g, 0, dim, dtype))
    pages[77] = pages[20].clone()                                        # an exact tie
    q_lens = q_lens or torch.randint(1, 33, (7,), generator=g).tolist()
    qs = [_unit(g, int(k), dim, dtype) for k in q_lens]
    return pages, qs


def _search_specs(n_q, n, seed=3):
    r = np.random.default_rng(seed)
    specs = _specs(r, n_q, n, 0.1)
    specs[0][1][[10, 20, 77, 150]] = True                                # allowed 0-row pages, and the tie
    specs[1][1][2] = False
    specs[1][1][2, [5, 10, 200]] = True                                  # k larger than this query's allowed count
    specs[1][1][3, [20, 77, 303]] = True
    return specs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_both_routes_equal_the_truth_over_the_scan(amd, dtype):
    pages, qs = _search_case(dtype)
    n, n_q, base, k = len(pages), len(qs), 40, 12
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=base)
    pq = _packed(amd, qs)
    s = amd.maxsim_scores(pq, corpus).cpu().numpy()
    assert np.isneginf(s[:, [10, 150, 303]]).all() and np.isfinite(np.delete(s, [10, 150, 303], axis=1)).all()
    r1 = amd.ShardedRetriever(corpus)
    plain = r1.search(pq, k)
    for spec in _search_specs(n_q, n):
        ok = ft.allowed(spec, n_q, n)
        want_s, want_i = ft.search_truth(s, ok, k, base)
        assert (want_i[:, -1] >= 0).any() and (spec[0] == "shared" or (want_i[:, -1] == -1).any())      # full rows, and starved ones
        for route in ("mask", "list", "auto"):
            got_s, got_i = r1.search(pq, k, filter=_filter(amd, spec, base), filter_route=route)
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=f"{spec[0]} {route}")
        got_s, got_i = r1.search(qs, k, filter=_filter(amd, spec, base))                 # a host list of queries
        np.testing.assert_array_equal(got_i.cpu().numpy(), want_i)
        for world in (2, 3):                                             # virtual shards: the answer does not depend on their number
            shards = []
            for rank in range(world):
                lo, hi = amd.shard_range(n, world, rank)
                sub = (("shared", spec[1][lo:hi]) if spec[0] == "shared" else ("per_query", spec[1][:, lo:hi]) if spec[0] == "per_query"
                       else ("labels", spec[1][lo:hi], spec[2]))
                shards.append((amd.pack_passages(pages[lo:hi], DEV, batch_size=None, id_base=base + lo), sub, base + lo))
            for route in ("mask", "list"):
                nbytes = (n_q * k * 4 + 7) // 8 * 8 + n_q * k * 8
                messages = [torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(world)]
                for _ in range(2):                                       # the first pass fills every rank's message
                    for rank, (shard, sub, lo) in enumerate(shards):
                        rr = amd.ShardedRetriever(shard, world=world, rank=rank, dist=_FakeDist(messages, rank))
                        got_s, got_i = rr.search(pq, k, filter=_filter(amd, sub, lo), filter_route=route)
                np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{spec[0]} {route} world={world}")
                np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32))
    again = r1.search(pq, k, filter=None)                                # filter=None is the unfiltered search
    assert torch.equal(again[1], plain[1]) and torch.equal(again[0], plain[0])


@pytest.fixture(scope="module")
def dist():
    import os
    import socket

    import torch.distributed as d

    created = False
    if not d.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        d.init_process_group(backend="nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
        created = True
    yield d
    if created:
        d.destroy_process_group()


def test_a_forced_one_rank_collective_gives_the_same_answer(amd, dist):
    pages, qs = _search_case(torch.bfloat16, seed=2)
    n, n_q, k = len(pages), len(qs), 9
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    pq = _packed(amd, qs)
    s = amd.maxsim_scores(pq, corpus).cpu().numpy()
    r = amd.ShardedRetriever(corpus, world=1, rank=0, dist=dist, force_collective=True)
    for spec in _search_specs(n_q, n):
        want_s, want_i = ft.search_truth(s, ft.allowed(spec, n_q, n), k)
        for route in ("mask", "list"):
            got_s, got_i = r.search(pq, k, filter=_filter(amd, spec), filter_route=route)
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ width 320
def test_width_320_routes(amd):
    """Six query lengths: the scan runs the flat panel kernel and the routes are bit-identical.  A uniform 4 x 32 batch: the scan
    runs the butterfly kernel; the list route carries the flat panel kernel's bits, which agree with the scan's to the header's
    bound |difference| <= 2 g(L - 1) sum_i |M_i|, g(n) = n 2^-24 / (1 - n 2^-24), sum_i |M_i| <= 1.01 L for unit rows."""
    pages, qs = _search_case(torch.bfloat16, 320, seed=4, q_lens=[1, 17, 32, 33, 64, 100])
    n, k = len(pages), 10
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    r = amd.ShardedRetriever(corpus)
    pq = _packed(amd, qs)
    s = amd.maxsim_scores(pq, corpus).cpu().numpy()
    for spec in _search_specs(6, n):
        want_s, want_i = ft.search_truth(s, ft.allowed(spec, 6, n), k)
        for route in ("mask", "list", "auto"):
            got_s, got_i = r.search(pq, k, filter=_filter(amd, spec), filter_route=route)
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=f"{spec[0]} {route}")
    g = torch.Generator().manual_seed(5)
    L = 32
    uni = [_unit(g, L, 320) for _ in range(4)]
    pu = _packed(amd, uni)
    scan = amd.maxsim_scores(pu, corpus).cpu().numpy()
    forced = amd.maxsim_scores(_packed(amd, uni + [_unit(g, 33, 320)]), corpus).cpu().numpy()[:4]          # a 33-token query forces K1bPF
    n1 = (L - 1) * 2.0 ** -24
    bound = 2.0 * (n1 / (1.0 - n1)) * 1.01 * L
    finite = np.isfinite(scan)
    diff = float(np.abs(scan[finite].astype(np.float64) - forced[finite].astype(np.float64)).max())
    print(f"width 320, uniform 4 x 32: max |scan - flat panel| = {diff:.3e}, bound = {bound:.3e}")
    assert diff <= bound and (np.isfinite(forced) == finite).all()
    spec = _search_specs(4, n)[0]
    ok = ft.allowed(spec, 4, n)
    for route, scores in (("mask", scan), ("list", forced)):
        want_s, want_i = ft.search_truth(scores, ok, k)
        got_s, got_i = r.search(pu, k, filter=_filter(amd, spec), filter_route=route)
        np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=route)
        np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=route)


# ----------------------------------------------------------------------------------------------------------------------- fp32
def test_fp32_corpus_takes_the_mask_route_only(amd):
    pages, qs = _search_case(torch.float32, seed=6)
    n, n_q, k = len(pages), len(qs), 8
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    q = amd.pack_queries(qs, DEV)
    s = amd.maxsim_scores(q, corpus).cpu().numpy()
    r = amd.ShardedRetriever(corpus)
    for spec in _search_specs(n_q, n):
        want_s, want_i = ft.search_truth(s, ft.allowed(spec, n_q, n), k)
        for route in ("mask", "auto"):
            got_s, got_i = r.search(q, k, filter=_filter(amd, spec), filter_route=route)
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{spec[0]} {route}")
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32))
        with pytest.raises(NotImplementedError):
            r.search(q, k, filter=_filter(amd, spec), filter_route="list")


# ------------------------------------------------------------------------------------------------------------------ two-stage
def test_two_stage_search_under_a_filter(amd):
    pages, qs = _search_case(torch.bfloat16, seed=7)
    n, n_q, base, k = len(pages), len(qs), 40, 6
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=base)
    pooled = amd.pack_passages([p[::3].contiguous() for p in pages], DEV, batch_size=None, id_base=base)
    index = amd.Int8Index.build(corpus)
    pq = _packed(amd, qs)
    exact = amd.maxsim_scores(pq, corpus).cpu().numpy()
    r = amd.ShardedRetriever(corpus)
    for prefilter, coarse in ((pooled, amd.maxsim_scores(pq, pooled)), (index, amd.int8_scores(pq, index))):
        coarse = coarse.cpu().numpy()
        for spec in _search_specs(n_q, n):
            ok = ft.allowed(spec, n_q, n)
            sizes = ok.sum(1)
            n_cand = int(sizes[sizes > 0].min()) + 5                     # larger than the smallest allowed set
            want_s, want_i = ft.two_stage_truth(coarse, exact, ok, n_cand, k, base)
            got_s, got_i = r.search(pq, k, prefilter=prefilter, n_candidates=n_cand, filter=_filter(amd, spec, base))
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=spec[0])
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=spec[0])
            got = got_i.cpu().numpy()
            for row, allowed_row in zip(got, ok):
                assert allowed_row[row[row >= 0] - base].all()           # no returned id is disallowed


def test_candidates_under_a_filter(amd):
    pages, qs = _search_case(torch.bfloat16, seed=8)
    n, n_q, base, k = len(pages), len(qs), 40, 6
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=base)
    pq = _packed(amd, qs)
    exact = amd.maxsim_scores(pq, corpus).cpu().numpy()
    g = torch.Generator().manual_seed(8)
    cand = torch.stack([torch.randperm(n + 10, generator=g)[:60] + base - 5 for _ in range(n_q)])      # no duplicates; some off the shard
    cand[0, :3] = -1
    listed = np.zeros((n_q, n), dtype=bool)
    for q_, row in enumerate(cand.numpy()):
        inside = row[(row >= base) & (row < base + n)] - base
        listed[q_, inside] = True
    cand_d = cand.to(DEV)
    before = cand_d.clone()
    r = amd.ShardedRetriever(corpus)
    for spec in _search_specs(n_q, n):
        want_s, want_i = ft.search_truth(exact, listed & ft.allowed(spec, n_q, n), k, base)
        got_s, got_i = r.search(pq, k, candidates=cand_d, filter=_filter(amd, spec, base))
        np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=spec[0])
        np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=spec[0])
    assert torch.equal(cand_d, before)                                   # the caller's list is not written


# ----------------------------------------------------------------------------------------------------------------- LiveCorpus
def test_live_corpus_filters_the_live_pages(amd):
    g = torch.Generator().manual_seed(9)
    pages = [_unit(g, int(k)) for k in torch.randint(1, 41, (90,), generator=g)]
    qs = [_unit(g, k) for k in (8, 20, 5, 32)]
    pq = _packed(amd, qs)
    n, n_q, base, k = 90, 4, 100, 7
    live = amd.LiveCorpus.from_packed(amd.pack_passages(pages[:60], DEV, batch_size=None, id_base=base), spare_rows=1500, spare_docs=40)
    live.add(pages[60:])
    deleted = list(range(1, 90, 3))
    live.delete([base + d for d in deleted])
    alive = np.ones(n, dtype=np.uint8)
    alive[deleted] = 0
    exact = amd.maxsim_scores(pq, live.view()).cpu().numpy()             # before the compaction: every slot still has its rows
    specs = _specs(np.random.default_rng(9), n_q, n, 0.2)
    for step in ("deleted", "compacted"):
        coarse = amd.int8_scores(pq, live.int8_index()).cpu().numpy()
        for spec in specs:
            ok = ft.with_alive(ft.allowed(spec, n_q, n), alive)
            want_s, want_i = ft.search_truth(exact, ok, k, base)
            for route in ("mask", "list", "auto"):
                got_s, got_i = live.search(pq, k, filter=_filter(amd, spec, base), filter_route=route)
                np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{step} {spec[0]} {route}")
                np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=f"{step} {spec[0]} {route}")
                assert not np.isin(got_i.cpu().numpy(), [base + d for d in deleted]).any()
            sizes = ok.sum(1)
            n_cand = int(sizes[sizes > 0].min()) + 3
            want_s, want_i = ft.two_stage_truth(coarse, exact, ok, n_cand, k, base)
            got_s, got_i = live.search(pq, k, prefilter=live.int8_index(), n_candidates=n_cand, filter=_filter(amd, spec, base))
            np.testing.assert_array_equal(got_i.cpu().numpy(), want_i, err_msg=f"{step} {spec[0]} int8")
            np.testing.assert_array_equal(_bits(got_s), want_s.view(np.int32), err_msg=f"{step} {spec[0]} int8")
        live.compact()
    live.check()


# --------------------------------------------------------------------------------------------------------------------- capture
def test_graph_replays_reproduce_the_eager_bits(amd, monkeypatch):
    pages, qs = _search_case(torch.bfloat16, seed=10)
    n, n_q, k = len(pages), len(qs), 8
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=10)
    pq = _packed(amd, qs)
    r = amd.ShardedRetriever(corpus)
    spec = _search_specs(n_q, n)[1]
    fresh = _filter(amd, spec, 10)
    assert fresh.max_allowed is None
    r.search(pq, k, filter=fresh)                                        # an unprepared filter synchronises once ...
    assert fresh.max_allowed == int(ft.allowed(spec, n_q, n).sum(1).max())
    unprepared = _filter(amd, spec, 10)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="before the capture"):        # ... which a capture cannot hold
        r.search(pq, k, filter=unprepared)
    monkeypatch.undo()
    for route in ("mask", "list"):
        flt = _filter(amd, spec, 10).prepare()
        eager = [t.clone() for t in r.search(pq, k, filter=flt, filter_route=route)]
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = r.search(pq, k, filter=flt, filter_route=route)
        for _ in range(2):
            for t in outs:
                t.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(outs[1], eager[1]) and torch.equal(outs[0].view(torch.int32), eager[0].view(torch.int32)), route


# ---------------------------------------------------------------------------------------------------------------------- errors
def test_error_paths(amd):
    pages, qs = _search_case(torch.bfloat16, seed=11)
    n, n_q = len(pages), len(qs)
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=5)
    pq = _packed(amd, qs)
    r = amd.ShardedRetriever(corpus)
    ones = torch.ones(n, dtype=torch.bool, device=DEV)
    PF = amd.PageFilter
    good = PF.from_mask(ones, 5)
    assert (r.search(pq, 3, filter=good)[1] >= 5).all()
    host_labels = PF.from_labels(torch.zeros(n, dtype=torch.int32), torch.zeros(n_q, dtype=torch.int32), 5)
    for bad in (PF.from_mask(ones[:-1], 5), PF.from_mask(ones, 0), PF.from_mask(ones.repeat(n_q + 1, 1), 5), host_labels,
                PF.from_labels(torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n_q + 2, dtype=torch.int32, device=DEV), 5)):
        for route in ("auto", "mask", "list"):
            with pytest.raises(ValueError):
                r.search(pq, 3, filter=bad, filter_route=route)
    with pytest.raises(ValueError, match="filter_route"):
        r.search(pq, 3, filter=good, filter_route="fastest")
    with pytest.raises(ValueError):
        PF.from_mask(ones.cpu())                                         # the packing is a gfx950 kernel
    scores = torch.zeros((n_q, n), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError):
        amd.filter.filter_mask(scores[:, :-1], good)
    with pytest.raises(ValueError):
        amd.filter.filter_mask(scores, good, alive=torch.ones(n - 1, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        amd.filter.filter_ids(torch.zeros((n_q + 1, 4), dtype=torch.int64, device=DEV), PF.from_mask(ones.repeat(n_q, 1), 5))
