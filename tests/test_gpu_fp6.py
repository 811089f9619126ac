"""E2M3 (FP6) query tokens against the FP4 index on the MI355X (msim_f6_encode_rows, msim_f4_scores_q6, colpali_amd.fp6_scores,
ShardedRetriever(fp4_score_fn=fp6_scores)).

Codes and scores are checked bit for bit against the numpy restatement in tests/fp6_truth.py; nothing here has a tolerance.  With
two formats in one instruction the operand map is no longer symmetric, so the first test settles on hand-made data what the scorer
rests on: (d) nibble j of an FP4 lane meets 6-bit field j of the FP6 lane, ascending from the low bit of the lane's registers,
(e) the B scale is byte 0 of its register at op_sel 0, (f) the mixed-format sum is exact.  The scorer's body is new, so the shapes
are those of tests/test_gpu_fp4.py: rows around the 16-row chunk, pages of 1-3 rows, page ranges of 1, 8-16 and 63 pages, queries
around the 16-token tile and past one wave's 128 tokens, every launch form.  The page side, the helpers and the seeds are that
file's."""
import numpy as np
import pytest
import torch

from tests import fp4_truth as ft
from tests import fp6_truth as f6
from tests import test_fp6_host as host
from tests import test_gpu_fp4 as t4
from tests.test_gpu_fp4 import (DEV, D, K, M_CAND, NT, _bits, _index_of_codes, _packed, _passes, _plan, _ragged_range_lens, _random_codes,
                                _scaled, _unit)

pytestmark = pytest.mark.gpu

PAGE_LENS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 100)
QUERY_LENS = (0, 1, 15, 16, 17, 32, 33, 127, 128, 129, 300)
ALL_FORMS = {(NT, 1, D), (NT, 2, D), (NT, 4, D)}

# query batches by the launch form they reach: name -> (query lengths, GW, passes); at 32 tokens n_q <= 4, 5-8 and >= 9
BATCHES = dict(t4.BATCHES)
BATCHES.update({"gw1-32x4": ([32] * 4, 1, 1), "gw2-32x5": ([32] * 5, 2, 1), "gw2-32x8": ([32] * 8, 2, 1), "gw4-32x9": ([32] * 9, 4, 1)})


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _q_codes(q):
    return f6.encode(ft.raw_bits(q.tokens.cpu()), f16=q.tokens.dtype == torch.float16)


def _truth(q, codes, scales, off, clamp0=None):
    """the truth scores of packed queries `q` (coded as e2m3 by the truth) against host FP4 codes"""
    qc, qs = _q_codes(q)
    return f6.scores(qc, qs, q.offsets_host.numpy(), codes, scales, off, clamp0)


def _check(amd, q, idx, codes, scales, off, clamp0=None):
    got = amd.fp6_scores(q, idx)
    want = _truth(q, codes, scales, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    return got, want


# ------------------------------------------------------------------------------------------------------- the hardware's facts
def exact_data():
    """145 hand-made tokens and 17 page rows.
    Tokens 0 .. 127 are one-hot, one per dimension k: code k % 31 + 1 with sign k & 1 (31 is odd: every non-zero code with both
    signs), so token k reads column k of the page rows and nothing else.  Tokens 128 .. 144 are dense: all -7.5, all +7.5 and 15
    of random fields (never the -0 field 32).  Page row 0 is all +6 (|I| = 128 * 7.5 * 6 = 5760 against tokens 128 and 129); the
    others carry random nibbles (never -0), every column of the 17 rows different from every other, so a field that met another
    nibble of its lane -- or another lane's -- would change a one-hot token's Z.  Exponents -8 .. 8 on both sides."""
    rng = np.random.default_rng(6)
    d_nib = rng.integers(0, 16, (17, 128), dtype=np.uint8)
    d_nib[d_nib == 8] = 0
    d_nib[0] = 7
    q_f = np.zeros((145, 128), dtype=np.uint8)
    k = np.arange(128)
    q_f[k, k] = (k % 31 + 1) | ((k & 1) << 5)
    dense = rng.integers(0, 64, (17, 128), dtype=np.uint8)
    dense[dense == 32] = 0
    dense[0], dense[1] = 63, 31
    dense[2, :63] = [v for v in range(64) if v != 32]               # every field value in one token, at positions 0 .. 62
    q_f[128:] = dense
    ds = (127 + (np.arange(17) * 5) % 17 - 8).astype(np.uint8)
    qs = (127 + (np.arange(145) * 7 + 3) % 17 - 8).astype(np.uint8)
    return ft.pack_nibbles(d_nib), ds, f6.pack_fields(q_f), qs, d_nib, q_f


def test_exact_data_settles_the_field_order_the_scale_byte_and_the_sum(amd):
    """Every Z_ij bit for bit: each of the 17 rows as a page of its own against each of the 145 tokens as a query of its own (a
    one-token score is 0 + M), then the 17 rows as ONE page (a full chunk and a masked one), and the 145 tokens as one query (two
    passes)."""
    dc, ds, qc, qs, d_nib, q_f = exact_data()
    assert set(np.unique(d_nib)) == set(range(16)) - {8}                                                   # all 15 FP4 values
    assert set(np.unique(q_f[:128][q_f[:128] > 0])) == set(range(64)) - {0, 32}                            # one-hot: all 62 non-zero
    assert set(np.unique(q_f[128:])) == set(range(64)) - {32}
    assert len({c.tobytes() for c in ft.decode(dc).T}) == 128                                              # no two columns alike
    assert len(set(ds.tolist())) == 17 and len(set(qs.tolist())) == 17
    lens = [1] * 17 + [17]
    codes, scales = np.concatenate([dc, dc]), np.concatenate([ds, ds])
    idx, off = _index_of_codes(amd, codes, scales, lens)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for q_off in (np.arange(146, dtype=np.int32), np.array([0, 145], dtype=np.int32)):
        max_q = int(np.diff(q_off).max())
        got = amd.fp4_scores_from_codes(t(qc), t(qs), t(q_off), max_q, idx, query_code="e2m3").cpu().numpy()
        want = f6.scores(qc, qs, q_off, codes, scales, off)
        if len(q_off) == 146:
            Z = f6.maxima(qc, qs, dc, ds, np.arange(18))
            np.testing.assert_array_equal(want[:, :17], Z)                                  # the one-row pages ARE the Z matrix
            assert Z[128, 0] == -5760 * 2.0 ** (int(qs[128]) + int(ds[0]) - 254)
            assert Z[129, 0] == 5760 * 2.0 ** (int(qs[129]) + int(ds[0]) - 254)
            kk = np.arange(128)                                                                # a one-hot token reads ITS column
            vq = f6.GRID[kk % 31 + 1] * np.where(kk & 1, -1.0, 1.0)
            np.testing.assert_array_equal(Z[:128], np.ldexp(vq[:, None] * ft.decode(dc).T,
                                                            qs[:128, None].astype(int) + ds[None, :].astype(int) - 254))
        dev = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        assert not len(bad), (f"{len(q_off) - 1} queries: {len(bad)} scores differ, first (query, page) {bad[:8].tolist()}; largest "
                              f"deviation {dev:g} (largest |score| {np.abs(want).max():g})")


# ---------------------------------------------------------------------------------------------------------------------- encode
def encode_rows(dtype):
    """raw 16-bit rows: random rows of many magnitudes (87: the last 16-row block of the launch is partial) with the host file's
    edge rows written over the first ones"""
    g = torch.Generator().manual_seed(1)
    lens = [0, 1, 15, 16, 17, 33, 5]
    raw = ft.raw_bits(torch.cat([_scaled(g, n, dtype) for n in lens])).copy()
    edge = host.edge_rows()[0] if dtype == torch.bfloat16 else host.edge_rows_f16()
    raw[20:20 + len(edge)] = edge
    return raw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encode_is_bit_equal_to_the_truth(amd, dtype):
    raw = encode_rows(dtype)
    want_c, want_s = f6.encode(raw, dtype == torch.float16)
    blob = torch.from_numpy(raw.view(np.int16)).view(dtype)
    qc, qs = amd.fp6_quantize_queries(_packed(amd, [blob[:33], blob[33:34], blob[34:87]]))
    assert qc.shape == (87, 96) and qc.dtype == torch.uint8 and qs.shape == (87,) and qs.dtype == torch.uint8
    np.testing.assert_array_equal(qs.cpu().numpy(), want_s)
    np.testing.assert_array_equal(qc.cpu().numpy(), want_c)
    qc2, qs2 = amd.fp6_quantize_queries([blob[36:60], blob[60:87]], DEV)        # a host list (of the random rows) is packed first
    assert torch.equal(qc2, qc[36:]) and torch.equal(qs2, qs[36:])


# ---------------------------------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module")
def edges(amd):
    """The page lengths round the 16-row chunk, empty pages first, among them and last, clamp0 on a random half"""
    g = torch.Generator().manual_seed(2)
    lens = list(PAGE_LENS) + [47, 0, 64, 0, 0]
    pages = [_scaled(g, n) for n in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    clamp0 = (torch.rand(len(lens), generator=g) < 0.5).to(torch.uint8)
    corpus.clamp0 = clamp0.to(DEV)
    idx = amd.Fp4Index.build(corpus)
    codes, scales = ft.encode(ft.raw_bits(torch.cat(pages)))
    return idx, codes, scales, corpus.offsets.cpu().numpy(), clamp0.numpy(), lens


@pytest.mark.parametrize("name", list(BATCHES))
def test_scores_are_bit_equal_to_the_truth(amd, edges, name):
    idx, codes, scales, off, clamp0, lens = edges
    qlens, gw, passes = BATCHES[name]
    assert _plan(amd, len(qlens), max(qlens), len(idx), len(codes))[:3] == (NT, gw, D) and _passes(max(qlens)) == passes
    g = torch.Generator().manual_seed(len(name) + sum(qlens))
    q = _packed(amd, [_scaled(g, n) for n in qlens])
    got, want = _check(amd, q, idx, codes, scales, off, clamp0)
    got = got.cpu().numpy()
    empty = [i for i, n in enumerate(lens) if n == 0]
    assert np.isneginf(got[:, empty]).all() and np.isfinite(np.delete(got, empty, axis=1)).all()
    for i, n in enumerate(qlens):
        if n == 0:                                                  # a 0-token query scores 0 against every page that has rows
            assert (np.delete(got[i], empty) == 0).all()


@pytest.fixture(scope="module")
def tiny_pages(amd):
    """60 000 pages of 0-3 rows (one 16-row chunk closes several pages), the last three empty, clamp0 on a random half: one wave
    scores a range of 8 or more pages"""
    rng = np.random.default_rng(3)
    n = 60000
    lens = rng.choice(np.array([0, 1, 1, 2, 2, 3]), n)
    lens[-3:] = 0
    if lens.sum() % 16 == 0:
        lens[0] += 1
    codes, scales = _random_codes(rng, int(lens.sum()))
    clamp0 = (rng.random(n) < 0.5).astype(np.uint8)
    idx, off = _index_of_codes(amd, codes, scales, lens, clamp0)
    return idx, codes, scales, off, clamp0


@pytest.mark.parametrize("name", ["gw1-four", "gw1-passes2", "gw2-seven", "gw2-passes3", "gw4-wide"])
def test_ranges_of_one_to_three_row_pages(amd, tiny_pages, name):
    idx, codes, scales, off, clamp0 = tiny_pages
    qlens, gw, _ = BATCHES[name]
    plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
    assert plan[:3] == (NT, gw, D) and plan[3] >= 8, plan
    g = torch.Generator().manual_seed(40 + sum(qlens))
    _check(amd, _packed(amd, [_scaled(g, n) for n in qlens]), idx, codes, scales, off, clamp0)


@pytest.mark.parametrize("n_pages", [63, 64, 65, 130])
@pytest.mark.parametrize("name", ["gw1-four", "gw4-wide"])
def test_page_counts_around_a_full_range(amd, n_pages, name):
    rng = np.random.default_rng(n_pages)
    lens = rng.integers(0, 41, n_pages)
    codes, scales = _random_codes(rng, int(lens.sum()))
    clamp0 = (rng.random(n_pages) < 0.5).astype(np.uint8)
    idx, off = _index_of_codes(amd, codes, scales, lens, clamp0)
    qlens = BATCHES[name][0]
    g = torch.Generator().manual_seed(n_pages)
    _check(amd, _packed(amd, [_scaled(g, n) for n in qlens]), idx, codes, scales, off, clamp0)


def test_full_ranges_of_63_pages(amd):
    """Enough 0-3 row pages that one query group's waves take the full 63 pages each, 65 pages past a whole number of waves"""
    want_waves = torch.cuda.get_device_properties(DEV).multi_processor_count * 32
    n = want_waves * 63 + 65
    rng = np.random.default_rng(5)
    lens = rng.choice(np.array([0, 1, 1, 1, 2, 3]), n)
    codes, scales = _random_codes(rng, int(lens.sum()))
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qlens = [32, 7]
    assert _plan(amd, len(qlens), 32, n, len(codes)) == (NT, 1, D, 63)
    g = torch.Generator().manual_seed(6)
    _check(amd, _packed(amd, [_scaled(g, k) for k in qlens]), idx, codes, scales, off)


def test_every_launch_form_is_reached(amd, edges, tiny_pages):
    """The shapes of the parity tests above, by the form msim_f4_scores_plan names for them (it describes both scorers): every
    (NT, GW, D), one pass and several, page ranges of 1 and of 8 or more; at 32-token queries GW 1, 2, 4 at n_q <= 4, 5-8, >= 9."""
    forms, passes, ranges = set(), set(), set()
    for idx, codes in ((edges[0], edges[1]), (tiny_pages[0], tiny_pages[1])):
        for qlens, gw, n_pass in BATCHES.values():
            plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
            assert plan[1] == gw
            forms.add(plan[:3])
            passes.add((plan[1], _passes(max(qlens)) > 1))
            ranges.add(1 if plan[3] == 1 else 8 if plan[3] >= 8 else 0)
    assert forms == ALL_FORMS, (forms, ALL_FORMS)
    assert passes == {(gw, many) for gw in (1, 2, 4) for many in (False, True)}
    assert ranges == {1, 8}
    for n_q in range(1, 13):
        assert _plan(amd, n_q, 32, len(edges[0]), len(edges[1]))[1] == (1 if n_q <= 4 else 2 if n_q <= 8 else 4)


# ------------------------------------------------------------------------------------------------------- the all-negative tier
@pytest.mark.parametrize("name,n_pages", [("gw1-four", 12), ("gw4-wide", 12), ("gw1-passes2", 12), ("gw1-four", 60000), ("gw2-seven", 60000)])
def test_rows_past_a_range_never_score(amd, name, n_pages):
    """Every similarity is negative, so ONE zero row -- what the descriptors return past a range's end -- that reached a maximum
    would raise it to 0 and change the score: asserted on the truth before the device's output is read."""
    qlens = [n for n in BATCHES[name][0] if n]
    rng = np.random.default_rng(8)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)                     # no range ends on a chunk boundary
    assert _plan(amd, len(qlens), max(qlens), n_pages, int(lens.sum()))[3] == ppw and (ppw == 1) == (n_pages == 12)
    qs, codes, scales, _ = t4.far_side(7, qlens, lens, planted=False)
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    assert (f6.maxima(qc, qsc, codes, scales, off) < 0).all()        # a leaked zero row would have changed every maximum
    _check(amd, q, idx, codes, scales, off)


@pytest.mark.parametrize("n_pages", [12, 60000])
def test_a_winner_on_the_first_and_the_last_row_scores(amd, n_pages):
    """The mask's other side: a row on the queries' side planted on row 0 of every even page and on the last row of every odd one
    is the winner of every token; every other row stays negative."""
    qlens = [17, 32, 5]
    rng = np.random.default_rng(10)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)
    lens[lens == 1] = 2                                              # two rows at least: first and last differ
    for p0 in range(0, n_pages, ppw):
        if lens[p0:p0 + ppw].sum() % 16 == 0:
            lens[min(p0 + ppw, n_pages) - 1] += 1
    assert all(lens[p0:p0 + ppw].sum() % 16 for p0 in range(0, n_pages, ppw)) and lens.max() < 32
    qs, codes, scales, rows = t4.far_side(9, qlens, lens, planted=True)
    assert all(r == (0 if c % 2 == 0 else lens[c] - 1) for c, r in enumerate(rows))
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    M = f6.maxima(qc, qsc, codes, scales, off)
    won = f6.maxima(qc, qsc, codes[off[:-1] + np.asarray(rows)], scales[off[:-1] + np.asarray(rows)], np.arange(n_pages + 1))
    assert (M > 0).all() and np.array_equal(M, won)                  # the planted row wins every token of every page
    _check(amd, q, idx, codes, scales, off)


# ------------------------------------------------------------------------------------------------------------------- placement
def test_permuting_the_pages_permutes_the_bits(amd, edges):
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(11)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    base = amd.fp6_scores(q, idx)
    perm = np.random.default_rng(12).permutation(len(lens))
    p_codes = np.concatenate([codes[off[c]:off[c + 1]] for c in perm])
    p_scales = np.concatenate([scales[off[c]:off[c + 1]] for c in perm])
    p_idx, _ = _index_of_codes(amd, p_codes, p_scales, np.asarray(lens)[perm], clamp0[perm])
    np.testing.assert_array_equal(_bits(amd.fp6_scores(q, p_idx)), _bits(base)[:, perm])


def test_scores_do_not_depend_on_the_batch(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(13)
    lens = torch.randint(1, 40, (300,), generator=g).tolist()
    qs = [_unit(g, n) for n in lens]
    full = amd.fp6_scores(_packed(amd, qs), idx)                          # GW 4
    for i in (0, 1, 157, 299):
        np.testing.assert_array_equal(_bits(amd.fp6_scores(_packed(amd, [qs[i]]), idx)[0]), _bits(full[i]))     # GW 1
    np.testing.assert_array_equal(_bits(amd.fp6_scores(_packed(amd, qs[:3]), idx)), _bits(full[:3]))
    long_q = [_unit(g, 300), qs[7]]                                       # beside a query of several passes: GW 2
    np.testing.assert_array_equal(_bits(amd.fp6_scores(_packed(amd, long_q), idx)[1]), _bits(full[7]))
    np.testing.assert_array_equal(_bits(amd.fp6_scores(_packed(amd, qs), idx)), _bits(full))


def test_broken_device_offsets_come_back_as_nan_over_that_range_only(amd, edges):
    """Offsets are checked before they become addresses (the scorer's contract): nothing is read out of bounds"""
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(14)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17)])
    assert _plan(amd, 3, 32, len(idx), len(codes))[3] == 1               # one page per range: a broken offset spoils its two pages
    want = _truth(q, codes, scales, off, clamp0)
    for j, bad_value in ((5, len(codes) + 7), (9, -1)):
        bad = torch.from_numpy(off.copy())
        bad[j] = bad_value
        broken = amd.Fp4Index(idx.codes, idx.scales, bad.to(DEV), idx.clamp0, idx.lengths)
        got = amd.fp6_scores(q, broken).cpu().numpy()
        assert np.isnan(got[:, [j - 1, j]]).all()
        keep = [c for c in range(len(lens)) if c not in (j - 1, j)]
        np.testing.assert_array_equal(got[:, keep].view(np.int32), want[:, keep].view(np.int32))
    # a query whose offsets leave the token count: NaN over that query only (an empty page stays -inf)
    qc, qs = amd.fp6_quantize_queries(q)
    q_bad = q.offsets.clone()
    q_bad[2] = int(q.tokens.shape[0]) + 3
    got = amd.fp4_scores_from_codes(qc, qs, q_bad, 32, idx, query_code="e2m3").cpu().numpy()
    rows = [c for c, n in enumerate(lens) if n]
    assert np.isnan(got[1:, rows]).all()
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


def test_a_captured_fp6_scores_replays_the_eager_bits(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(18)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.fp6_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.fp6_scores(q, idx, out=out)                                  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.fp6_scores(q, idx, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(first))


# ------------------------------------------------------------------------------------------------------------ two-stage search
def fp6_ranks(qs, pages, off, allowed=None):
    """the truth's FP6 score matrix as ranks: rank[q, c] = pages (allowed ones) that (score desc, id asc) puts before page c"""
    S = f6.score_blocks([ft.raw_bits(q) for q in qs], ft.raw_bits(torch.cat(pages)), off).astype(np.float64)
    if allowed is not None:
        S = np.where(allowed[None, :], S, -np.inf)
    order = np.argsort(-S, axis=1, kind="stable")
    ranks = np.empty_like(order)
    for i in range(len(qs)):
        ranks[i, order[i]] = np.arange(S.shape[1])
    return ranks


@pytest.fixture(scope="module")
def search(amd):
    """the case and the seeds of the FP4 test; the precondition on the truth alone: every exact top-5 page ranks below m = 64"""
    pages, qs = t4.search_case()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pages])])
    exact = t4.exact_scores(qs, torch.cat(pages).double().numpy(), off)
    worst = t4.worst_rank(exact, fp6_ranks(qs, pages, off))
    print(f"worst FP6 rank of an exact top-{K} page: {worst}")
    assert worst < M_CAND
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=100)
    return corpus, amd.Fp4Index.build(corpus), _packed(amd, qs), pages, qs, off, exact


def test_two_stage_search_returns_the_exact_search(amd, search):
    corpus, idx, q, pages, qs, off, exact = search
    r = amd.ShardedRetriever(corpus, fp4_score_fn=amd.fp6_scores)
    es, ei = r.search(q, k=K)
    s, i = r.search(q, k=K, prefilter=idx, n_candidates=M_CAND)
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    assert (ei[:, 0].cpu() - 100).tolist() == [37 * j + 11 for j in range(6)]       # the planted pages come first
    _, cand = amd.topk(amd.fp6_scores(q, idx), M_CAND, idx.id_base)                 # stage 1 is fp6_scores: (score desc, id asc)
    want = np.argsort(-_truth(q, *ft.encode(ft.raw_bits(torch.cat(pages))), off).astype(np.float64), axis=1, kind="stable")[:, :M_CAND]
    np.testing.assert_array_equal(cand.cpu().numpy() - 100, want)


def test_two_stage_search_with_a_filter_and_with_groups(amd, search):
    corpus, idx, q, pages, qs, off, exact = search
    n = len(corpus)
    g = torch.Generator().manual_seed(16)
    allowed = torch.rand(n, generator=g) < 0.5
    assert t4.worst_rank(exact, fp6_ranks(qs, pages, off, allowed.numpy()), allowed=allowed.numpy()) < M_CAND
    r = amd.ShardedRetriever(corpus, fp4_score_fn=amd.fp6_scores)
    flt = amd.PageFilter.from_mask(allowed.to(DEV), 100)
    es, ei = r.search(q, k=K, filter=flt)
    s, i = r.search(q, k=K, prefilter=idx, n_candidates=M_CAND, filter=flt)
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    assert allowed[(i - 100).cpu()].all()

    labels = torch.randint(0, 60, (n,), generator=g)
    lab = labels.numpy()
    best = np.full((len(qs), 60), -1)
    doc_s = np.full((len(qs), 60), -np.inf)
    for c in range(n):                                               # every document's best page, the lower id on a tie
        better = exact[:, c] > doc_s[:, lab[c]]
        doc_s[better, lab[c]], best[better, lab[c]] = exact[better, c], c
    top_docs = np.argsort(-doc_s, axis=1, kind="stable")[:, :K]
    ranks = fp6_ranks(qs, pages, off)
    assert np.take_along_axis(ranks, np.take_along_axis(best, top_docs, axis=1), axis=1).max() < M_CAND
    groups = amd.PageGroups.from_labels(labels.to(DEV), 100)
    es, eg, ep = r.search(q, k=K, group_by=groups)
    gs, gg, gp = r.search(q, k=K, prefilter=idx, n_candidates=M_CAND, group_by=groups)
    np.testing.assert_array_equal(gg.cpu().numpy(), eg.cpu().numpy())
    np.testing.assert_array_equal(gp.cpu().numpy(), ep.cpu().numpy())
    np.testing.assert_array_equal(_bits(gs), _bits(es))


def test_two_stage_search_over_a_residual_corpus(amd, search):
    corpus, idx, q, pages, qs, off, _ = search                       # the index was built from the bf16 pages
    g = torch.Generator().manual_seed(17)
    C = corpus.blob[torch.randperm(int(corpus.blob.shape[0]), generator=g)[:256].to(DEV)].contiguous()
    rc = amd.ResidualCorpus.build(corpus, index=amd.CentroidIndex.build(corpus, centroids=C), bits=4)
    decoded = rc.decompress().blob.double().cpu().numpy()            # the rows the compressed shard scores, for the precondition
    assert t4.worst_rank(t4.exact_scores(qs, decoded, off), fp6_ranks(qs, pages, off)) < M_CAND
    es, ei = amd.ShardedRetriever(rc, score_fn=amd.residual_scores).search(q, k=K)
    s, i = amd.ShardedRetriever(rc, fp4_score_fn=amd.fp6_scores).search(q, k=K, prefilter=idx, n_candidates=M_CAND)
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    assert (i >= 100).all()


# ------------------------------------------------------------------------------------------------- the stored index stays FP4
def test_one_index_serves_both_query_codes(amd, edges):
    idx, codes, scales, off, clamp0, lens = edges
    before = [t.clone() for t in (idx.codes, idx.scales, idx.offsets, idx.clamp0)]
    g = torch.Generator().manual_seed(21)
    q = _packed(amd, [_scaled(g, n) for n in (32, 5, 17, 33)])
    got6 = amd.fp6_scores(q, idx)
    got4 = amd.fp4_scores(q, idx)
    again6 = amd.fp4_scores(q, idx, query_code="e2m3")
    np.testing.assert_array_equal(_bits(got6), _truth(q, codes, scales, off, clamp0).view(np.int32))
    np.testing.assert_array_equal(_bits(got4), t4._truth(q, codes, scales, off, clamp0).view(np.int32))
    np.testing.assert_array_equal(_bits(again6), _bits(got6))
    assert not torch.equal(got4, got6)
    for t, b in zip((idx.codes, idx.scales, idx.offsets, idx.clamp0), before):
        assert torch.equal(t, b)
    with pytest.raises(ValueError, match="out must be"):
        amd.fp6_scores(q, idx, out=torch.empty(3, 5, device=DEV))
    with pytest.raises(NotImplementedError, match="the fp4 index takes bfloat16 / float16 queries of width 128"):
        amd.fp6_scores(_packed(amd, [torch.randn(4, 320).to(torch.bfloat16)]), idx)
