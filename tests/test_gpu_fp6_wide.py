"""E2M3 (FP6) query tokens against the 320-wide FP4 index on the MI355X (msim_f6w_encode_rows, msim_f4w_scores_q6,
colpali_amd.fp6_wide_scores).

Codes and scores are checked bit for bit against the numpy restatement in tests/fp6_wide_truth.py; nothing here has a tolerance.
With two formats in one instruction the wide kernel's symmetry argument is gone, so the first test settles on hand-made data what
the scorer rests on beyond the facts of tests/test_gpu_fp6.py and tests/test_gpu_fp4_wide.py: in the HALF-FILLED third K block,
fields 0 .. 15 of a lane's FP6 operand meet nibbles 0 .. 15 of its FP4 operand, the zero registers above them add nothing, and the
three mixed-format blocks chain exactly through the C operand.  The scorer's body is new, so the shapes are those of
tests/test_gpu_fp4_wide.py: rows around the 16-row chunk, pages of 0-3 rows, page ranges of 1, 8-16 and 63 pages, queries around the
16-token tile and past one wave's NT tiles, every launch form.  The page side, the helpers and the seeds are that file's."""
import numpy as np
import pytest
import torch

from tests import fp4_wide_truth as wt
from tests import fp6_truth as f6
from tests import fp6_wide_truth as f6w
from tests import test_fp6_wide_host as host
from tests import test_gpu_fp4_wide as tw
from tests.test_gpu_fp4_wide import (ALL_FORMS, BATCHES, DEV, MARGIN, NT, PAGE_LENS, D, W, _bits, _index_of_codes, _packed, _passes, _plan,
                                     _ragged_range_lens, _random_codes, _scaled, _unit)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _q_codes(q):
    return f6w.encode(wt.raw_bits(q.tokens.cpu()), f16=q.tokens.dtype == torch.float16)


def _truth(q, codes, scales, off, clamp0=None):
    """the truth scores of packed queries `q` (coded as e2m3 by the truth) against host FP4 codes"""
    qc, qs = _q_codes(q)
    return f6w.scores(qc, qs, q.offsets_host.numpy(), codes, scales, off, clamp0)


def _check(amd, q, idx, codes, scales, off, clamp0=None):
    got = amd.fp6_wide_scores(q, idx)
    want = _truth(q, codes, scales, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    return got, want


# ------------------------------------------------------------------------------------------------------- the hardware's facts
N_ROWS, N_TOK = 23, 343


def exact_data():
    """Hand-made codes.
    Page rows (23): row 0 all +6; rows 1 .. 16 random nibbles (never -0), every one of the 320 columns different from every other;
    rows 17 .. 20 have K block 0 all +6 and block 1 all -6 (or the signs swapped) and ONE small value in block 2; rows 21 and 22 have
    32 dimensions of -6 (+6) in each of blocks 0 and 1 and all 64 dimensions of block 2 at +6 (-6).
    Tokens (343): token k < 320 is one-hot at dimension k -- code k % 31 + 1 with sign k & 1, so token k reads column k of the rows
    and nothing else: every dimension of block 2 on its own, and every one of blocks 0 and 1.  Tokens 320 .. 336 are dense: all -7.5,
    all +7.5, every field value in one token, 14 random ones.  Tokens 337 .. 340 meet rows 17 .. 20: +7.5 over blocks 0 and 1 (the
    block sums are +-5760 and cancel) and one value at the row's small dimension.  Tokens 341 and 342 meet rows 21 and 22: 7.5 where
    the row has values, so that blocks 0 + 1 give -1440 - 1440 (+2880) and block 2 +2880 (-2880) but for ONE field of block 2 at 7.0
    (5.0): the answer is -3 (+15), what is left when blocks 0 + 1 cancel block 2.
    Scale bytes: 17 different ones on each side, never equal for a row and the token made for it."""
    rng = np.random.default_rng(4)
    d_nib = rng.integers(0, 16, (N_ROWS, W), dtype=np.uint8)
    d_nib[d_nib == 8] = 0
    d_nib[0] = 7
    q_f = np.zeros((N_TOK, W), dtype=np.uint8)
    k = np.arange(W)
    q_f[k, k] = (k % 31 + 1) | ((k & 1) << 5)
    dense = rng.integers(0, 64, (17, W), dtype=np.uint8)
    dense[dense == 32] = 0
    dense[0], dense[1] = 63, 31
    dense[2, 250:313] = [v for v in range(64) if v != 32]              # every field value in one token, across blocks 1 and 2
    q_f[320:337] = dense
    for r, (s0, s1, k2, v2, f2) in enumerate([(7, 15, 256, 1, 1), (15, 7, 319, 1, 33), (7, 15, 300, 9, 31), (15, 7, 271, 7, 24)]):
        d_nib[17 + r] = 0
        d_nib[17 + r, :128], d_nib[17 + r, 128:256], d_nib[17 + r, k2] = s0, s1, v2
        q_f[337 + r] = 0
        q_f[337 + r, :256], q_f[337 + r, k2] = 31, f2
    for r, (s01, s2, k2, f2) in enumerate([(15, 7, 287, 30), (7, 15, 256, 26)]):
        d_nib[21 + r] = 0
        d_nib[21 + r, 40:72], d_nib[21 + r, 200:232], d_nib[21 + r, 256:] = s01, s01, s2
        q_f[341 + r] = 0
        q_f[341 + r, 40:72], q_f[341 + r, 200:232], q_f[341 + r, 256:] = 31, 31, 31
        q_f[341 + r, k2] = f2
    ds = (127 + (np.arange(N_ROWS) * 5) % 17 - 8).astype(np.uint8)
    qs = (127 + (np.arange(N_TOK) * 7 + 3) % 17 - 8).astype(np.uint8)
    ds[17:23] = [127 + 3, 127 - 5, 127 + 8, 127 - 8, 127 + 5, 127 - 2]
    qs[337:343] = [127 - 7, 127 + 6, 127 + 7, 127 - 6, 127 - 4, 127 + 1]
    return wt.pack_nibbles(d_nib), ds, f6w.pack_fields(q_f), qs, d_nib, q_f


def test_exact_data_settles_the_half_filled_block_and_the_mixed_chain(amd):
    """Every Z_ij bit for bit: each of the 23 rows as a page of its own against each of the 343 tokens as a query of its own (a
    one-token score is 0 + M), then the 23 rows as ONE page (16 + 7 rows: a full chunk and a masked one) against the one-token
    queries and against all tokens as one query (six passes).  What the one-hot tokens' Z must be is worked out from the grids alone,
    without the truth's packing: token k reads column k.  A field of block 2 that met another nibble of its lane, another lane's, or
    the empty upper half changes that token's Z, since no two columns of the rows are alike and row 0 has no zero; a C operand that
    is scaled again or rounded changes the cancelling rows."""
    dc, ds, qc, qs, d_nib, q_f = exact_data()
    assert set(np.unique(d_nib)) == set(range(16)) - {8}                                                   # all 15 FP4 values
    assert set(np.unique(q_f[:W][q_f[:W] > 0])) == set(range(64)) - {0, 32}                                # one-hot: all 62 non-zero
    assert set(np.unique(q_f[W:])) == set(range(64)) - {32}
    vd = wt.decode(dc)
    assert len({c.tobytes() for c in vd[:17].T}) == W                                                       # no two columns alike
    assert len(set(ds.tolist())) == 17 and len(set(qs.tolist())) == 17
    assert all(int(qs[337 + r]) != int(ds[17 + r]) for r in range(6))
    Z = f6w.maxima(qc, qs, dc, ds, np.arange(N_ROWS + 1))
    two = lambda t, r: 2.0 ** (int(qs[t]) + int(ds[r]) - 254)
    assert Z[320, 0] == -14400 * two(320, 0) and Z[321, 0] == 14400 * two(321, 0)
    for r, want in enumerate([0.125 * 0.5, -0.125 * 0.5, 7.5 * -0.5, 4.0 * 6.0]):                              # 5760 - 5760 + the third block
        assert Z[337 + r, 17 + r] == want * two(337 + r, 17 + r), r
    assert Z[341, 21] == -3.0 * two(341, 21) and Z[342, 22] == 15.0 * two(342, 22)                        # -2880 + 2877; 2880 - 2865
    kk = np.arange(W)                                                                                      # a one-hot token reads ITS column
    vq = f6.GRID[kk % 31 + 1] * np.where(kk & 1, -1.0, 1.0)
    np.testing.assert_array_equal(Z[:W], np.ldexp(vq[:, None] * vd.T, qs[:W, None].astype(int) + ds[None, :].astype(int) - 254))
    lens = [1] * N_ROWS + [N_ROWS]
    codes, scales = np.concatenate([dc, dc]), np.concatenate([ds, ds])
    idx, off = _index_of_codes(amd, codes, scales, lens)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for q_off in (np.arange(N_TOK + 1, dtype=np.int32), np.array([0, N_TOK], dtype=np.int32)):
        max_q = int(np.diff(q_off).max())
        got = amd.fp4_wide_scores_from_codes(t(qc), t(qs), t(q_off), max_q, idx, query_code="e2m3").cpu().numpy()
        want = f6w.scores(qc, qs, q_off, codes, scales, off)
        if len(q_off) == N_TOK + 1:
            np.testing.assert_array_equal(want[:, :N_ROWS], Z)                              # the one-row pages ARE the Z matrix
        dev = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        print(f"{len(q_off) - 1} queries: {len(bad)} of {got.size} scores differ, largest deviation {dev:g}")
        assert not len(bad), (f"{len(q_off) - 1} queries: {len(bad)} scores differ, first (query, page) {bad[:8].tolist()}: got "
                              f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}; largest deviation {dev:g} "
                              f"(largest |score| {np.abs(want).max():g})")


# ---------------------------------------------------------------------------------------------------------------------- encode
def encode_rows(dtype):
    """raw 16-bit rows: random rows of many magnitudes (119: the last 32-row block of the launch is partial) with the host file's
    edge rows written over the first ones and a row whose maximum sits only in the third K block"""
    g = torch.Generator().manual_seed(1)
    lens = [0, 1, 15, 16, 17, 33, 37]
    raw = wt.raw_bits(torch.cat([_scaled(g, n, dtype) for n in lens])).copy()
    edge = host.edge_rows()[0] if dtype == torch.bfloat16 else host.edge_rows_f16()
    raw[20:20 + len(edge)] = edge
    raw[50, :256] = 0                                                # nothing but the third block
    return raw


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encode_is_bit_equal_to_the_truth(amd, dtype):
    raw = encode_rows(dtype)
    assert len(raw) == 119 and len(raw) % 32
    want_c, want_s = f6w.encode(raw, dtype == torch.float16)
    assert not want_c[50, :192].any() and want_c[50, 192:].any()
    blob = torch.from_numpy(raw.view(np.int16)).view(dtype)
    qc, qs = amd.fp6_wide_quantize_queries(_packed(amd, [blob[:33], blob[33:34], blob[34:119]]))
    assert qc.shape == (119, 240) and qc.dtype == torch.uint8 and qs.shape == (119,) and qs.dtype == torch.uint8
    np.testing.assert_array_equal(qs.cpu().numpy(), want_s)
    np.testing.assert_array_equal(qc.cpu().numpy(), want_c)
    qc2, qs2 = amd.fp6_wide_quantize_queries([blob[36:60], blob[60:119]], DEV)      # a host list is packed first
    assert torch.equal(qc2, qc[36:]) and torch.equal(qs2, qs[36:])
    for n in (1, 31, 32, 33):                                        # row counts around the 32 rows of a workgroup
        c, s = amd.fp6_wide_quantize_queries(_packed(amd, [blob[20:20 + n]]))
        np.testing.assert_array_equal(c.cpu().numpy(), want_c[20:20 + n])
        np.testing.assert_array_equal(s.cpu().numpy(), want_s[20:20 + n])


# ---------------------------------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module")
def edges(amd):
    """tests/test_gpu_fp4_wide.py's: the page lengths round the 16-row chunk, an empty page among them and two more at the end,
    clamp0 on a random half"""
    g = torch.Generator().manual_seed(2)
    lens = list(PAGE_LENS) + [0, 0]
    pages = [_scaled(g, n) for n in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    clamp0 = (torch.rand(len(lens), generator=g) < 0.5).to(torch.uint8)
    corpus.clamp0 = clamp0.to(DEV)
    idx = amd.Fp4WideIndex.build(corpus)
    codes, scales = wt.encode(wt.raw_bits(torch.cat(pages)))
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
    """60 000 pages of 0-3 rows (one 16-row chunk closes several pages, empty ones among them), the last three empty, clamp0 on a
    random half: one wave scores a range of 8 or more pages"""
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


@pytest.mark.parametrize("name", ["gw1-group", "gw1-passes2", "gw2-groups", "gw2-passes3", "gw4-wide"])
def test_ranges_of_zero_to_three_row_pages(amd, tiny_pages, name):
    idx, codes, scales, off, clamp0 = tiny_pages
    qlens, gw, _ = BATCHES[name]
    plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
    assert plan[:3] == (NT, gw, D) and plan[3] >= 8, plan
    g = torch.Generator().manual_seed(40 + sum(qlens))
    _check(amd, _packed(amd, [_scaled(g, n) for n in qlens]), idx, codes, scales, off, clamp0)


@pytest.mark.parametrize("n_pages", [63, 64, 65, 130])
@pytest.mark.parametrize("name", ["gw1-group", "gw4-wide"])
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
    """Enough 0-3 row pages that one query group's waves take the full 63 pages each: 65 pages past a whole number of waves, so the
    last ranges are a full one and a short one."""
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
    """The shapes of the parity tests above, by the form msim_f4w_scores_plan names for them (it describes both query codes): every
    (NT, GW, D) the dispatcher instantiates, each with 1, 2 and 3 passes, and page ranges of 1, of 8 or more and
    (test_full_ranges_of_63_pages) of the full 63."""
    forms, passes, ranges = set(), set(), set()
    for idx, codes in ((edges[0], edges[1]), (tiny_pages[0], tiny_pages[1])):
        for qlens, gw, n_pass in BATCHES.values():
            plan = _plan(amd, len(qlens), max(qlens), len(idx), len(codes))
            assert plan[1] == gw and _passes(max(qlens)) == n_pass
            forms.add(plan[:3])
            passes.add((plan[1], n_pass))
            ranges.add(1 if plan[3] == 1 else 8 if plan[3] >= 8 else 0)
    assert forms == ALL_FORMS, (forms, ALL_FORMS)
    assert passes >= {(gw, p) for gw in (1, 2, 4) for p in (1, 2, 3)}
    assert ranges == {1, 8}


# ------------------------------------------------------------------------------------------------------- the all-negative tier
@pytest.mark.parametrize("name,n_pages", [("gw1-group", 12), ("gw4-wide", 12), ("gw1-passes2", 12), ("gw1-group", 60000), ("gw2-groups", 60000)])
def test_rows_past_a_range_never_score(amd, name, n_pages):
    """Every similarity is negative, so ONE zero row -- what the descriptors return past a range's end -- that reached a maximum
    would raise it to 0 and change the score: asserted on the truth, with a margin, before the device's output is read."""
    qlens = [n for n in BATCHES[name][0] if n]
    rng = np.random.default_rng(8)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)
    assert _plan(amd, len(qlens), max(qlens), n_pages, int(lens.sum()))[3] == ppw and (ppw == 1) == (n_pages == 12)
    qs, codes, scales, _ = tw.far_side(7, qlens, lens, planted=False)
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    M = f6w.maxima(qc, qsc, codes, scales, off)
    assert (M < -MARGIN).all()                                       # a leaked zero row would have changed every maximum
    np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(q, idx)), wt.sum_tokens(M, q.offsets_host.numpy(), off).view(np.int32))


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
    qs, codes, scales, rows = tw.far_side(9, qlens, lens, planted=True)
    assert all(r == (0 if c % 2 == 0 else lens[c] - 1) for c, r in enumerate(rows))
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    M = f6w.maxima(qc, qsc, codes, scales, off)
    won = f6w.maxima(qc, qsc, codes[off[:-1] + np.asarray(rows)], scales[off[:-1] + np.asarray(rows)], np.arange(n_pages + 1))
    assert (M > MARGIN).all() and np.array_equal(M, won)             # the planted row wins every token of every page
    np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(q, idx)), wt.sum_tokens(M, q.offsets_host.numpy(), off).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------- placement
def test_permuting_the_pages_permutes_the_bits(amd, edges):
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(11)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    base = amd.fp6_wide_scores(q, idx)
    perm = np.random.default_rng(12).permutation(len(lens))
    p_codes = np.concatenate([codes[off[c]:off[c + 1]] for c in perm])
    p_scales = np.concatenate([scales[off[c]:off[c + 1]] for c in perm])
    p_idx, _ = _index_of_codes(amd, p_codes, p_scales, np.asarray(lens)[perm], clamp0[perm])
    np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(q, p_idx)), _bits(base)[:, perm])


def test_scores_do_not_depend_on_the_batch(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(13)
    lens = torch.randint(1, 40, (300,), generator=g).tolist()
    qs = [_unit(g, n) for n in lens]
    full = amd.fp6_wide_scores(_packed(amd, qs), idx)                          # GW 4
    for i in (0, 1, 157, 299):
        np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(_packed(amd, [qs[i]]), idx)[0]), _bits(full[i]))     # GW 1
    np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(_packed(amd, qs[:3]), idx)), _bits(full[:3]))
    long_q = [_unit(g, 300), qs[7]]                                            # beside a query of several passes: GW 2
    np.testing.assert_array_equal(_bits(amd.fp6_wide_scores(_packed(amd, long_q), idx)[1]), _bits(full[7]))
    again = amd.fp6_wide_scores(_packed(amd, qs), idx)
    np.testing.assert_array_equal(_bits(again), _bits(full))


# -------------------------------------------------------------------------------------------------------------- broken offsets
def test_broken_device_offsets_come_back_as_nan_over_that_range_only(amd, edges):
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(14)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17)])
    assert _plan(amd, 3, 32, len(idx), len(codes))[3] == 1               # one page per range: a broken offset spoils its two pages
    want = _truth(q, codes, scales, off, clamp0)
    for j, bad_value in ((5, len(codes) + 7), (9, -1)):
        bad = torch.from_numpy(off.copy())
        bad[j] = bad_value
        broken = amd.Fp4WideIndex(idx.codes, idx.scales, bad.to(DEV), idx.clamp0, idx.lengths)
        got = amd.fp6_wide_scores(q, broken).cpu().numpy()
        assert np.isnan(got[:, [j - 1, j]]).all()
        keep = [c for c in range(len(lens)) if c not in (j - 1, j)]
        np.testing.assert_array_equal(got[:, keep].view(np.int32), want[:, keep].view(np.int32))
    # a query whose offsets leave the token count: NaN over that query only (an empty page stays -inf)
    qc, qs = amd.fp6_wide_quantize_queries(q)
    q_bad = q.offsets.clone()
    q_bad[2] = int(q.tokens.shape[0]) + 3
    got = amd.fp4_wide_scores_from_codes(qc, qs, q_bad, 32, idx, query_code="e2m3").cpu().numpy()
    rows = [c for c, n in enumerate(lens) if n]
    assert np.isnan(got[1:, rows]).all()
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


# --------------------------------------------------------------------------------------------------------------------- hipGraph
def test_a_captured_fp6_wide_scores_replays_the_eager_bits(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(18)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.fp6_wide_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.fp6_wide_scores(q, idx, out=out)                             # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.fp6_wide_scores(q, idx, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(first))


# ------------------------------------------------------------------------------------------------------------------- one index
def test_one_index_serves_both_query_codes(amd, edges):
    """The Fp4WideIndex is untouched by e2m3 scoring, fp4_wide_scores keeps its bits on it, and the two codes differ."""
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(22)
    q = _packed(amd, [_scaled(g, n) for n in (32, 5, 17, 64, 1)])
    before = {name: getattr(idx, name).clone() for name in ("codes", "scales", "offsets", "clamp0")}
    ptrs = {name: getattr(idx, name).data_ptr() for name in before}
    s4 = amd.fp4_wide_scores(q, idx).clone()
    np.testing.assert_array_equal(_bits(s4), tw._truth(q, codes, scales, off, clamp0).view(np.int32))
    s6 = amd.fp6_wide_scores(q, idx).clone()
    cand = torch.arange(len(lens), dtype=torch.int64, device=DEV).expand(5, len(lens)).contiguous()
    l6, _ = amd.fp6_wide_rerank_scores(q, idx, cand)
    torch.cuda.synchronize()
    for name, t in before.items():
        assert torch.equal(getattr(idx, name), t) and getattr(idx, name).data_ptr() == ptrs[name], name
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, idx)), _bits(s4))
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, idx, query_code="e2m3")), _bits(s6))
    np.testing.assert_array_equal(_bits(l6), _bits(s6))
    rows = [c for c, n in enumerate(lens) if n]
    assert not np.array_equal(_bits(s6)[:, rows], _bits(s4)[:, rows])


def test_error_paths(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(19)
    narrow = amd.Fp4Index.build(amd.pack_passages([torch.nn.functional.normalize(torch.randn(4, 128, generator=g), dim=-1).to(torch.bfloat16)],
                                                  DEV, batch_size=None))
    q128 = _packed(amd, [torch.randn(4, 128).to(torch.bfloat16)])
    with pytest.raises(NotImplementedError, match=r"queries of width 320 .*width 128\).*Fp4Index / fp6_scores"):
        amd.fp6_wide_scores(q128, idx)
    with pytest.raises(NotImplementedError, match=r"queries of width 320 .*width 128\).*Fp4Index / fp6_scores"):
        amd.fp6_wide_rerank_scores(q128, idx, torch.zeros((1, 2), dtype=torch.int64, device=DEV))
    q = _packed(amd, [_unit(g, 5)])
    with pytest.raises(TypeError, match=r"takes an Fp4WideIndex \(got Fp4Index\).*fp6_scores"):
        amd.fp6_wide_scores(q, narrow)
    with pytest.raises(NotImplementedError, match="an Fp4Index of a 128-wide shard takes fp6_rerank_scores"):
        amd.fp6_wide_rerank_scores(q, narrow, torch.zeros((1, 2), dtype=torch.int64, device=DEV))
    with pytest.raises(NotImplementedError, match="the fp4 index takes bfloat16 / float16 queries of width 128"):
        amd.fp6_scores(q, narrow)                                    # the 128-wide function keeps refusing 320-wide queries
    with pytest.raises(ValueError, match="out must be"):
        amd.fp6_wide_scores(q, idx, out=torch.empty(3, 5, device=DEV))
