"""The 320-wide FP4 index on the MI355X (msim_f4w_*, colpali_amd.Fp4WideIndex / fp4_wide_scores, search(prefilter=<Fp4WideIndex>)).

Codes and scores are checked bit for bit against the numpy restatement in tests/fp4_wide_truth.py: the codes come from integer /
fp32 logic, every per-token maximum is exactly representable in fp32 (the truth asserts it) and the score's fp32 order is
documented, so nothing here has a tolerance.  The first test settles, on hand-made data, what the kernel rests on beyond the facts
of the 128-wide index: the map of a 160-byte row onto three K blocks of v_mfma_scale_f32_16x16x128_f8f6f4 (the third half empty)
and that the instruction adds its C operand unscaled and exactly, so the three blocks may be chained through it.  The shapes are the
kernel's edges: rows around the 16-row chunk, pages of 0-3 rows so that one chunk closes several pages, page ranges of 1, 8-16 and
63 pages, queries around the 16-token tile and past one wave's NT tiles, and every launch form the dispatcher can choose.
"""
import numpy as np
import pytest
import torch

from tests import fp4_wide_truth as wt
from tests import helpers

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 320
PAGE_LENS = (1, 15, 16, 17, 31, 32, 33, 47, 64, 100, 0)
QUERY_LENS = (0, 1, 15, 16, 17, 32, 33, 127, 128, 129, 300)
NT, D = 4, 4                                                # the shipped form
P1 = 16 * NT                                                # the longest query of one pass
ALL_FORMS = {(NT, 1, D), (NT, 2, D), (NT, 4, D)}            # every (NT, GW, D) msim_f4w_scores instantiates

# query batches by the launch form they reach: name -> (query lengths, GW, passes)
BATCHES = {
    "gw1-one": ([15], 1, 1),
    "gw1-group": ([32, 17, 1, 5][:NT // 2], 1, 1),
    "gw1-passes2": ([P1 + 1], 1, 2),
    "gw1-passes3": ([2 * P1 + 1], 1, 3),
    "gw2-groups": ([32] * (NT - 1), 2, 1),
    "gw2-passes2": ([P1 + 1, 40], 2, 2),
    "gw2-passes3": ([2 * P1 + 1, P1 + 1], 2, 3),
    "gw4-tiles": ([0, 1, 16, 17, 32, 33, P1 - 1, P1], 4, 1),
    "gw4-passes2": ([2 * P1, 3, 20, 40], 4, 2),
    "gw4-passes3": ([3 * P1, 16, 5], 4, 3),
    "gw4-all": (list(QUERY_LENS), 4, -(-((300 + 15) // 16) // NT)),
    "gw4-wide": ([17, 32, 1, 0, 16, 33, 5], 4, 1),
}


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, W, generator=g), dim=-1).to(dtype)


def _scaled(g, n, dtype=torch.bfloat16):
    """unit rows times a power of two per row (2^-5 .. 2^5): the rows' scale bytes differ inside every chunk"""
    return (_unit(g, n, torch.float32) * torch.exp2(torch.randint(-5, 6, (n, 1), generator=g).float())).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _plan(amd, n_q, max_q, n_d, d_rows):
    """(NT, GW, D, pages per wave range) of msim_f4w_scores for a shape"""
    plan = torch.zeros(4, dtype=torch.int32)
    assert amd._lib.lib().msim_f4w_scores_plan(n_q, max_q, n_d, d_rows, plan.data_ptr()) == 0
    return tuple(plan.tolist())


def _passes(max_q):
    tiles = (max_q + 15) // 16
    return max(1, (tiles + NT - 1) // NT)


def _random_codes(rng, rows, lo=-12, hi=12):
    """random nibbles (never the -0 nibble 8, which the encoder does not write) and random scale bytes 127 + lo .. 127 + hi"""
    nib = rng.integers(0, 16, (rows, W), dtype=np.uint8)
    nib[nib == 8] = 0
    return wt.pack_nibbles(nib), (127 + rng.integers(lo, hi + 1, rows)).astype(np.uint8)


def _index_of_codes(amd, codes, scales, lens, clamp0=None, id_base=0):
    """an Fp4WideIndex straight from host codes uint8 [rows, 160], scales uint8 [rows] and page lengths"""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c0 = None if clamp0 is None else torch.from_numpy(np.asarray(clamp0, dtype=np.uint8)).to(DEV)
    return amd.Fp4WideIndex(torch.from_numpy(codes).to(DEV), torch.from_numpy(scales).to(DEV), torch.from_numpy(off).to(DEV), c0,
                            torch.from_numpy(np.asarray(lens, dtype=np.int64)), id_base), off


def _q_codes(q):
    return wt.encode(wt.raw_bits(q.tokens.cpu()), f16=q.tokens.dtype == torch.float16)


def _truth(q, codes, scales, off, clamp0=None):
    """the truth scores of packed queries `q` (coded by the truth) against host codes"""
    qc, qs = _q_codes(q)
    return wt.scores(qc, qs, q.offsets_host.numpy(), codes, scales, off, clamp0)


def _check(amd, q, idx, codes, scales, off, clamp0=None):
    got = amd.fp4_wide_scores(q, idx)
    want = _truth(q, codes, scales, off, clamp0)
    np.testing.assert_array_equal(_bits(got), want.view(np.int32))
    return got, want


# ------------------------------------------------------------------------------------------------------- the hardware's facts
VALUES15 = [1, 2, 3, 4, 5, 6, 7, 9, 10, 11, 12, 13, 14, 15]            # the 14 non-zero nibbles; 0 is the fifteenth value


def exact_data():
    """Hand-made codes.  Rows (21): row 0 all +6; rows 1 .. 16 random nibbles; rows 17 .. 20 the cancelling rows -- K block 0 all +6,
    block 1 all -6, block 2 one small value (and the same with the signs of blocks 0 and 1 swapped).  Tokens (341): 320 one-hot
    tokens, token k holding one non-zero nibble at dimension k (the 14 non-zero nibbles in turn); then token 320 all -6 (against
    row 0: I = -11 520), 16 random ones, and four that meet the cancelling rows: +6 over blocks 0 and 1 and 0.5 (or 6) at the
    row's small value.  Exponents -8 .. 8 on both sides, the cancelling ones away from 0."""
    rng = np.random.default_rng(4)
    d_nib = rng.integers(0, 16, (21, W), dtype=np.uint8)
    q_nib = np.zeros((341, W), dtype=np.uint8)
    q_nib[np.arange(W), np.arange(W)] = np.asarray(VALUES15, dtype=np.uint8)[np.arange(W) % 14]
    q_nib[320:337] = rng.integers(0, 16, (17, W), dtype=np.uint8)
    d_nib[d_nib == 8], q_nib[q_nib == 8] = 0, 0
    d_nib[0], q_nib[320] = 7, 15
    for r, (s0, s1, k2, v2) in enumerate([(7, 15, 256, 1), (15, 7, 319, 1), (7, 15, 300, 9), (15, 7, 257, 7)]):
        d_nib[17 + r] = 0
        d_nib[17 + r, :128], d_nib[17 + r, 128:256], d_nib[17 + r, k2] = s0, s1, v2
        q_nib[337 + r] = 0
        q_nib[337 + r, :256], q_nib[337 + r, k2] = 7, (1 if r < 2 else 7)
    ds = (127 + (np.arange(21) * 5) % 17 - 8).astype(np.uint8)
    qs = (127 + (np.arange(341) * 7 + 3) % 17 - 8).astype(np.uint8)
    ds[17:21] = [127 + 3, 127 - 5, 127 + 8, 127 - 8]
    qs[337:341] = [127 - 7, 127 + 6, 127 + 8, 127 - 8]
    return wt.pack_nibbles(d_nib), ds, wt.pack_nibbles(q_nib), qs, d_nib, q_nib


def test_exact_data_settles_the_block_map_and_the_chained_c_operand(amd):
    """Every Z_ij bit for bit: each of the 21 rows as a page of its own against each of the 341 tokens as a query of its own (a
    one-token score is 0 + M), then the 21 rows as ONE page (16 + 5 rows: a full chunk and a masked one) against the one-token
    queries and against all tokens as one query (several passes).  A nibble of any K block that is dropped or lands on another
    dimension -- block 2's empty half included -- changes a one-hot token's Z, since no two columns of the rows are alike; a C
    operand that is scaled again or rounded changes the cancelling rows, whose first two block sums are +-4608 and whose answer is
    the third block's 0.25 .. 36 times a power of two away from 1."""
    dc, ds, qc, qs, d_nib, q_nib = exact_data()
    assert set(np.unique(d_nib)) == set(range(16)) - {8} and set(np.unique(q_nib)) == set(range(16)) - {8}   # all 15 values
    assert len({d_nib[:, k].tobytes() for k in range(W)}) == W                                                 # no two columns alike
    assert set(ds.tolist()) >= set(range(119, 136)) and set(qs.tolist()) >= set(range(119, 136))              # exponents -8 .. 8
    lens = [1] * 21 + [21]
    codes, scales = np.concatenate([dc, dc]), np.concatenate([ds, ds])
    Z = wt.maxima(qc, qs, dc, ds, np.arange(22))
    assert Z[320, 0] == -11520 * 2.0 ** (int(qs[320]) + int(ds[0]) - 254)
    for r, want in enumerate([0.25, 0.25, -3.0, 36.0]):                                                        # 4608 - 4608 + the third block
        assert Z[337 + r, 17 + r] == want * 2.0 ** (int(qs[337 + r]) + int(ds[17 + r]) - 254)
    onehot = Z[:W, :17].astype(np.float64) / np.ldexp(wt.decode(qc)[np.arange(W), np.arange(W)], qs[:W].astype(np.int64) - 127)[:, None]
    assert len({row.tobytes() for row in onehot}) == W                       # a misplaced dimension shows in the Z of its token
    idx, off = _index_of_codes(amd, codes, scales, lens)
    t = lambda a: torch.from_numpy(a).to(DEV)
    for q_off in (np.arange(342, dtype=np.int32), np.array([0, 341], dtype=np.int32)):
        max_q = int(np.diff(q_off).max())
        got = amd.fp4_wide_scores_from_codes(t(qc), t(qs), t(q_off), max_q, idx).cpu().numpy()
        want = wt.scores(qc, qs, q_off, codes, scales, off)
        if len(q_off) == 342:
            np.testing.assert_array_equal(want[:, :21], Z)                                  # the one-row pages ARE the Z matrix
        dev = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
        bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
        assert not len(bad), (f"{len(q_off) - 1} queries: {len(bad)} scores differ, first (query, page) {bad[0].tolist()}: got "
                              f"{got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}; largest deviation {dev:g} "
                              f"(largest |score| {np.abs(want).max():g})")


# ---------------------------------------------------------------------------------------------------------------------- encode
def encode_rows(dtype):
    """raw 16-bit rows for the encode test: random rows of many magnitudes, every tie, exact and one-ulp-above maxima, zero rows,
    subnormals, rows whose maximum sits only in the third K block and (bf16 only: f16 cannot reach them) both exponent clamps"""
    g = torch.Generator().manual_seed(1)
    lens = [0, 1, 15, 16, 17, 33, 37]                                # 119 rows: the last 32-row block of the launch is partial
    rows = torch.cat([_scaled(g, n, dtype) for n in lens])
    raw = wt.raw_bits(rows).copy()
    one = lambda v: int(wt.raw_bits(torch.tensor([[v]], dtype=dtype))[0, 0])
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    raw[2] = 0
    raw[2, :15] = [one(6.0)] + [one(v) for v in ties] + [one(-v) for v in ties]       # e = 0: every tie, both signs
    raw[3] = 0
    raw[3, 300:315] = [one(6.0 * 2.0 ** -9)] + [one(v * 2.0 ** -9) for v in ties] + [one(-v * 2.0 ** -9) for v in ties]
    raw[4] = 0                                                       # a row of +0.0
    raw[5] = 0x8000                                                  # a row of -0.0
    raw[6, 7] = one(6.0 * 2.0 ** 3)                                  # the maximum exactly 6 * 2^3 ...
    raw[6, :7] &= 0x7fff
    raw[7] = raw[6]
    raw[7, 7] += 1                                                   # ... and one ulp above
    raw[8] = 0
    raw[8, 0], raw[8, 319] = 0x0001, 0x8001                          # subnormals only
    raw[9] = 0
    raw[9, 3], raw[9, 260] = 0x03ff, one(2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126)   # the largest f16 subnormal / bf16 one
    raw[13, 319] = one(-6.0 * 2.0 ** 4)                              # the maximum in the row's last dimension only ...
    raw[14, 256] = one(6.0 * 2.0 ** 4 * 1.0078125)                   # ... and in the third block's first, one step above 6 * 2^4
    raw[15, :256] = 0
    raw[15, 280] = one(3.0)                                          # nothing but the third block
    if dtype == torch.bfloat16:
        raw[10] = 0
        raw[10, 0], raw[10, 1], raw[10, 290] = one(2.0 ** -31), one(-(2.0 ** -34)), one(2.0 ** -33)    # e clamps at -32
        raw[11, 0], raw[11, 301] = one(-(2.0 ** 40)), one(2.0 ** 33)                                  # e clamps at +32
        raw[12, 5] = one(6.0 * 2.0 ** 32)
    else:
        raw[10, 300] = 0x7bff                                        # 65504
        raw[11, 0] = 0xfbff
    return raw, lens


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_encode_is_bit_equal_to_the_truth(amd, dtype):
    raw, lens = encode_rows(dtype)
    f16 = dtype == torch.float16
    want_c, want_s = wt.encode(raw, f16)
    assert want_s[4] == 127 and want_s[5] == 127 and not want_c[4:6].any()
    assert want_s[6] == 130 and want_s[7] == 131 and want_s[13] == 131 and want_s[14] == 132
    assert not want_c[15, :128].any() and want_c[15, 128:].any()
    if not f16:
        assert want_s[8] == 95 and want_s[10] == 95 and want_s[11] == 159 and want_s[12] == 159
    blob = torch.from_numpy(raw.view(np.int16)).view(dtype)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    corpus = amd.PackedCorpus(blob=blob.to(DEV), offsets=torch.from_numpy(off).to(DEV),
                              clamp0=torch.tensor([1, 0, 0, 1, 0, 0, 1], dtype=torch.uint8, device=DEV),
                              lengths=torch.tensor(lens, dtype=torch.int64), id_base=11)
    idx = amd.Fp4WideIndex.build(corpus)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.scales.cpu().numpy(), want_s)
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), want_c)
    assert len(idx) == len(corpus) and idx.device == DEV and idx.id_base == 11
    assert idx.nbytes == 119 * 161 + 8 * 4 + 7
    assert torch.equal(idx.offsets, corpus.offsets) and idx.offsets.data_ptr() != corpus.offsets.data_ptr()
    assert torch.equal(idx.clamp0, corpus.clamp0) and idx.clamp0.data_ptr() != corpus.clamp0.data_ptr()
    # the query side is the same code
    qc, qs = amd.fp4_wide_quantize_queries(_packed(amd, [blob[:33], blob[33:119]]))
    np.testing.assert_array_equal(qc.cpu().numpy(), want_c)
    np.testing.assert_array_equal(qs.cpu().numpy(), want_s)


# ---------------------------------------------------------------------------------------------------------------------- scores
@pytest.fixture(scope="module")
def edges(amd):
    """The page lengths round the 16-row chunk, an empty page among them and two more at the end, clamp0 on a random half: built
    through Fp4WideIndex.build from a bf16 corpus whose rows have many magnitudes."""
    g = torch.Generator().manual_seed(2)
    lens = list(PAGE_LENS) + [0, 0]
    pages = [_scaled(g, n) for n in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    clamp0 = (torch.rand(len(lens), generator=g) < 0.5).to(torch.uint8)
    corpus.clamp0 = clamp0.to(DEV)
    idx = amd.Fp4WideIndex.build(corpus)
    codes, scales = wt.encode(wt.raw_bits(torch.cat(pages)))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), codes)
    np.testing.assert_array_equal(idx.scales.cpu().numpy(), scales)
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
    random half; the codes are random, so the index is made from them directly.  One wave scores a range of 8 or more pages."""
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
    """The shapes of the parity tests above, by the form msim_f4w_scores_plan names for them: every (NT, GW, D) the dispatcher
    instantiates, each with 1, 2 and 3 passes, and page ranges of 1, of 8 or more and (test_full_ranges_of_63_pages) of the full 63."""
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
MARGIN = 0.05                   # every similarity of the far-side case is far below this in size: tests/helpers.py puts rows 0.7 u apart


def _ragged_range_lens(rng, n, ppw):
    """page lengths of which no wave range of `ppw` pages (a wave's row stream) ends on a 16-row chunk boundary"""
    lens = rng.choice(np.array([1, 2, 3, 5, 17] if n <= 64 else [1, 2, 3]), n)          # many pages: short ones, a small case
    for p0 in range(0, n, ppw):
        if lens[p0:p0 + ppw].sum() % 16 == 0:
            lens[min(p0 + ppw, n) - 1] += 1
    assert all(lens[p0:p0 + ppw].sum() % 16 for p0 in range(0, n, ppw))
    return lens


def far_side(seed, qlens, lens, planted):
    """the far-side case of tests/helpers.py as codes: (query blocks, page codes, scales, planted row per page)"""
    qs, ps, rows = helpers.far_side_case(seed, qlens, [int(n) for n in lens], W, torch.bfloat16, planted=planted)
    codes, scales = wt.encode(wt.raw_bits(torch.cat(ps)))
    return qs, codes, scales, rows


@pytest.mark.parametrize("name,n_pages", [("gw1-group", 12), ("gw4-wide", 12), ("gw1-passes2", 12), ("gw1-group", 60000), ("gw2-groups", 60000)])
def test_rows_past_a_range_never_score(amd, name, n_pages):
    """Every similarity is negative, so ONE zero row -- what the descriptors return past a range's end -- that reached a maximum
    would raise it to 0 and change the score: asserted on the truth, with a margin, before the device's output is read."""
    qlens = [n for n in BATCHES[name][0] if n]
    rng = np.random.default_rng(8)
    ppw = _plan(amd, len(qlens), max(qlens), n_pages, 2 * n_pages)[3]
    lens = _ragged_range_lens(rng, n_pages, ppw)
    assert _plan(amd, len(qlens), max(qlens), n_pages, int(lens.sum()))[3] == ppw and (ppw == 1) == (n_pages == 12)
    qs, codes, scales, _ = far_side(7, qlens, lens, planted=False)
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    M = wt.maxima(qc, qsc, codes, scales, off)
    assert (M < -MARGIN).all()                                       # a leaked zero row would have changed every maximum
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, idx)), wt.sum_tokens(M, q.offsets_host.numpy(), off).view(np.int32))


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
    qs, codes, scales, rows = far_side(9, qlens, lens, planted=True)
    assert all(r == (0 if c % 2 == 0 else lens[c] - 1) for c, r in enumerate(rows))
    q = _packed(amd, qs)
    idx, off = _index_of_codes(amd, codes, scales, lens)
    qc, qsc = _q_codes(q)
    M = wt.maxima(qc, qsc, codes, scales, off)
    won = wt.maxima(qc, qsc, codes[off[:-1] + np.asarray(rows)], scales[off[:-1] + np.asarray(rows)], np.arange(n_pages + 1))
    assert (M > MARGIN).all() and np.array_equal(M, won)             # the planted row wins every token of every page
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, idx)), wt.sum_tokens(M, q.offsets_host.numpy(), off).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------- placement
def test_permuting_the_pages_permutes_the_bits(amd, edges):
    idx, codes, scales, off, clamp0, lens = edges
    g = torch.Generator().manual_seed(11)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    base = amd.fp4_wide_scores(q, idx)
    perm = np.random.default_rng(12).permutation(len(lens))
    p_codes = np.concatenate([codes[off[c]:off[c + 1]] for c in perm])
    p_scales = np.concatenate([scales[off[c]:off[c + 1]] for c in perm])
    p_idx, _ = _index_of_codes(amd, p_codes, p_scales, np.asarray(lens)[perm], clamp0[perm])
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, p_idx)), _bits(base)[:, perm])


def test_scores_do_not_depend_on_the_batch(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(13)
    lens = torch.randint(1, 40, (300,), generator=g).tolist()
    qs = [_unit(g, n) for n in lens]
    full = amd.fp4_wide_scores(_packed(amd, qs), idx)                          # GW 4
    for i in (0, 1, 157, 299):
        np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(_packed(amd, [qs[i]]), idx)[0]), _bits(full[i]))     # GW 1
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(_packed(amd, qs[:3]), idx)), _bits(full[:3]))
    long_q = [_unit(g, 300), qs[7]]                                            # beside a query of several passes: GW 2
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(_packed(amd, long_q), idx)[1]), _bits(full[7]))
    again = amd.fp4_wide_scores(_packed(amd, qs), idx)
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
        got = amd.fp4_wide_scores(q, broken).cpu().numpy()
        assert np.isnan(got[:, [j - 1, j]]).all()
        keep = [c for c in range(len(lens)) if c not in (j - 1, j)]
        np.testing.assert_array_equal(got[:, keep].view(np.int32), want[:, keep].view(np.int32))
    # a query whose offsets leave the token count: NaN over that query only (an empty page stays -inf)
    qc, qs = amd.fp4_wide_quantize_queries(q)
    q_bad = q.offsets.clone()
    q_bad[2] = int(q.tokens.shape[0]) + 3
    got = amd.fp4_wide_scores_from_codes(qc, qs, q_bad, 32, idx).cpu().numpy()
    rows = [c for c, n in enumerate(lens) if n]
    assert np.isnan(got[1:, rows]).all()
    np.testing.assert_array_equal(got[0].view(np.int32), want[0].view(np.int32))


# ------------------------------------------------------------------------------------------------------------ two-stage search
SEARCH_SEED = 20
K, M_CAND = 5, 64


def search_case(seed=SEARCH_SEED):
    """300 pages of 20-60 unit rows and 6 planted queries: noisy copies of rows of one page each"""
    g = torch.Generator().manual_seed(seed)
    pages = [_unit(g, int(n)) for n in torch.randint(20, 61, (300,), generator=g)]
    qs = []
    for i, n in enumerate((5, 16, 17, 32, 33, 9)):
        src = pages[37 * i + 11].float()
        rows = src[torch.randint(0, src.shape[0], (n,), generator=g)]
        qs.append(torch.nn.functional.normalize(rows + 0.05 * torch.randn(n, W, generator=g), dim=-1).to(torch.bfloat16))
    return pages, qs


def exact_scores(qs, rows, off):
    """float64 MaxSim [n_q, n] of bf16 query blocks against rows float [R, 320] of pages with offsets off (no empty page)"""
    out = np.zeros((len(qs), len(off) - 1))
    for i, q in enumerate(qs):
        S = q.double().numpy() @ rows.T
        out[i] = np.maximum.reduceat(S, off[:-1], axis=1).sum(axis=0)
    return out


def fp4_ranks(qs, pages, off, allowed=None):
    """the truth's FP4 score matrix as ranks: rank[q, c] = pages (allowed ones) that (score desc, id asc) puts before page c"""
    S = wt.score_blocks([wt.raw_bits(q) for q in qs], wt.raw_bits(torch.cat(pages)), off).astype(np.float64)
    if allowed is not None:
        S = np.where(allowed[None, :], S, -np.inf)
    order = np.argsort(-S, axis=1, kind="stable")
    ranks = np.empty_like(order)
    for i in range(len(qs)):
        ranks[i, order[i]] = np.arange(S.shape[1])
    return ranks


def worst_rank(exact, ranks, k=K, allowed=None):
    """the worst FP4 rank of a page of the exact top-k (among the allowed pages)"""
    E = exact if allowed is None else np.where(allowed[None, :], exact, -np.inf)
    top = np.argsort(-E, axis=1, kind="stable")[:, :k]
    return int(np.take_along_axis(ranks, top, axis=1).max())


@pytest.fixture(scope="module")
def search(amd):
    pages, qs = search_case()
    off = np.concatenate([[0], np.cumsum([len(p) for p in pages])])
    exact = exact_scores(qs, torch.cat(pages).double().numpy(), off)
    ranks = fp4_ranks(qs, pages, off)
    assert worst_rank(exact, ranks) <= 24                            # the precondition, on the truth alone, with margin to 64
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=100)
    return corpus, amd.Fp4WideIndex.build(corpus), _packed(amd, qs), pages, qs, off, exact


def test_two_stage_search_returns_the_exact_search(amd, search):
    corpus, idx, q, pages, qs, off, exact = search
    r = amd.ShardedRetriever(corpus)
    es, ei = r.search(q, k=K)
    s, i = r.search(q, k=K, prefilter=idx, n_candidates=M_CAND)
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    assert (ei[:, 0].cpu() - 100).tolist() == [37 * j + 11 for j in range(6)]       # the planted pages come first
    _, cand = amd.topk(amd.fp4_wide_scores(q, idx), M_CAND, idx.id_base)            # stage 1 is fp4_wide_scores: (score desc, id asc)
    want = np.argsort(-_truth(q, *wt.encode(wt.raw_bits(torch.cat(pages))), off).astype(np.float64), axis=1, kind="stable")[:, :M_CAND]
    np.testing.assert_array_equal(cand.cpu().numpy() - 100, want)


def test_two_stage_search_with_a_filter_and_with_groups(amd, search):
    corpus, idx, q, pages, qs, off, exact = search
    n = len(corpus)
    g = torch.Generator().manual_seed(16)
    allowed = torch.rand(n, generator=g) < 0.5
    assert worst_rank(exact, fp4_ranks(qs, pages, off, allowed.numpy()), allowed=allowed.numpy()) < M_CAND
    r = amd.ShardedRetriever(corpus)
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
    ranks = fp4_ranks(qs, pages, off)
    assert np.take_along_axis(ranks, np.take_along_axis(best, top_docs, axis=1), axis=1).max() < M_CAND
    groups = amd.PageGroups.from_labels(labels.to(DEV), 100)
    es, eg, ep = r.search(q, k=K, group_by=groups)
    gs, gg, gp = r.search(q, k=K, prefilter=idx, n_candidates=M_CAND, group_by=groups)
    np.testing.assert_array_equal(gg.cpu().numpy(), eg.cpu().numpy())
    np.testing.assert_array_equal(gp.cpu().numpy(), ep.cpu().numpy())
    np.testing.assert_array_equal(_bits(gs), _bits(es))


# --------------------------------------------------------------------------------------------------------------------- hipGraph
def test_a_captured_fp4_wide_scores_replays_the_eager_bits(amd, edges):
    idx = edges[0]
    g = torch.Generator().manual_seed(18)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.fp4_wide_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.fp4_wide_scores(q, idx, out=out)                             # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.fp4_wide_scores(q, idx, out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(out), _bits(first))


# ------------------------------------------------------------------------------------------------------------------ persistence
def test_save_and_load_round_trip_and_a_flipped_scale_byte(amd, edges, tmp_path):
    idx = edges[0]
    g = torch.Generator().manual_seed(20)
    q = _packed(amd, [_unit(g, n) for n in (32, 5)])
    base = amd.fp4_wide_scores(q, idx)
    path = tmp_path / "fp4w.msim"
    idx.save(path, chunk_bytes=4096)
    assert amd.verify_file(path)["kind"] == "Fp4WideIndex"
    back = amd.Fp4WideIndex.load(path, DEV)
    for name in ("codes", "scales", "offsets", "clamp0"):
        assert torch.equal(getattr(back, name), getattr(idx, name)), name
    assert torch.equal(back.lengths, idx.lengths) and back.id_base == idx.id_base
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, back)), _bits(base))
    lo, hi = 3, 9
    part = amd.load(path, DEV, pages=(lo, hi))
    assert isinstance(part, amd.Fp4WideIndex) and len(part) == hi - lo and part.id_base == idx.id_base + lo
    np.testing.assert_array_equal(_bits(amd.fp4_wide_scores(q, part)), _bits(base)[:, lo:hi])
    entry = next(e for e in amd.verify_file(path)["tensors"] if e["name"] == "scales")
    with open(path, "r+b") as f:
        f.seek(entry["offset"] + 40)
        b = f.read(1)
        f.seek(entry["offset"] + 40)
        f.write(bytes([b[0] ^ 0x10]))
    with pytest.raises(amd.ShardFileError, match=r"scales.*chunk 0"):
        amd.Fp4WideIndex.load(path, DEV)


def test_error_paths(amd, search):
    corpus, idx, q = search[:3]
    g = torch.Generator().manual_seed(19)
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 pages of width 320"):
        amd.Fp4WideIndex.build(amd.pack_passages([torch.randn(4, W)], DEV, batch_size=None))
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 pages of width 320.*Fp4Index"):
        amd.Fp4WideIndex.build(amd.pack_passages([torch.randn(4, 128).to(torch.bfloat16)], DEV, batch_size=None))
    with pytest.raises(NotImplementedError, match="the wide fp4 index takes bfloat16 / float16 queries of width 320"):
        amd.fp4_wide_scores(_packed(amd, [torch.randn(4, 128).to(torch.bfloat16)]), idx)
    with pytest.raises(NotImplementedError, match="the fp4 index takes bfloat16 / float16 pages of width 128"):
        amd.Fp4Index.build(corpus)                                   # the 128-wide class keeps refusing this shard
    other = amd.Fp4WideIndex.build(amd.pack_passages([_unit(g, 7) for _ in range(5)], DEV, batch_size=None))
    with pytest.raises(ValueError, match="same documents"):
        amd.ShardedRetriever(corpus).search(q, prefilter=other, n_candidates=3)
    with pytest.raises(ValueError, match="out must be"):
        amd.fp4_wide_scores(q, idx, out=torch.empty(3, 5, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- large offsets
def test_an_index_whose_codes_pass_2_to_the_32_bytes(amd):
    """One coded block of 60 pages (tests/helpers.py: the large-offset block, 10 067 rows) written T times back to back until the code
    tensor passes 2^32 bytes.  MaxSim of a page does not depend on where the page lies, so every tile must carry tile 0's bits, and
    tile 0 must equal the CPU truth of the block; a failure names the first tile that differs and where its rows start."""
    free, _ = torch.cuda.mem_get_info(DEV)
    assert free > (6 << 30), f"this test needs 6 GB of free device memory, the device reports {free / 2**30:.1f} GB"
    lens = helpers.large_block_lens()
    R0, P = int(sum(lens)), len(lens)
    T = 2**32 // (wt.ROW_BYTES * R0) + 2                             # at least one whole tile past byte 2^32
    g = torch.Generator().manual_seed(1001)
    block = torch.nn.functional.normalize(torch.randn(R0, W, generator=g), dim=-1).to(torch.bfloat16)
    bc, bs = wt.encode(wt.raw_bits(block))
    codes = torch.empty((T * R0, wt.ROW_BYTES), dtype=torch.uint8, device=DEV)
    codes.view(T, R0, wt.ROW_BYTES).copy_(torch.from_numpy(bc).to(DEV).unsqueeze(0).expand(T, R0, wt.ROW_BYTES))
    scales = torch.from_numpy(bs).to(DEV).repeat(T)
    assert codes.numel() > 2**32 and T * R0 < 2**31
    boff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    off = np.concatenate([(boff[None, :-1] + (np.arange(T, dtype=np.int64) * R0)[:, None]).reshape(-1), [T * R0]])
    idx = amd.Fp4WideIndex(codes, scales, torch.from_numpy(off.astype(np.int32)).to(DEV), None,
                           torch.from_numpy(np.tile(np.asarray(lens, dtype=np.int64), T)))
    qg = torch.Generator().manual_seed(21)
    q = _packed(amd, [_unit(qg, n) for n in (32, 5, 17)])
    out = torch.full((3, T * P), float("nan"), dtype=torch.float32, device=DEV)
    got = amd.fp4_wide_scores(q, idx, out=out)
    torch.cuda.synchronize()
    want = _truth(q, bc, bs, boff)
    np.testing.assert_array_equal(_bits(got[:, :P]), want.view(np.int32))
    same = (got.view(torch.int32).view(3, T, P) == got[:, :P].contiguous().view(torch.int32).unsqueeze(1)).all(dim=2).all(dim=0).cpu().numpy()
    bounds = {name: nbytes // wt.ROW_BYTES // R0 for name, nbytes in (("byte 2^31", 2**31), ("byte 2^32", 2**32))}
    assert all(t + 1 < T for t in bounds.values())
    bad = np.flatnonzero(~same)
    assert not len(bad), (f"{len(bad)} of {T} tiles differ from tile 0; the first is tile {int(bad[0])}, whose codes start at byte "
                          f"{int(bad[0]) * R0 * wt.ROW_BYTES} (the tiles that hold the boundaries: {bounds})")
    for name, t in bounds.items():                                   # around the boundaries, element by element
        for tt in (t - 1, t, t + 1):
            np.testing.assert_array_equal(_bits(got[:, tt * P:(tt + 1) * P]), want.view(np.int32), err_msg=f"tile {tt}, at {name}")
