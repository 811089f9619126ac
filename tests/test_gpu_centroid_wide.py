"""The centroid-code index at width 320 on the MI355X (msim_cent_wide_*, colpali_amd.CentroidWideIndex, centroid_wide_scores and the
two-stage search behind it), against tests/residual_wide_truth.py.

Shapes: pages of 0 .. 300 rows (every tail class of the 16-row tile and of the 128-row encode block), at most 40 pages; queries of
0 .. 128 tokens (every table-block boundary); K = 256 and 2048; bf16 and f16."""
import numpy as np
import pytest
import torch

from tests import residual_wide_truth as wt

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 320
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300]
Q_LENS = [0, 1, 16, 17, 32, 33, 128]


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()      # must load: no fallback
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, W, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _np(t):
    return t.detach().float().cpu().numpy()


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _q_off(qs):
    return np.cumsum([0] + [len(q) for q in qs])


def _index(amd, C, codes, lens, clamp0=None):
    """An index straight from codes (numpy) and page lengths."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c0 = None if clamp0 is None else torch.from_numpy(np.asarray(clamp0, np.uint8)).to(DEV)
    codes = torch.from_numpy(np.asarray(codes, np.uint16).view(np.int16)).to(DEV).view(torch.uint16)
    return amd.CentroidWideIndex(C.to(DEV), codes, torch.from_numpy(off).to(DEV), c0, torch.from_numpy(np.asarray(lens, np.int64)))


def _check_scores(got, qs, C, idx, label=""):
    """got fp32 [n_q, n] against the float64 truth over the index's own codes, within the documented tolerance."""
    q_rows = np.concatenate([_np(q) for q in qs]) if len(qs) else np.zeros((0, W))
    codes, off = _u16(idx.codes), idx.offsets.cpu().numpy()
    c0 = None if idx.clamp0 is None else idx.clamp0.cpu().numpy()
    want = wt.scores64(q_rows, _np(C), _q_off(qs), codes, off, c0)
    tol = wt.score_tolerance(q_rows, _np(C), _q_off(qs), want)
    got = got.cpu().numpy().astype(np.float64)
    empty = off[1:] == off[:-1]
    assert np.isneginf(got[:, empty]).all() and np.isfinite(got[:, ~empty]).all(), label
    err = np.abs(got[:, ~empty] - want[:, ~empty])
    worst = float((err / np.maximum(tol[:, ~empty], 1e-300)).max()) if err.size else 0.0
    print(f"{label}: max |err| {float(err.max()) if err.size else 0:.3e}, worst err / tol {worst:.3f}")
    assert (err <= tol[:, ~empty]).all(), (label, worst)
    return want, tol


# ------------------------------------------------------------------------------------------------------------------ 1. encode
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", [256, 2048])
def test_codes_are_near_argmax_and_planted_rows_exact(amd, K, dtype):
    g = torch.Generator().manual_seed(K)
    C = _unit(g, K, dtype)
    dup_lo, dup_hi = 37, K - 100
    C[dup_hi] = C[dup_lo]                                             # two equal centroids: the lower id must win
    lens = [LENS[i % len(LENS)] for i in range(40)]
    pages = [_unit(g, n, dtype) * (0.5 + 0.1 * i) for i, n in enumerate(lens)]
    # planted rows: exact copies of centroids at the ends, around the 16-centroid streaming tiles and the duplicate pair
    planted = [0, 15, 16, 17, 31, 32, K // 2 - 1, K // 2, K - 17, K - 16, K - 1, dup_lo, dup_hi]
    where = []
    for j, k in enumerate(planted):
        p = [i for i, n in enumerate(lens) if n >= 15][j]
        r = (j * 7) % lens[p]
        pages[p][r] = C[k]
        where.append((p, r, k))
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    idx = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV), chunk_docs=7)
    again = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV))
    torch.cuda.synchronize()
    codes = _u16(idx.codes)
    assert codes.shape == (sum(lens),) and int(codes.max()) < K
    np.testing.assert_array_equal(codes, _u16(again.codes))           # the chunking changes nothing; a rebuild gives the same bits
    assert len(idx) == 40 and idx.device == DEV and idx.n_centroids == K and idx.nbytes >= 2 * sum(lens) + 640 * K
    assert torch.equal(idx.offsets, corpus.offsets) and idx.offsets.data_ptr() != corpus.offsets.data_ptr()
    rows = _np(corpus.blob)[:sum(lens)]
    sim = wt.sims64(rows, _np(C))
    chosen = sim[np.arange(len(codes)), codes.astype(np.int64)]
    assert (chosen >= sim.max(axis=1) - wt.encode_slack(rows, _np(C))).all()
    off = corpus.offsets.cpu().numpy()
    for p, r, k in where:
        assert codes[off[p] + r] == (dup_lo if k == dup_hi else k), (p, r, k)
    assert not (codes == dup_hi).any()                                 # an equal similarity never names the higher id


# ------------------------------------------------------------------------------------------------------------------ 2. scores
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
@pytest.mark.parametrize("K", [256, 2048])
def test_scores_match_the_truth_over_the_index_codes(amd, K, dtype):
    g = torch.Generator().manual_seed(K + 1)
    C = _unit(g, K, dtype)
    lens = [LENS[(5 * i) % len(LENS)] for i in range(40)]
    corpus = amd.pack_passages([_unit(g, n, dtype) for n in lens], DEV, batch_size=None, id_base=11)
    clamp0 = (np.random.default_rng(22).random(len(lens)) < 0.3).astype(np.uint8)
    corpus.clamp0 = torch.from_numpy(clamp0).to(DEV)
    assert clamp0.any() and not clamp0.all()
    idx = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV))
    qs = [_unit(g, n, dtype) for n in Q_LENS]
    q = _packed(amd, qs)
    got = amd.centroid_wide_scores(q, idx)
    assert got.shape == (len(qs), len(idx)) and got.dtype == torch.float32
    _check_scores(got, qs, C, idx, f"K={K} {dtype}")
    nz = np.array(lens) > 0
    assert (got[0].cpu().numpy()[nz] == 0).all()                       # the query of 0 tokens
    # rerun, out= and a host list: the same bits
    np.testing.assert_array_equal(_bits(amd.centroid_wide_scores(q, idx)), _bits(got))
    out = torch.full_like(got, 7.0)
    assert amd.centroid_wide_scores(q, idx, out=out) is out
    np.testing.assert_array_equal(_bits(out), _bits(got))
    np.testing.assert_array_equal(_bits(amd.centroid_wide_scores(qs, idx)), _bits(got))


# ------------------------------------------------------------------------------------------------------------------ 3. sign tier
def _negative_setup(g, K, n_q=5):
    pos = lambda n: torch.nn.functional.normalize(torch.rand(n, W, generator=g) + 0.1, dim=-1)
    C = pos(K).to(torch.bfloat16)
    qs = [(-pos(n)).to(torch.bfloat16) for n in (32, 1, 33, 128, 17)[:n_q]]
    return C, qs


def test_sign_tier_all_table_entries_negative(amd):
    K = 256
    g = torch.Generator().manual_seed(31)
    C, qs = _negative_setup(g, K)
    S64 = wt.sims64(np.concatenate([_np(q) for q in qs]), _np(C))
    assert S64.max() <= -0.05                                           # the precondition, before any output is read
    rng = np.random.default_rng(32)
    lens = np.array([LENS[i % len(LENS)] for i in range(40)])
    codes = rng.integers(0, K, int(lens.sum())).astype(np.uint16)
    flags = (rng.random(len(lens)) < 0.5).astype(np.uint8)
    plain = _index(amd, C, codes, lens)
    flagged = _index(amd, C, codes, lens, flags)
    q = _packed(amd, qs)
    got = amd.centroid_wide_scores(q, plain)
    want, tol = _check_scores(got, qs, C, plain, "sign tier")
    live = lens > 0
    assert (want[:, live] <= -0.05).all() and (got.cpu().numpy()[:, live] < 0).all()
    got_f = amd.centroid_wide_scores(q, flagged).cpu().numpy()
    on = flags.astype(bool)
    assert (got_f[:, on & live] == 0).all() and not np.signbit(got_f[:, on & live]).any()      # exactly +0
    np.testing.assert_array_equal(got_f[:, ~on].view(np.int32), _bits(got)[:, ~on])          # unflagged pages keep their bits
    assert np.isneginf(got_f[:, ~live]).all() and np.isneginf(got.cpu().numpy()[:, ~live]).all()   # a 0-row page: -inf either way


@pytest.mark.parametrize("pos", [0, 63, 64, 255, 256, 299], ids=lambda p: f"row{p}")
def test_sign_tier_planted_winner(amd, pos):
    """One row of a 300-row page names the only centroid with positive entries."""
    K = 256
    g = torch.Generator().manual_seed(33)
    C, qs = _negative_setup(g, K, n_q=3)
    winner = 200
    C[winner] = -C[winner]
    S64 = wt.sims64(np.concatenate([_np(q) for q in qs]), _np(C))
    assert np.delete(S64, winner, axis=1).max() <= -0.05 and S64[:, winner].min() >= 0.05
    rng = np.random.default_rng(34)
    lens = np.array([5, 300, 0, 300, 64])
    codes = rng.integers(0, winner, int(lens.sum())).astype(np.uint16)
    codes[5 + pos] = winner                                            # page 1 only
    for flags in (None, np.array([1, 1, 1, 1, 0], np.uint8)):
        idx = _index(amd, C, codes, lens, flags)
        got = amd.centroid_wide_scores(_packed(amd, qs), idx)
        want, _ = _check_scores(got, qs, C, idx, f"planted winner at row {pos}, clamp0 {flags is not None}")
        res = got.cpu().numpy()
        assert (res[:, 1] > 0).all() and (want[:, 1] > 0).all()
        if flags is None:
            assert (res[:, [0, 3, 4]] < 0).all()
        else:
            assert (res[:, [0, 3]] == 0).all() and (res[:, 4] < 0).all()


# ------------------------------------------------------------------------------------------------------------------ 4. broken index
def test_a_code_outside_the_table_scores_nan(amd):
    K = 256
    g = torch.Generator().manual_seed(51)
    C = _unit(g, K)
    rng = np.random.default_rng(52)
    lens = np.array([20, 300, 0, 7, 64, 130])
    codes = rng.integers(0, K, int(lens.sum())).astype(np.uint16)
    q = _packed(amd, [_unit(g, n) for n in (32, 40, 3)])
    good = amd.centroid_wide_scores(q, _index(amd, C, codes, lens))
    for page, row, bad in ((1, 299, K), (1, 64, 65535), (5, 0, K), (3, 6, 2048)):
        broken = codes.copy()
        broken[int(lens[:page].sum()) + row] = bad
        got = amd.centroid_wide_scores(q, _index(amd, C, broken, lens))
        res = got.cpu().numpy()
        assert np.isnan(res[:, page]).all(), (page, row, bad)
        others = [c for c in range(len(lens)) if c != page]
        np.testing.assert_array_equal(_bits(got)[:, others], _bits(good)[:, others])


# ------------------------------------------------------------------------------------------------------------------ 5. two-stage search
def test_two_stage_search_with_every_page_kept_is_the_exact_search(amd):
    g = torch.Generator().manual_seed(61)
    K = 256
    C = _unit(g, K)
    lens = [LENS[(7 * i) % len(LENS)] for i in range(30)]
    pages = [_unit(g, n) for n in lens]
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=5)
    idx = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV))
    qs = [_unit(g, n) for n in (1, 17, 33, 128, 40)]             # several lengths: the scan runs the kernel whose bits the rerank carries
    q = _packed(amd, qs)
    r = amd.ShardedRetriever(corpus)
    n = len(pages)
    for k in (1, 7, n):
        es, ei = r.search(q, k=k)
        s, i = r.search(q, k=k, prefilter=idx, n_candidates=n)
        live = torch.isfinite(es).cpu().numpy()                  # an empty page is -inf on both routes; its id is the scan's only
        np.testing.assert_array_equal(i.cpu().numpy()[live], ei.cpu().numpy()[live])
        np.testing.assert_array_equal(_bits(s), _bits(es))
    # the width mismatches, worded like the FdeIndex / FdeWideIndex one
    narrow = amd.pack_passages([torch.nn.functional.normalize(torch.randn(max(n_, 1), 128, generator=g), dim=-1).to(torch.bfloat16)
                                for n_ in lens], DEV, batch_size=None, id_base=5)
    C128 = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).to(torch.bfloat16).to(DEV)
    nidx = amd.CentroidIndex.build(narrow, centroids=C128)
    with pytest.raises(ValueError, match="320-wide shard takes a CentroidWideIndex"):
        r.search(q, k=3, prefilter=nidx, n_candidates=3)
    with pytest.raises(ValueError, match="320-wide shard takes a CentroidWideIndex"):
        amd.ShardedRetriever(narrow).search([x[:, :128].contiguous() for x in qs], k=3, prefilter=idx, n_candidates=3)
    # each scorer refuses the other class by its type, before any kernel runs
    with pytest.raises(NotImplementedError, match="width 320"):
        amd.centroid_scores(q, idx)
    with pytest.raises(NotImplementedError, match="width 128"):
        amd.centroid_wide_scores(q, nidx)
    with pytest.raises(NotImplementedError):
        amd.CentroidWideIndex.build(narrow, centroids=C128)
    with pytest.raises(NotImplementedError):
        amd.CentroidIndex.build(corpus, centroids=C.to(DEV))


# ------------------------------------------------------------------------------------------------------------------ 6. capture
def test_graph_replay_is_bit_identical(amd):
    K = 512
    g = torch.Generator().manual_seed(81)
    C = _unit(g, K).to(DEV)
    corpus = amd.pack_passages([_unit(g, n) for n in (100, 3, 256, 0, 31, 64)], DEV, batch_size=None)
    idx = amd.CentroidWideIndex.build(corpus, centroids=C)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.centroid_wide_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.centroid_wide_scores(q, idx, out=out)                           # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.centroid_wide_scores(q, idx, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out), _bits(first))


# ------------------------------------------------------------------------------------------------------------------ 7. training
def test_training_lowers_the_objective(amd):
    g = torch.Generator().manual_seed(71)
    K = 256
    dirs = torch.nn.functional.normalize(torch.randn(64, W, generator=g), dim=-1)
    rows = torch.nn.functional.normalize(dirs[torch.randint(0, 64, (8192,), generator=g)] + 0.3 * torch.randn(8192, W, generator=g) / 17.9,
                                         dim=-1).to(torch.bfloat16)
    corpus = amd.pack_passages(list(rows.split(64)), DEV, batch_size=None)
    rows64 = _np(corpus.blob)
    cost = {}
    for iters in (0, 1, 4):
        idx = amd.CentroidWideIndex.build(corpus, n_centroids=K, iters=iters, seed=3)
        C = idx.centroids
        assert C.shape == (K, W) and C.dtype == torch.bfloat16 and C.device == DEV and C.is_contiguous() and len(idx) == 128
        norms = np.linalg.norm(C.double().cpu().numpy(), axis=1)
        assert (np.abs(norms - 1) <= 2.0**-8).all()                      # unit rows within bf16 rounding
        cost[iters] = 1.0 - float(wt.sims64(rows64, _np(C)).max(axis=1).mean())     # the spherical k-means objective
    print("objective by iterations:", cost)
    assert cost[1] <= cost[0] + 2.0**-8 and cost[4] <= cost[1] + 2.0**-8   # rounding each centroid to bf16 once may cost 2^-8
    assert cost[4] < cost[0]
    a = amd.CentroidWideIndex.build(corpus, n_centroids=K, iters=0, seed=3).centroids
    src = {bytes(r) for r in corpus.blob.cpu().view(torch.int16).numpy()}
    assert all(bytes(r) in src for r in a.cpu().view(torch.int16).numpy())                     # iters=0: sampled rows
