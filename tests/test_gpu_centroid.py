"""The centroid-code index on the MI355X (msim_cent_*, colpali_amd.CentroidIndex / centroid_scores / train_centroids,
search(prefilter=<CentroidIndex>)) against the float64 restatement in tests/centroid_truth.py.

Codes must be float64 near-arg-maxima (exact where a row is a copy of a centroid); scores are compared with the float64 sum of
maxima over the index's OWN codes within sum_i (2^-12 + 128 * 2^-24 * sum_k |q_ik C_k|) + Lq * 2^-24 * |score| (the fp16 rounding of
a table entry below 1, the fp32 chain, the fp32 token sum); everything the contract calls bit-stable is compared bit for bit.
"""
import numpy as np
import pytest
import torch

from tests import centroid_truth as ct

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LENS = (0, 1, 15, 16, 17, 63, 64, 65, 300)
Q_LENS = (0, 1, 31, 32, 33, 64, 128)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _unit(g, n, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _np(t):
    return t.detach().float().cpu().numpy()


def _packed(amd, q_blocks):
    return amd.pack_queries(list(q_blocks), DEV, layout="flat", compact=False)


def _q_off(qs):
    return np.cumsum([0] + [len(q) for q in qs])


def _index(amd, C, codes, lens, clamp0=None):
    """An index straight from codes (numpy) and page lengths."""
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    c0 = None if clamp0 is None else torch.from_numpy(np.asarray(clamp0, np.uint8)).to(DEV)
    return amd.CentroidIndex(C.to(DEV), torch.from_numpy(np.asarray(codes, np.uint16)).to(DEV), torch.from_numpy(off).to(DEV), c0,
                             torch.from_numpy(np.asarray(lens, np.int64)))


def _check_scores(got, qs, C, idx, label=""):
    """got fp32 [n_q, n] against the float64 truth over the index's own codes, within the documented tolerance."""
    q_rows = np.concatenate([_np(q) for q in qs]) if len(qs) else np.zeros((0, 128))
    codes, off = idx.codes.cpu().numpy(), idx.offsets.cpu().numpy()
    c0 = None if idx.clamp0 is None else idx.clamp0.cpu().numpy()
    want = ct.scores64(q_rows, _np(C), _q_off(qs), codes, off, c0)
    tol = ct.score_tolerance(q_rows, _np(C), _q_off(qs), want)
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
    planted = [0, K - 1, 15, 16, 17, 31, 32, K // 2 - 1, K // 2, K - 16, K - 17, dup_lo, dup_hi]
    where = []
    for j, k in enumerate(planted):
        p = [i for i, n in enumerate(lens) if n >= 15][j]
        r = (j * 7) % lens[p]
        pages[p][r] = C[k]
        where.append((p, r, k))
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    idx = amd.CentroidIndex.build(corpus, centroids=C.to(DEV), chunk_docs=7)
    again = amd.CentroidIndex.build(corpus, centroids=C.to(DEV))
    torch.cuda.synchronize()
    codes = idx.codes.cpu().numpy()
    assert codes.dtype == np.uint16 and codes.shape == (sum(lens),) and int(codes.max()) < K
    np.testing.assert_array_equal(codes, again.codes.cpu().numpy())   # the chunking changes nothing; a rebuild gives the same bits
    assert len(idx) == 40 and idx.device == DEV and idx.n_centroids == K and idx.nbytes >= 2 * sum(lens) + 256 * K
    assert torch.equal(idx.offsets, corpus.offsets) and idx.offsets.data_ptr() != corpus.offsets.data_ptr()
    rows = _np(corpus.blob)
    sim = ct.sims64(rows, _np(C))
    chosen = sim[np.arange(len(codes)), codes.astype(np.int64)]
    assert (chosen >= sim.max(axis=1) - ct.encode_slack(rows, _np(C))).all()
    off = corpus.offsets.cpu().numpy()
    for p, r, k in where:
        assert codes[off[p] + r] == (dup_lo if k == dup_hi else k), (p, r, k)
    assert not (codes == dup_hi).any()                                 # an equal similarity never names the higher id


# ------------------------------------------------------------------------------------------------------------------ 2. scores
def _ragged_lens(n_pages, seed):
    rng = np.random.default_rng(seed)
    return rng.choice(np.array([0, 0, 1, 2, 3, 5, 7, 15, 16, 17, 31, 64, 65]), n_pages)


@pytest.fixture(scope="module")
def ragged(amd):
    """12 000 short ragged pages (about 200 k rows) and the ragged query batch, shared by the score tests."""
    g = torch.Generator().manual_seed(21)
    lens = _ragged_lens(12000, 21)
    rows = _unit(g, int(lens.sum()))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    clamp0 = (np.random.default_rng(22).random(len(lens)) < 0.2).astype(np.uint8)
    corpus = amd.PackedCorpus(blob=rows.to(DEV), offsets=torch.from_numpy(off).to(DEV), clamp0=torch.from_numpy(clamp0).to(DEV),
                              lengths=torch.from_numpy(lens.astype(np.int64)))
    qs = [_unit(g, n) for n in Q_LENS]
    return corpus, qs


@pytest.mark.parametrize("K", [256, 1024, 2048])
def test_scores_match_the_truth_over_the_index_codes(amd, ragged, K):
    from colpali_amd import centroid

    corpus, qs = ragged
    g = torch.Generator().manual_seed(K + 1)
    C = _unit(g, K)
    idx = amd.CentroidIndex.build(corpus, centroids=C.to(DEV))
    q = _packed(amd, qs)
    nb, ppw, waves, wgs = centroid.scores_plan(q, idx)
    assert nb == 4 and ppw > 16 and waves == 8                         # several parked batches per wave, four table blocks
    assert wgs == len(qs) * -(-len(idx) // (ppw * waves)) and wgs > len(qs)
    got = amd.centroid_scores(q, idx)
    assert got.shape == (len(qs), len(idx)) and got.dtype == torch.float32
    want, _ = _check_scores(got, qs, C, idx, f"K={K} ragged")
    nz = corpus.lengths.numpy() > 0
    assert (got[0].cpu().numpy()[nz] == 0).all()                       # the query of 0 tokens
    # a small problem: one page per wave, fewer workgroups than CUs
    small = amd.PackedCorpus(blob=corpus.blob[:int(corpus.offsets[301])], offsets=corpus.offsets[:302].clone(),
                             clamp0=corpus.clamp0[:301].clone(), lengths=corpus.lengths[:301].clone())
    sidx = amd.CentroidIndex.build(small, centroids=C.to(DEV))
    assert centroid.scores_plan(q, sidx)[1] == 1
    sgot = amd.centroid_scores(q, sidx)
    np.testing.assert_array_equal(_bits(sgot), _bits(got[:, :301]))    # the launch plan does not touch a score's bits


# ------------------------------------------------------------------------------------------------------------------ 3. sign tier
def _negative_setup(g, K, n_q=5):
    pos = lambda n: torch.nn.functional.normalize(torch.rand(n, 128, generator=g) + 0.1, dim=-1)
    C = pos(K).to(torch.bfloat16)
    qs = [(-pos(n)).to(torch.bfloat16) for n in (32, 1, 33, 128, 17)[:n_q]]
    return C, qs


def test_sign_tier_all_table_entries_negative(amd):
    K = 256
    g = torch.Generator().manual_seed(31)
    C, qs = _negative_setup(g, K)
    S64 = ct.sims64(np.concatenate([_np(q) for q in qs]), _np(C))
    assert S64.max() <= -0.05                                           # the precondition, before any output is read
    rng = np.random.default_rng(32)
    lens = np.array([LENS[i % len(LENS)] for i in range(90)])
    codes = rng.integers(0, K, int(lens.sum())).astype(np.uint16)
    flags = (rng.random(len(lens)) < 0.5).astype(np.uint8)
    plain = _index(amd, C, codes, lens)
    flagged = _index(amd, C, codes, lens, flags)
    q = _packed(amd, qs)
    got = amd.centroid_scores(q, plain)
    want, tol = _check_scores(got, qs, C, plain, "sign tier")
    live = lens > 0
    assert (want[:, live] <= -0.05).all() and (got.cpu().numpy()[:, live] < 0).all()
    got_f = amd.centroid_scores(q, flagged).cpu().numpy()
    on = flags.astype(bool)
    assert (got_f[:, on & live] == 0).all() and not np.signbit(got_f[:, on & live]).any()      # exactly +0
    np.testing.assert_array_equal(got_f[:, ~on].view(np.int32), _bits(got)[:, ~on])          # unflagged pages keep their bits
    assert (on & ~live).any() and (~on & ~live).any()
    assert np.isneginf(got_f[:, ~live]).all() and np.isneginf(got.cpu().numpy()[:, ~live]).all()   # a 0-row page: -inf either way


@pytest.mark.parametrize("pos", [0, 63, 64, 255, 256, 299], ids=lambda p: f"row{p}")
def test_sign_tier_planted_winner(amd, pos):
    """One row of a 300-row page names the only centroid with positive entries: first row, last row, both sides of the 64-lane and of
    the 4-step (256-row) boundaries."""
    K = 256
    g = torch.Generator().manual_seed(33)
    C, qs = _negative_setup(g, K, n_q=3)
    winner = 200
    C[winner] = -C[winner]
    S64 = ct.sims64(np.concatenate([_np(q) for q in qs]), _np(C))
    assert np.delete(S64, winner, axis=1).max() <= -0.05 and S64[:, winner].min() >= 0.05
    rng = np.random.default_rng(34)
    lens = np.array([5, 300, 0, 300, 64])
    codes = rng.integers(0, winner, int(lens.sum())).astype(np.uint16)
    codes[5 + pos] = winner                                            # page 1 only
    for flags in (None, np.array([1, 1, 1, 1, 0], np.uint8)):
        idx = _index(amd, C, codes, lens, flags)
        got = amd.centroid_scores(_packed(amd, qs), idx)
        want, _ = _check_scores(got, qs, C, idx, f"planted winner at row {pos}, clamp0 {flags is not None}")
        res = got.cpu().numpy()
        assert (res[:, 1] > 0).all() and (want[:, 1] > 0).all()
        if flags is None:
            assert (res[:, [0, 3, 4]] < 0).all()
        else:
            assert (res[:, [0, 3]] == 0).all() and (res[:, 4] < 0).all()


# ------------------------------------------------------------------------------------------------------------------ 4. bit identities
def test_bit_identities(amd):
    K = 1024
    g = torch.Generator().manual_seed(41)
    C = _unit(g, K).to(DEV)
    lens = [LENS[i % len(LENS)] for i in range(50)]
    pages = [_unit(g, n) for n in lens]
    flags = [i % 3 == 0 for i in range(50)]
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    corpus.clamp0 = torch.tensor(flags, dtype=torch.uint8, device=DEV)
    idx = amd.CentroidIndex.build(corpus, centroids=C)
    qs = [_unit(g, n) for n in (32, 5, 128, 64, 1, 33, 97)]
    q = _packed(amd, qs)
    first = amd.centroid_scores(q, idx).clone()
    np.testing.assert_array_equal(_bits(amd.centroid_scores(q, idx)), _bits(first))                    # a rerun
    out = torch.full_like(first, 7.0)
    assert amd.centroid_scores(q, idx, out=out) is out
    np.testing.assert_array_equal(_bits(out), _bits(first))                                            # out=
    for i in (0, 2, 6):                                                                                # alone vs in a batch of 7
        np.testing.assert_array_equal(_bits(amd.centroid_scores(_packed(amd, [qs[i]]), idx)[0]), _bits(first[i]))
    perm = torch.randperm(50, generator=g).tolist()                                                    # pages permuted
    pcorpus = amd.pack_passages([pages[j] for j in perm], DEV, batch_size=None)
    pcorpus.clamp0 = torch.tensor([flags[j] for j in perm], dtype=torch.uint8, device=DEV)
    pidx = amd.CentroidIndex.build(pcorpus, centroids=C)
    np.testing.assert_array_equal(_bits(amd.centroid_scores(q, pidx)), _bits(first)[:, perm])
    dense = torch.stack([qs[0], qs[0].flip(0)]).to(DEV)                                                # a dense device tensor is packed here
    np.testing.assert_array_equal(_bits(amd.centroid_scores(dense, idx)[0]), _bits(first[0]))


# ------------------------------------------------------------------------------------------------------------------ 5. broken index
def test_a_code_outside_the_table_scores_nan(amd):
    K = 256
    g = torch.Generator().manual_seed(51)
    C = _unit(g, K)
    rng = np.random.default_rng(52)
    lens = np.array([20, 300, 0, 7, 64, 130])
    codes = rng.integers(0, K, int(lens.sum())).astype(np.uint16)
    qs = [_unit(g, n) for n in (32, 40, 3)]
    q = _packed(amd, qs)
    good = amd.centroid_scores(q, _index(amd, C, codes, lens))
    for page, row, bad in ((1, 299, K), (1, 64, 65535), (5, 0, K), (3, 6, 2048)):
        broken = codes.copy()
        broken[int(lens[:page].sum()) + row] = bad
        got = amd.centroid_scores(q, _index(amd, C, broken, lens))
        torch.cuda.synchronize()
        res = got.cpu().numpy()
        assert np.isnan(res[:, page]).all(), (page, row, bad)
        others = [c for c in range(len(lens)) if c != page]
        np.testing.assert_array_equal(_bits(got)[:, others], _bits(good)[:, others])


# ------------------------------------------------------------------------------------------------------------------ 6. two-stage search
def _exact_model(seed):
    """300 pages x 64 rows, every row an exact copy of one of 256 unit centroids; 8 queries x 32 tokens."""
    g = torch.Generator().manual_seed(seed)
    C = _unit(g, 256)
    pick = torch.randint(0, 256, (300, 64), generator=g)
    pages = [C[pick[p]] for p in range(300)]
    qs = [_unit(g, 32) for _ in range(8)]
    return C, pick, pages, qs


def test_two_stage_search_is_exact_where_the_model_is_exact(amd):
    k, m = 10, 40
    C, pick, pages, qs = _exact_model(61)
    q_rows = np.concatenate([_np(x) for x in qs])
    off = np.arange(301) * 64
    want = ct.scores64(q_rows, _np(C), _q_off(qs), pick.reshape(-1).numpy(), off)             # = the exact MaxSim of these pages
    tol = ct.score_tolerance(q_rows, _np(C), _q_off(qs), want)
    ranked = -np.sort(-want, axis=1)
    assert ((ranked[:, k - 1] - ranked[:, m]) > 2 * tol.max(axis=1)).all()                     # the precondition (seed chosen on the CPU)
    corpus = amd.pack_passages(pages, DEV, batch_size=None)
    idx = amd.CentroidIndex.build(corpus, centroids=C.to(DEV))
    np.testing.assert_array_equal(idx.codes.cpu().numpy(), pick.reshape(-1).numpy().astype(np.uint16))
    q = _packed(amd, qs)
    r = amd.ShardedRetriever(corpus)
    es, ei = r.search(q, k=k)
    s, i = r.search(q, k=k, prefilter=idx, n_candidates=m)
    np.testing.assert_array_equal(i.cpu().numpy(), ei.cpu().numpy())
    np.testing.assert_array_equal(_bits(s), _bits(es))
    _, cand = amd.topk(amd.centroid_scores(q, idx), m)                  # search's stage 1 is centroid_scores + the library's top-k
    rs, ri = amd.rerank(q, corpus, cand, k=k)
    np.testing.assert_array_equal(ri.cpu().numpy(), i.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ 7. training
def test_training_improves_the_objective(amd):
    g = torch.Generator().manual_seed(71)
    K = 256
    dirs = torch.nn.functional.normalize(torch.randn(64, 128, generator=g), dim=-1)
    rows = torch.nn.functional.normalize(dirs[torch.randint(0, 64, (8192,), generator=g)] + 0.3 * torch.randn(8192, 128, generator=g) / 11.3,
                                         dim=-1).to(torch.bfloat16)
    lens = [64] * 128
    corpus = amd.pack_passages(list(rows.split(64)), DEV, batch_size=None)
    rows64 = _np(corpus.blob)
    obj = {}
    for iters in (0, 1, 4):
        C = amd.train_centroids(corpus, K, iters, 1 << 18, 3)
        assert C.shape == (K, 128) and C.dtype == torch.bfloat16 and C.device == DEV and C.is_contiguous()
        norms = np.linalg.norm(C.double().cpu().numpy(), axis=1)
        assert (np.abs(norms - 1) <= 2.0**-8).all()                      # unit rows within bf16 rounding
        obj[iters] = float(ct.sims64(rows64, _np(C)).max(axis=1).mean())
    print("objective by iterations:", obj)
    assert obj[1] >= obj[0] - 2.0**-8 and obj[4] >= obj[1] - 2.0**-8     # rounding each centroid to bf16 once may cost 2^-8
    assert obj[4] > obj[0]
    a, b = amd.train_centroids(corpus, K, 0, 1 << 18, 3), amd.train_centroids(corpus, K, 0, 1 << 18, 3)
    assert torch.equal(a, b) and not torch.equal(a, amd.train_centroids(corpus, K, 0, 1 << 18, 4))
    src = {bytes(r) for r in corpus.blob.cpu().view(torch.int16).numpy()}
    assert all(bytes(r) in src for r in a.cpu().view(torch.int16).numpy())                     # iters=0: sampled rows
    idx = amd.CentroidIndex.build(corpus, n_centroids=K, iters=2, seed=3)                      # centroids=None trains first
    assert idx.n_centroids == K and len(idx) == len(lens)


# ------------------------------------------------------------------------------------------------------------------ 8. capture
def test_graph_replay_is_bit_identical(amd):
    K = 512
    g = torch.Generator().manual_seed(81)
    C = _unit(g, K).to(DEV)
    corpus = amd.pack_passages([_unit(g, n) for n in (100, 3, 256, 0, 31, 64)], DEV, batch_size=None)
    idx = amd.CentroidIndex.build(corpus, centroids=C)
    q = _packed(amd, [_unit(g, n) for n in (32, 5, 17, 64, 1)])
    first = amd.centroid_scores(q, idx).clone()
    out = torch.empty_like(first)
    amd.centroid_scores(q, idx, out=out)                                # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.centroid_scores(q, idx, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(out), _bits(first))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(amd):
    g = torch.Generator().manual_seed(91)
    C = _unit(g, 256).to(DEV)
    with pytest.raises(NotImplementedError):
        amd.CentroidIndex.build(amd.pack_passages([torch.randn(4, 128)], DEV, batch_size=None), centroids=C)
    with pytest.raises(NotImplementedError):
        amd.CentroidIndex.build(amd.pack_passages([torch.randn(4, 320).to(torch.bfloat16)], DEV, batch_size=None), centroids=C)
    corpus = amd.pack_passages([_unit(g, 300), _unit(g, 20)], DEV, batch_size=None)
    for k in (128, 300, 4096):
        with pytest.raises(ValueError):
            amd.CentroidIndex.build(corpus, n_centroids=k)
    with pytest.raises(ValueError):
        amd.CentroidIndex.build(corpus, centroids=C.to(torch.float16))   # not the corpus dtype
    idx = amd.CentroidIndex.build(corpus, centroids=C)
    with pytest.raises(NotImplementedError):
        amd.centroid_scores(_packed(amd, [_unit(g, 129)]), idx)
    with pytest.raises(NotImplementedError):
        amd.centroid_scores([torch.randn(4, 128)], idx)
    with pytest.raises(ValueError):
        amd.centroid_scores(_packed(amd, [_unit(g, 4)]), idx, out=torch.empty(1, 3, device=DEV))
    other = amd.CentroidIndex.build(amd.pack_passages([_unit(g, 5)], DEV, batch_size=None), centroids=C)
    with pytest.raises(ValueError, match="same documents"):
        amd.ShardedRetriever(corpus).search(_packed(amd, [_unit(g, 4)]), prefilter=other, n_candidates=1)
