"""The residual-compressed shard at width 320 on the MI355X (msim_res_wide_*, colpali_amd.ResidualWideCorpus,
residual_wide_rerank_scores, the two- and three-stage search over it, create_plaid_index(nbits=) and save / load).

The contracts: the packed residuals and the decoded rows equal tests/residual_wide_truth.py bit for bit;
residual_wide_rerank_scores(q, rc, cand) equals rerank_scores(q, rc.decompress(), cand) bit for bit; and the scores stay within the
320-wide rerank test's tolerance of the float64 MaxSim of the truth's decoded rows.  Shapes: K = 256 and 2048, 2 and 4 bits, bf16
and f16; pages of 0 .. 300 rows (every tail class of the 32-row slab, ten slabs in the longest), queries of 0 .. 128 tokens (every
unit count class boundary)."""
import numpy as np
import pytest
import torch

from tests import residual_wide_truth as wt
from tests.helpers import SIGN_MARGIN, far_side_axis, far_side_case, far_side_rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 320
PAGE_LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 300]
QUERY_LENS = [0, 1, 16, 17, 32, 33, 128]
ID_BASE = 1000
CASES = [(k, bits, dt) for k in (256, 2048) for bits in (2, 4) for dt in ("bf16", "f16")]
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
RTOL = 1e-5           # tests/test_gpu_rerank_wide.py (tests/test_gpu_parity.py: close): |got - want| <= RTOL * max(|want|, 1)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()      # must load: no fallback
    return colpali_amd


def _u16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _same(got, want):
    """(scores, ids) pairs: the same bits and the same ids"""
    np.testing.assert_array_equal(got[1].cpu().numpy(), want[1].cpu().numpy())
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))


def _codec(bits):
    """given cutoffs and weights; 0.0 is a cutoff, so a dimension that equals its centroid's sits ON one"""
    nb = 1 << bits
    cut = (torch.arange(1, nb, dtype=torch.float32) - nb // 2) * (0.04 / (nb // 2))
    edges = torch.cat([cut[:1] - 0.025, cut, cut[-1:] + 0.025])
    return cut.contiguous(), ((edges[:-1] + edges[1:]) / 2).contiguous()


_cases = {}


def _case(amd, K, bits, dt):
    """One corpus per (K, bits, dtype), built once and left unchanged: given centroids, cutoffs and weights, pages clustered round
    the centroids, one row that IS a centroid, clamp0 on a random half of the pages, id_base != 0."""
    key = (K, bits, dt)
    if key in _cases:
        return _cases[key]
    dtype = TORCH_DT[dt]
    g = torch.Generator().manual_seed(1000 * bits + K + (dt == "f16"))
    C = torch.nn.functional.normalize(torch.randn(K, W, generator=g), dim=-1).to(dtype)
    pages = []
    for n in PAGE_LENS:
        near = C[torch.randint(0, K, (n,), generator=g)].float()
        pages.append(torch.nn.functional.normalize(near + 0.022 * torch.randn(n, W, generator=g), dim=-1).to(dtype))
    pages[-1][7] = C[K // 3]
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    clamp = (torch.rand(len(pages), generator=g) < 0.5).to(torch.uint8)
    corpus.clamp0 = clamp.to(DEV)
    cutoffs, weights = _codec(bits)
    index = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV))
    rc = amd.ResidualWideCorpus.build(corpus, index=index, bits=bits, cutoffs=cutoffs.to(DEV), weights=weights.to(DEV))
    qs = [torch.nn.functional.normalize(C[torch.randint(0, K, (n,), generator=g)].float() + 0.06 * torch.randn(n, W, generator=g),
                                        dim=-1).to(dtype) for n in QUERY_LENS]
    qs[0] = torch.zeros(5, W, dtype=dtype)                         # compaction leaves a query of 0 tokens
    pq = amd.pack_queries(qs, DEV)
    assert pq.lengths.tolist() == QUERY_LENS
    rows = sum(PAGE_LENS)
    codes = _u16(rc.codes)[:rows]
    out = dict(rc=rc, corpus=corpus, pq=pq, qs=qs, pages=pages, rows=rows, clamp=clamp.numpy(), dt=dt, bits=bits, K=K,
               rows32=torch.cat(pages).float().numpy(), C32=C.float().numpy(), codes=codes, cutoffs=cutoffs.numpy(),
               weights=weights.numpy(), d_off=np.concatenate([[0], np.cumsum(PAGE_LENS)]), C=C)
    out["xhat_bits"] = wt.decode(out["C32"], codes, wt.encode(out["rows32"], out["C32"], codes, out["cutoffs"], bits), out["weights"], bits, dt)
    n = len(pages)
    out["all_ids"] = (torch.arange(n, device=DEV) + ID_BASE).expand(len(qs), n)
    out["dec"] = rc.decompress()
    out["all_scores"] = amd.residual_wide_rerank_scores(pq, rc, out["all_ids"])[0]
    _cases[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. encode
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_encode_matches_the_truth(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc = c["rc"]
    assert type(rc) is amd.ResidualWideCorpus and type(rc.index) is amd.CentroidWideIndex and rc.width == W and rc.dtype == TORCH_DT[dt]
    assert rc.residuals.shape == (max(c["rows"], 1), 40 * bits) and rc.bits == bits and len(rc) == len(PAGE_LENS) and rc.id_base == ID_BASE
    sims = wt.sims64(c["rows32"], c["C32"])
    stored = sims[np.arange(c["rows"]), c["codes"].astype(np.int64)]
    assert (stored >= sims.max(axis=1) - wt.encode_slack(c["rows32"], c["C32"])).all()
    # the residual bytes: the truth's, for the codes the kernel itself stored
    want = wt.encode(c["rows32"], c["C32"], c["codes"], c["cutoffs"], bits)
    np.testing.assert_array_equal(rc.residuals.cpu().numpy()[:c["rows"]], want)
    b = wt.unpack(want, bits)
    assert len(np.unique(b)) == 1 << bits                                   # every bucket is in use
    on_cutoff = (c["rows32"] - c["C32"][c["codes"].astype(np.int64)]) == 0.0
    assert on_cutoff.any() and (b[on_cutoff] == (1 << bits) // 2).all()     # e == 0.0 is ON a cutoff: the upper bucket
    # .index is the stage 1 over the same tensors
    assert rc.index.codes.data_ptr() == rc.codes.data_ptr() and rc.index.centroids.data_ptr() == rc.centroids.data_ptr()
    assert rc.nbytes == (K * 640 + max(c["rows"], 1) * (2 + 40 * bits) + 4 * ((2 << bits) - 1) + 4 * (len(PAGE_LENS) + 1) + len(PAGE_LENS))


# ---------------------------------------------------------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_decompress_matches_the_truth(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    dec = c["dec"]
    assert dec.blob.dtype == TORCH_DT[dt] and dec.blob.shape[1] == W and dec.id_base == ID_BASE and dec.lengths.tolist() == PAGE_LENS
    np.testing.assert_array_equal(dec.offsets.cpu().numpy(), c["d_off"])
    np.testing.assert_array_equal(dec.clamp0.cpu().numpy(), c["clamp"])
    np.testing.assert_array_equal(_u16(dec.blob)[:c["rows"]], c["xhat_bits"])
    # the codec is lossy but beats the centroid alone
    x, xh = c["rows32"].astype(np.float64), wt.from_bits(c["xhat_bits"], dt).astype(np.float64)
    cent = c["C32"][c["codes"].astype(np.int64)].astype(np.float64)
    assert ((x - xh) ** 2).sum() < ((x - cent) ** 2).sum()
    # listed local pages, in the order given, duplicates and the empty page included: the matching slices
    ids = [11, 0, 3, 10, 3, 1]
    part = c["rc"].decompress(ids)
    want = np.concatenate([c["xhat_bits"][c["d_off"][p]:c["d_off"][p + 1]] for p in ids])
    assert part.lengths.tolist() == [PAGE_LENS[p] for p in ids] and part.id_base == 0
    np.testing.assert_array_equal(part.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum([PAGE_LENS[p] for p in ids])]))
    np.testing.assert_array_equal(_u16(part.blob)[:len(want)], want)
    np.testing.assert_array_equal(part.clamp0.cpu().numpy(), c["clamp"][ids])
    one = c["rc"].decompress(torch.tensor([4]))
    np.testing.assert_array_equal(_u16(one.blob), c["xhat_bits"][c["d_off"][4]:c["d_off"][5]])
    assert len(c["rc"].decompress([])) == 0
    with pytest.raises(ValueError):
        c["rc"].decompress([len(PAGE_LENS)])


# ---------------------------------------------------------------------------------------------------------------- 3. identity
def _lists(n, n_q, seed):
    """per query: a random order of every page, then -1, an id below id_base, one past the end, one id twice in a row"""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for _ in range(n_q):
        ids = torch.randperm(n, generator=g) + ID_BASE
        extra = torch.tensor([-1, ID_BASE - 1, ID_BASE + n, int(ids[3]), int(ids[3]), 0, ID_BASE + n - 1])
        rows.append(torch.cat([ids, extra]))
    return torch.stack(rows).to(DEV)


@pytest.mark.parametrize("K,bits,dt", CASES)
def test_rerank_is_bit_identical_to_the_rerank_of_the_decompressed_pages(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, dec, pq = c["rc"], c["dec"], c["pq"]
    n, n_q = len(PAGE_LENS), len(QUERY_LENS)
    assert rc.clamp0 is not None and 0 < int(rc.clamp0.sum()) < n
    ref = amd.retrieval.rerank_scores
    cand = _lists(n, n_q, 5)
    got = amd.residual_wide_rerank_scores(pq, rc, cand)
    _same(got, ref(pq, dec, cand))
    s, i = got[0].cpu(), got[1].cpu()
    assert bool((i[:, n:n + 3] == -1).all()) and bool(torch.isinf(s[:, n:n + 3]).all()) and bool((s[:, n:n + 3] < 0).all())
    assert bool((i[:, n + 5] == -1).all())                                               # id 0 lies below id_base
    assert torch.equal(s[:, n + 3].view(torch.int32), s[:, n + 4].view(torch.int32))    # one id twice in a row: the same bits
    assert bool((s[0][i[0] >= 0] == 0).all())                                           # the 0-token query scores 0
    _same(amd.residual_wide_rerank_scores(pq, rc, cand), got)                           # a rerun: the same bits
    # the host list and the dense device box give the packed queries' bits
    _same(amd.residual_wide_rerank_scores(c["qs"], rc, cand), got)
    box = torch.nn.utils.rnn.pad_sequence(c["qs"][1:], batch_first=True).to(DEV)
    _same(amd.residual_wide_rerank_scores(box, rc, cand[1:]), ref(box, dec, cand[1:]))
    # a shared list with row stride 0, a strided view, out=
    shared = cand[2].expand(n_q, cand.shape[1])
    assert shared.stride(0) == 0
    _same(amd.residual_wide_rerank_scores(pq, rc, shared), ref(pq, dec, shared))
    wide = torch.cat([cand, cand.flip(1)], dim=1)
    view = wide[:, 3:3 + cand.shape[1]]
    assert view.stride(0) == 2 * cand.shape[1]
    _same(amd.residual_wide_rerank_scores(pq, rc, view), ref(pq, dec, view))
    out = torch.full(cand.shape, 7.0, dtype=torch.float32, device=DEV)
    assert amd.residual_wide_rerank_scores(pq, rc, cand, out=out)[0] is out
    np.testing.assert_array_equal(_bits(out), _bits(got[0]))
    # m = 0 and n_q = 0
    e0 = amd.residual_wide_rerank_scores(pq, rc, cand[:, :0])
    assert e0[0].shape == (n_q, 0) and e0[1].shape == (n_q, 0)
    none = amd.PackedQueries(tokens=pq.tokens[:1], offsets=pq.offsets[:1], offsets_host=pq.offsets_host[:1])
    z = amd.residual_wide_rerank_scores(none, rc, cand[:0])
    assert z[0].shape == (0, cand.shape[1]) and z[1].shape == (0, cand.shape[1])
    # rerank() dispatches on the container: the score matrix, and the top-k of the listed pages
    np.testing.assert_array_equal(_bits(amd.rerank(pq, rc, cand)), _bits(got[0]))
    _same(amd.rerank(pq, rc, cand, 5), amd.rerank(pq, dec, cand, 5))
    with pytest.raises(NotImplementedError):
        amd.rerank(pq, rc, cand, ref_rounding=True)


def test_refusals_on_the_device(amd):
    c = _case(amd, 256, 2, "bf16")
    rc, pq = c["rc"], c["pq"]
    cand = c["all_ids"].contiguous()
    g = torch.Generator().manual_seed(3)

    def unit(n, dtype=torch.bfloat16, width=W):
        return torch.nn.functional.normalize(torch.randn(n, width, generator=g), dim=-1).to(dtype)

    with pytest.raises(RuntimeError):                                      # the query dtype and rc's differ, as rerank raises
        amd.residual_wide_rerank_scores([unit(8, torch.float16)], rc, cand[:1])
    with pytest.raises(NotImplementedError, match="width 320"):            # width 128
        amd.residual_wide_rerank_scores([unit(8, width=128)], rc, cand[:1])
    with pytest.raises(NotImplementedError):                               # a query over 128 tokens
        amd.residual_wide_rerank_scores([unit(129)], rc, cand[:1])
    for bad in (cand.to(torch.int32), cand.cpu(), cand[0], cand[:1]):
        with pytest.raises(ValueError):
            amd.residual_wide_rerank_scores(pq, rc, bad)
    # everything that exists at width 128 only refuses the wide shard by its type, naming the width, before any kernel runs
    for call in (lambda: amd.residual_rerank_scores(pq, rc, cand), lambda: amd.residual_scores(pq, rc),
                 lambda: amd.residual_align(pq, rc, cand), lambda: amd.residual_gather_pages(rc, cand),
                 lambda: amd.LiveResidualCorpus.like(rc, 100, 10), lambda: amd.LiveResidualCorpus.from_residual(rc, 100, 10)):
        with pytest.raises(NotImplementedError, match="width 128"):
            call()
    with pytest.raises(NotImplementedError):                               # the 128 classes keep refusing 320-wide pages
        amd.ResidualCorpus.build(c["corpus"], bits=2)
    narrow = amd.pack_passages([unit(300, width=128)], DEV, batch_size=None)
    with pytest.raises(NotImplementedError):
        amd.ResidualWideCorpus.build(narrow, bits=2)
    with pytest.raises(ValueError):
        amd.ResidualWideCorpus.build(c["corpus"], bits=3)
    with pytest.raises(ValueError):                                        # cutoffs without weights
        amd.ResidualWideCorpus.build(c["corpus"], index=rc.index, cutoffs=rc.cutoffs)
    other = amd.pack_passages([unit(300)], DEV, batch_size=None)
    with pytest.raises(ValueError):                                        # an index of another corpus
        amd.ResidualWideCorpus.build(other, index=rc.index)


# ---------------------------------------------------------------------------------------------------------------- 4. truth
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_scores_against_the_float64_maxsim_of_the_truths_rows(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    xhat = wt.from_bits(c["xhat_bits"], dt)
    Q = c["pq"].tokens.float().cpu().numpy()[:sum(QUERY_LENS)]
    want, chain = wt.maxsim64(Q, c["pq"].offsets_host.numpy(), xhat, c["d_off"], c["clamp"])
    got = c["all_scores"].double().cpu().numpy()
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin])                    # an unflagged page without rows: -inf
    assert (got[0][fin[0]] == 0).all()                                      # the query of 0 tokens
    err = np.abs(got[fin] - want[fin])
    tol = RTOL * np.maximum(np.abs(want[fin]), 1.0)
    print(f"    K={K} bits={bits} {dt}: largest error {err.max():.3e} (its tolerance {tol[err.argmax()]:.3e}, the fp32 chain's bound "
          f"{chain[fin][err.argmax()]:.3e})")
    assert (err <= tol).all()


# ---------------------------------------------------------------------------------------------------------------- 5. tail masking
def _far_case(amd, planted, dtype=torch.bfloat16, seed=41):
    """All similarities negative (tests/helpers.py: far_side_case), pages of every tail class plus five 65-row and three 33-row
    pages; planted: one row on the queries' side at row 0, 31, 32, 63, 64 of the 65-row pages, at row 0, 31, 32 of the 33-row pages
    and at the last row of every other page.  256 given centroids: page rows, and six rows on the queries' side so that a planted
    row has a centroid near it."""
    lens = PAGE_LENS + [65] * 5 + [33] * 3
    qs, ps, _ = far_side_case(seed, [1, 16, 17, 33, 128], lens, W, dtype, planted=False)
    g = torch.Generator().manual_seed(seed)
    u = far_side_axis(W, g)
    g2 = torch.Generator().manual_seed(seed + 1)
    winners = [-1] * len(ps)
    if planted:
        special = [0, 31, 32, 63, 64, 0, 31, 32]
        for c, p in enumerate(ps):
            if p.shape[0]:
                winners[c] = special[c - len(PAGE_LENS)] if c >= len(PAGE_LENS) else p.shape[0] - 1
                p[winners[c]] = far_side_rows(1, u, +1, g2, dtype)[0]
    C = torch.cat([ps[PAGE_LENS.index(300)][20:270], far_side_rows(6, u, +1, g2, dtype)])
    corpus = amd.pack_passages(ps, DEV, batch_size=None, id_base=ID_BASE)
    rc = amd.ResidualWideCorpus.build(corpus, index=amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV)), bits=4, sample_rows=4096,
                                      seed=2)
    return qs, ps, winners, rc


@pytest.mark.parametrize("planted", [False, True], ids=["all-negative", "planted"])
def test_rows_past_the_page_end_are_masked_not_zero_filled(amd, planted):
    qs, ps, winners, rc = _far_case(amd, planted)
    n = len(ps)
    lens = [int(p.shape[0]) for p in ps]
    assert lens.count(33) >= 3 and lens.count(65) >= 5
    d_off = np.concatenate([[0], np.cumsum(lens)])
    pq = amd.pack_queries(qs, DEV)
    q_off = pq.offsets_host.numpy()
    dec = rc.decompress()
    rows = int(d_off[-1])
    codes = _u16(rc.codes)[:rows]
    C32, rows32 = rc.centroids.float().cpu().numpy(), torch.cat(ps).float().numpy()
    xhat_bits = wt.decode(C32, codes, wt.encode(rows32, C32, codes, rc.cutoffs.cpu().numpy(), 4), rc.weights.cpu().numpy(), 4, "bf16")
    np.testing.assert_array_equal(_u16(dec.blob)[:rows], xhat_bits)
    xhat = wt.from_bits(xhat_bits, "bf16").astype(np.float64)
    Q = torch.cat(qs).double().numpy()
    S = Q @ xhat.T
    # the precondition, on the truth's own decoded rows
    if not planted:
        assert S.max() <= -SIGN_MARGIN, S.max()
    else:
        for c in range(n):
            if lens[c]:
                page = S[:, d_off[c]:d_off[c + 1]]
                w = winners[c]
                assert (page.argmax(axis=1) == w).all() and page[:, w].min() >= SIGN_MARGIN
                assert np.delete(page, w, axis=1).max(initial=-1.0) <= -SIGN_MARGIN
    cand = (torch.arange(n, device=DEV) + ID_BASE).expand(len(qs), n)
    got = amd.residual_wide_rerank_scores(pq, rc, cand)
    _same(got, amd.retrieval.rerank_scores(pq, dec, cand))                  # the identity holds here too
    want, tol = wt.maxsim64(Q, q_off, xhat, d_off)
    s = got[0].double().cpu().numpy()
    empty = np.array(lens) == 0
    assert np.isneginf(s[:, empty]).all()
    err = np.abs(s[:, ~empty] - want[:, ~empty])
    print(f"    {'planted' if planted else 'all-negative'}: largest error {err.max():.3e}, smallest bound {tol[:, ~empty].min():.3e}")
    assert (err <= tol[:, ~empty]).all()                                    # one leaked zero or one lost row is >= 0.05 away


# ---------------------------------------------------------------------------------------------------------------- 6. a bad code
@pytest.mark.parametrize("K,bits,dt,code", [(256, 2, "bf16", 256), (2048, 4, "f16", 2048), (2048, 2, "bf16", 65535)])
def test_a_code_beyond_k_poisons_its_page_only(amd, K, bits, dt, code):
    c = _case(amd, K, bits, dt)
    rc = c["rc"]
    page = PAGE_LENS.index(65)
    row = int(c["d_off"][page]) + 40
    codes = rc.codes.clone()
    codes.view(torch.int16)[row] = code if code < 32768 else code - 65536
    bad = amd.ResidualWideCorpus(rc.centroids, codes, rc.residuals, rc.cutoffs, rc.weights, rc.offsets, rc.clamp0, rc.lengths, rc.id_base,
                                 bits)
    got = amd.residual_wide_rerank_scores(c["pq"], bad, c["all_ids"])[0].cpu()
    want = c["all_scores"].cpu()
    assert bool(torch.isnan(got[1:, page]).all()) and float(got[0, page]) == 0.0          # (a query of 0 tokens reads no page)
    keep = [p for p in range(len(PAGE_LENS)) if p != page]
    np.testing.assert_array_equal(_bits(got[:, keep]), _bits(want[:, keep]))
    dec = bad.decompress([page])
    bits16 = _u16(dec.blob)
    assert (bits16[40] == (0x7E00 if dt == "f16" else 0x7FC0)).all()
    np.testing.assert_array_equal(np.delete(bits16, 40, axis=0), np.delete(c["xhat_bits"][c["d_off"][page]:c["d_off"][page + 1]], 40, axis=0))


def test_encode_writes_zero_buckets_for_a_code_beyond_k(amd):
    c = _case(amd, 256, 4, "bf16")
    rc = c["rc"]
    codes = rc.codes.clone()
    codes.view(torch.int16)[5] = 256
    codes.view(torch.int16)[6] = -1                                          # 65535
    res = torch.full_like(rc.residuals, 0xEE)
    L = amd._lib.lib()
    rcode = L.msim_res_wide_encode_docs(0, c["corpus"].blob.data_ptr(), c["rows"], W, codes.data_ptr(), rc.centroids.data_ptr(), 256,
                                        rc.cutoffs.data_ptr(), 4, res.data_ptr(), amd._lib.current_stream_handle(DEV))
    assert rcode == 0
    got = res.cpu().numpy()[:c["rows"]]
    want = rc.residuals.cpu().numpy()[:c["rows"]].copy()
    want[5:7] = 0
    np.testing.assert_array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------- 7. broken q_off
def test_device_offsets_that_disagree_with_the_host_copy_poison_the_call(amd):
    """The call validates q_off_host; a device q_off that says otherwise is never trusted as an address: every score is NaN."""
    c = _case(amd, 256, 2, "bf16")
    pq = c["pq"]
    off = pq.offsets.clone()
    off[-1] = 100000
    bad = amd.PackedQueries(tokens=pq.tokens, offsets=off, offsets_host=pq.offsets_host)
    s = amd.residual_wide_rerank_scores(bad, c["rc"], c["all_ids"])[0]
    assert bool(torch.isnan(s).all())


# ---------------------------------------------------------------------------------------------------------------- 8. - 10. search
@pytest.mark.parametrize("K,bits,dt", [(256, 2, "bf16"), (2048, 4, "f16")])
def test_two_stage_search_over_the_compressed_shard(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, pq, dec = c["rc"], c["pq"], c["dec"]
    n = len(rc)
    r = amd.ShardedRetriever(rc)
    assert r._rerank is amd.residual_wide_rerank_scores
    for k in (1, 5, n + 3):
        want = amd.rerank(pq, dec, c["all_ids"], k)                        # rerank over decompress()
        _same(r.search(pq, k=k, prefilter=rc.index, n_candidates=n), want)
        _same(r.search(pq, k=k, candidates=c["all_ids"]), want)
    _same(r.search(c["qs"], k=5, prefilter=rc.index, n_candidates=n), amd.rerank(pq, dec, c["all_ids"], 5))      # a host list
    # a short list: stage 1 decides what is reranked
    _, ci = amd.topk(amd.centroid_wide_scores(pq, rc.index), 3, ID_BASE)
    _same(r.search(pq, k=3, prefilter=rc.index, n_candidates=3), amd.rerank(pq, dec, ci, 3))
    # three stages: the FP4 rows of the corpus, built before it is freed, between the centroid scan and the residual rerank
    fp4 = amd.Fp4WideIndex.build(c["corpus"])
    # (rows 1 ..: for the query of 0 tokens every page ties at 0 and the empty page, which the refine stage scores -inf and drops, would
    # lead the list by its id)
    for k in (1, 5):
        want = amd.rerank(pq, dec, c["all_ids"], k)
        for got in (r.search(pq, k=k, prefilter=rc.index, n_candidates=n, refine=fp4, n_refine=n),
                    r.search(pq, k=k, candidates=c["all_ids"], refine=fp4, n_refine=n)):
            np.testing.assert_array_equal(_bits(got[0][1:]), _bits(want[0][1:]))
            np.testing.assert_array_equal(got[1][1:].cpu().numpy(), want[1][1:].cpu().numpy())
    # a long list: as many entries as the selection takes
    long = (torch.arange(amd.TOPK_MAX_K, device=DEV) % n + ID_BASE).expand(len(pq), amd.TOPK_MAX_K)
    ls, li = r.search(pq, k=4, candidates=long)
    np.testing.assert_array_equal(_bits(ls[:, 0]), _bits(amd.rerank(pq, dec, c["all_ids"], 1)[0][:, 0]))
    # the scanning routes and align: refused, and the message sends nobody looking for a hook
    flt = object()
    for call in (lambda: r.search(pq, k=3), lambda: r.search(pq, k=3, filter=flt), lambda: r.search(pq, k=3, group_by=object()),
                 lambda: r.search(pq, k=3, candidates=c["all_ids"], filter=flt), lambda: r.align(pq, c["all_ids"]),
                 lambda: r.mine(pq, None, 2)):
        with pytest.raises(NotImplementedError, match="width 128 only"):
            call()
    for opt_in in (amd.ShardedRetriever(rc, score_fn=amd.residual_scores), amd.ShardedRetriever(rc, align_fn=amd.residual_align)):
        for call in (lambda: opt_in.search(pq, k=3), lambda: opt_in.align(pq, c["all_ids"])):
            with pytest.raises(NotImplementedError, match="width 128"):
                call()


# ---------------------------------------------------------------------------------------------------------------- 11. the drop-in
def test_create_plaid_index_with_nbits(amd):
    c = _case(amd, 256, 2, "bf16")
    ps = c["pages"]
    n = len(ps)
    g = torch.Generator().manual_seed(9)
    box = torch.nn.functional.normalize(torch.from_numpy(c["C32"][:60]).reshape(3, 20, W) + 0.06 * torch.randn(3, 20, W, generator=g),
                                        dim=-1).to(torch.bfloat16)
    index = amd.create_plaid_index(ps, DEV, nbits=2, n_centroids=256, n_candidates=10**6)
    shard = index.retriever.shard
    assert type(index) is amd.ResidualMaxSimIndex and type(shard) is amd.ResidualWideCorpus and shard.bits == 2 and shard.n_centroids == 256
    res = index.search(queries_embeddings=box, top_k=5)
    assert len(res) == 3 and all(len(r) == 5 for r in res)
    assert all(isinstance(i, int) and isinstance(s, float) for r in res for i, s in r)
    assert all(r[j][1] >= r[j + 1][1] for r in res for j in range(4))
    # the scores are the exact ones over the decoded pages
    dec = shard.decompress()
    all_ids = torch.arange(n, device=DEV).expand(3, n)
    s, i = amd.rerank(box.to(DEV), dec, all_ids, 5)
    assert [[t[0] for t in r] for r in res] == i.cpu().tolist()
    assert [[t[1] for t in r] for r in res] == s.cpu().tolist()
    assert type(amd.create_plaid_index(ps, DEV)) is amd.ExactMaxSimIndex       # nbits=None is still the exact index


# ---------------------------------------------------------------------------------------------------------------- 12. capture
def test_captured_rerank_replays_the_eager_bits_and_the_workspace_ignores_the_rows(amd):
    c = _case(amd, 2048, 4, "bf16")
    rc, pq = c["rc"], c["pq"]
    cand = _lists(len(rc), len(pq), 21)

    def fn():
        return amd.residual_wide_rerank_scores(pq, rc, cand)

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
        _same(captured, eager)
    # the workspace: a function of (n_q, m, n) with no row count to pass; nothing outside the stated bytes is written
    L = amd._lib.lib()
    n, n_q, m = len(rc), len(pq), int(cand.shape[1])
    nbytes = int(L.msim_res_wide_candidates_workspace_bytes(n_q, m, n))
    assert 0 < nbytes <= 64 and nbytes % 16 == 0 and nbytes == int(L.msim_res_wide_candidates_workspace_bytes(n_q, m, 10**6))
    guard = torch.full((nbytes + 512,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = guard[256:256 + nbytes]
    out = torch.empty((n_q, m), dtype=torch.float32, device=DEV)
    ids = torch.empty((n_q, m), dtype=torch.int64, device=DEV)
    rcode = L.msim_res_wide_candidates(0, pq.tokens.data_ptr(), pq.offsets.data_ptr(), pq.offsets_host.data_ptr(), n_q, rc.codes.data_ptr(),
                                       rc.residuals.data_ptr(), rc.centroids.data_ptr(), 2048, rc.weights.data_ptr(), 4,
                                       rc.offsets.data_ptr(), rc.clamp0.data_ptr(), n, int(rc.codes.shape[0]), W, cand.data_ptr(), m, m,
                                       ID_BASE, out.data_ptr(), m, ids.data_ptr(), ws.data_ptr(), amd._lib.current_stream_handle(DEV))
    assert rcode == 0
    torch.cuda.synchronize()
    gh = guard.cpu().numpy()
    assert (gh[:256] == 0xAB).all() and (gh[256 + nbytes:] == 0xAB).all()
    assert int(ws[:4].view(torch.int32).item()) == 0                       # the status word: no broken invariant
    _same((out, ids), eager)


# ---------------------------------------------------------------------------------------------------------------- 13. save / load
@pytest.mark.parametrize("K,bits,dt", [(256, 2, "bf16"), (2048, 4, "f16")])
def test_save_load_round_trip_and_page_ranges(amd, tmp_path, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc = c["rc"]

    def same_tensors(a, b, names):
        for name in names:
            x, y = getattr(a, name), getattr(b, name)
            assert (x is None) == (y is None), name
            if x is not None:
                assert x.dtype == y.dtype and x.shape == y.shape, name
                np.testing.assert_array_equal(x.cpu().contiguous().view(torch.uint8).numpy(), y.cpu().contiguous().view(torch.uint8).numpy())

    cent = ("centroids", "codes", "offsets", "clamp0", "lengths")
    res = cent + ("residuals", "cutoffs", "weights")
    for obj, names in ((rc, res), (rc.index, cent)):
        path = str(tmp_path / f"{type(obj).__name__}.msim")
        obj.save(path, chunk_bytes=1 << 12)
        assert amd.verify_file(path)["kind"] == type(obj).__name__
        for back in (type(obj).load(path, DEV), amd.load(path, DEV)):
            assert type(back) is type(obj) and back.id_base == obj.id_base and len(back) == len(obj)
            same_tensors(back, obj, names)
        other = amd.ResidualCorpus if obj is rc else amd.CentroidIndex
        with pytest.raises(amd.ShardFileError):
            other.load(path, DEV)                                           # the 128 class refuses the wide file by its kind
    # pages=(lo, hi): the build over that page range with the same centroids and codec
    lo, hi = 3, 11
    part = amd.pack_passages(c["pages"][lo:hi], DEV, batch_size=None, id_base=ID_BASE + lo)
    part.clamp0 = rc.clamp0[lo:hi].clone()
    pidx = amd.CentroidWideIndex.build(part, centroids=rc.centroids)
    prc = amd.ResidualWideCorpus.build(part, index=pidx, bits=bits, cutoffs=rc.cutoffs, weights=rc.weights)
    rows = sum(PAGE_LENS[lo:hi])
    got = amd.ResidualWideCorpus.load(str(tmp_path / "ResidualWideCorpus.msim"), DEV, pages=(lo, hi))
    assert got.id_base == ID_BASE + lo and got.lengths.tolist() == PAGE_LENS[lo:hi] and got.bits == bits
    np.testing.assert_array_equal(_u16(got.codes)[:rows], _u16(prc.codes)[:rows])
    np.testing.assert_array_equal(got.residuals.cpu().numpy()[:rows], prc.residuals.cpu().numpy()[:rows])
    np.testing.assert_array_equal(got.offsets.cpu().numpy(), prc.offsets.cpu().numpy())
    np.testing.assert_array_equal(got.clamp0.cpu().numpy(), prc.clamp0.cpu().numpy())
    gidx = amd.CentroidWideIndex.load(str(tmp_path / "CentroidWideIndex.msim"), DEV, pages=(lo, hi))
    assert gidx.id_base == ID_BASE + lo and len(gidx) == hi - lo
    np.testing.assert_array_equal(_u16(gidx.codes)[:rows], _u16(pidx.codes)[:rows])
    ids = (torch.arange(hi - lo, device=DEV) + ID_BASE + lo).expand(len(c["pq"]), hi - lo)
    _same(amd.residual_wide_rerank_scores(c["pq"], got, ids), amd.residual_wide_rerank_scores(c["pq"], prc, ids))
