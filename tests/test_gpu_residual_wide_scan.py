"""The full scan of a residual-compressed 320-wide shard on the MI355X (msim_res_wide_scores, colpali_amd.residual_wide_scores) and
the routes `ShardedRetriever(rc, score_fn=residual_wide_scores)` opens over it.

The contract: residual_wide_scores(q, rc) equals the rerank over all ids (residual_wide_rerank_scores) bit for bit, whatever queries
share a wave -- which are the bits of maxsim_scores(q, rc.decompress()) wherever that scan runs the flat panel kernel K1bPF (every
batch of mixed lengths) -- and stays within the rerank test's tolerance of the float64 MaxSim of the truth's decoded rows
(tests/residual_wide_truth.py).  A scan of the decompressed pages with ONE query length and at most four 32-token tiles runs K1sP,
whose token sum is a butterfly: against it the scan agrees to the bound include/maxsim.h states.  The corpora are the ones
tests/test_gpu_residual_wide.py builds (K = 256 and 2048, 2 and 4 bits, bf16 and f16; pages of 0 .. 300 rows, queries of 0 .. 128
tokens), shared with that module and left unchanged."""
import numpy as np
import pytest
import torch

from tests import residual_wide_truth as wt
from tests.helpers import SIGN_MARGIN
from tests.test_gpu_residual_wide import (CASES, DEV, ID_BASE, PAGE_LENS, QUERY_LENS, RTOL, W, _bits, _case, _codec, _far_case, _same, _u16,  # noqa: F401
                                          amd)
from tests.test_gpu_residual import dist  # noqa: F401

pytestmark = pytest.mark.gpu


def _eq(got, want, what=""):
    assert got.shape == want.shape
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _scan(amd, c):
    """the scan of a case, once"""
    if "scan" not in c:
        c["scan"] = amd.residual_wide_scores(c["pq"], c["rc"])
        c["full"] = amd.maxsim_scores(c["pq"], c["dec"])                    # mixed lengths: K1bPF
    return c["scan"]


# ---------------------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_scan_is_bit_identical_to_the_rerank_and_to_the_scan_of_the_decompressed_pages(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, dec, pq = c["rc"], c["dec"], c["pq"]
    n, n_q = len(PAGE_LENS), len(QUERY_LENS)
    assert rc.clamp0 is not None and 0 < int(rc.clamp0.sum()) < n and rc.id_base == ID_BASE != 0
    got = _scan(amd, c)
    assert got.shape == (n_q, n) and got.dtype == torch.float32
    _eq(got, c["all_scores"], "the rerank over all ids")
    _eq(got, c["full"], "maxsim_scores over the decompressed pages")
    s = got.cpu()
    assert bool((s[0] == 0).all())                                          # the 0-token query scores 0
    empty = PAGE_LENS.index(0)
    flagged = bool(c["clamp"][empty])
    assert bool((s[1:, empty] == (0.0 if flagged else float("-inf"))).all())
    _eq(amd.residual_wide_scores(pq, rc), got, "a rerun")
    _eq(amd.residual_wide_scores(c["qs"], rc), got, "the host list")
    box = torch.nn.utils.rnn.pad_sequence(c["qs"][1:], batch_first=True).to(DEV)
    _eq(amd.residual_wide_scores(box, rc), amd.maxsim_scores(box, dec), "the dense device box")
    out = torch.full((n_q, n), 7.0, dtype=torch.float32, device=DEV)
    assert amd.residual_wide_scores(pq, rc, out=out) is out
    _eq(out, got, "out=")
    none = amd.PackedQueries(tokens=pq.tokens[:1], offsets=pq.offsets[:1], offsets_host=pq.offsets_host[:1])
    assert amd.residual_wide_scores(none, rc).shape == (0, n)


# ---------------------------------------------------------------------------------------------------------------- 2. the K1sP corner
def test_the_single_length_scan_corner_agrees_to_summation_order(amd):
    """4 queries x 32 tokens: maxsim_scores of exactly these over the decompressed pages runs K1sP (butterfly token sum); the scan of
    the compressed shard carries the rerank's, that is K1bPF's, bits."""
    c = _case(amd, 2048, 4, "bf16")
    rc, dec, n = c["rc"], c["dec"], len(PAGE_LENS)
    g = torch.Generator().manual_seed(12)
    L = 32

    def query(tokens):
        near = c["C"][torch.randint(0, c["K"], (tokens,), generator=g)].float()
        return torch.nn.functional.normalize(near + 0.06 * torch.randn(tokens, W, generator=g), dim=-1).to(torch.bfloat16)

    qs = [query(L) for _ in range(4)]
    pq = amd.pack_queries(qs, DEV)
    got = amd.residual_wide_scores(pq, rc)
    all_ids = (torch.arange(n, device=DEV) + ID_BASE).expand(4, n)
    _eq(got, amd.residual_wide_rerank_scores(pq, rc, all_ids)[0], "the rerank over all ids")
    forced = amd.maxsim_scores(amd.pack_queries(qs + [query(33)], DEV), dec)[:4]          # a 33-token query forces K1bPF
    _eq(got, forced, "the four with a 33-token query appended")
    alone = amd.maxsim_scores(pq, dec)                                                    # K1sP
    # include/maxsim.h: |delta| <= 2 gamma(L - 1) sum_i |M_i|, |M_i| <= |q_i| |row| <= 1.01 x the longest decoded row
    norm = float(dec.blob.double().norm(dim=-1).max())
    n1 = (L - 1) * 2.0 ** -24
    bound = 2.0 * (n1 / (1.0 - n1)) * 1.01 * norm * L
    fin = torch.isfinite(alone).cpu()
    assert torch.equal(fin, torch.isfinite(got).cpu())
    np.testing.assert_array_equal(got.cpu()[~fin].numpy(), alone.cpu()[~fin].numpy())     # the empty page
    diff = float((got.double().cpu()[fin] - alone.double().cpu()[fin]).abs().max())
    print(f"    K1sP corner: max |scan - K1sP| = {diff:.3e}, bound = {bound:.3e}")
    assert diff <= bound


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_on_the_device(amd):
    c = _case(amd, 256, 2, "bf16")
    rc, pq = c["rc"], c["pq"]
    g = torch.Generator().manual_seed(3)

    def unit(n, dtype=torch.bfloat16, width=W):
        return torch.nn.functional.normalize(torch.randn(n, width, generator=g), dim=-1).to(dtype)

    with pytest.raises(RuntimeError):                                      # the query dtype and rc's differ
        amd.residual_wide_scores([unit(8, torch.float16)], rc)
    with pytest.raises((NotImplementedError, RuntimeError)):               # fp32
        amd.residual_wide_scores([unit(8, torch.float32)], rc)
    with pytest.raises(NotImplementedError, match="width 320"):            # width 128
        amd.residual_wide_scores([unit(8, width=128)], rc)
    with pytest.raises(NotImplementedError):                               # a query over 128 tokens
        amd.residual_wide_scores([unit(129)], rc)
    with pytest.raises(ValueError):
        amd.residual_wide_scores(pq, rc.index)
    narrow = amd.ResidualCorpus(torch.zeros(256, 128, dtype=torch.bfloat16, device=DEV), torch.zeros(4, dtype=torch.int16, device=DEV).view(torch.uint16),
                                torch.zeros(4, 32, dtype=torch.uint8, device=DEV), torch.zeros(3, device=DEV), torch.zeros(4, device=DEV),
                                torch.tensor([0, 4], dtype=torch.int32, device=DEV), None, torch.tensor([4]), 0, 2)
    with pytest.raises(NotImplementedError, match="width 320"):            # the sibling class: refused by type, naming the width
        amd.residual_wide_scores([unit(8, width=128)], narrow)
    with pytest.raises(NotImplementedError, match="width 128"):
        amd.residual_scores(pq, rc)
    n_q, n = len(pq), len(rc)
    for bad in (torch.empty((n_q, n), dtype=torch.float64, device=DEV), torch.empty((n_q, n + 1), device=DEV), torch.empty((n_q, n)),
                torch.empty((n, n_q), device=DEV).t(), torch.empty((n_q, 2 * n), device=DEV)[:, ::2]):
        with pytest.raises(ValueError):
            amd.residual_wide_scores(pq, rc, out=bad)


# ---------------------------------------------------------------------------------------------------------------- 4. groups
def test_the_bits_do_not_depend_on_which_queries_share_a_wave(amd):
    c = _case(amd, 2048, 2, "bf16")
    rc = c["rc"]
    n = len(rc)
    g = torch.Generator().manual_seed(77)
    C = rc.centroids.float().cpu()

    def query(tokens):
        near = C[torch.randint(0, C.shape[0], (tokens,), generator=g)]
        return torch.nn.functional.normalize(near + 0.1 * torch.randn(tokens, W, generator=g), dim=-1).to(torch.bfloat16)

    pool = {t: [query(t) for _ in range(k)] for t, k in ((1, 17), (16, 8), (32, 4), (128, 1), (33, 1))}
    zero = torch.zeros(3, W, dtype=torch.bfloat16)                         # compaction leaves a query of 0 tokens
    single = {}

    def alone(q):
        if id(q) not in single:
            single[id(q)] = amd.residual_wide_scores([q], rc)
            assert single[id(q)].shape == (1, n)
        return single[id(q)]

    batches = [pool[1][:k] for k in (1, 2, 8, 9, 17)]                      # the eight-query cap, not the token cap
    batches += [pool[16], pool[32], [pool[128][0], pool[1][0]], [zero, zero, zero]]      # exactly 128 tokens; 4 x 32; 8 units + 1; no token at all
    batches += [[zero, pool[1][3], zero, pool[32][1], pool[128][0], zero]]
    for batch in batches:
        pq = amd.pack_queries(batch, DEV)
        lens = pq.lengths.tolist()
        assert lens == [0 if q is zero else int(q.shape[0]) for q in batch]
        got = amd.residual_wide_scores(pq, rc)
        want = torch.cat([alone(q) for q in batch])
        _eq(got, want, f"batch of {lens}")
        if int(pq.lengths.sum()):
            # against the decompressed scan: a 33-token query appended and dropped sends every batch to K1bPF
            forced = amd.maxsim_scores(amd.pack_queries(list(batch) + pool[33], DEV), c["dec"])[:len(batch)]
            _eq(got, forced, f"batch of {lens} against the decompressed scan")
        # out= a column slice of a wider matrix: the other columns keep their bits
        wide = torch.full((len(batch), n + 7), -123.25, dtype=torch.float32, device=DEV)
        assert amd.residual_wide_scores(pq, rc, out=wide[:, 3:3 + n]).data_ptr() == wide[:, 3:].data_ptr()
        _eq(wide[:, 3:3 + n], want, "out= a column slice")
        rest = torch.cat([wide[:, :3], wide[:, 3 + n:]], dim=1).cpu()
        assert bool((rest == -123.25).all())
    assert bool((alone(zero) == 0).all())


# ---------------------------------------------------------------------------------------------------------------- 5. more pages than waves
def test_more_pages_than_waves(amd):
    """~1 300 pages of 1 .. 40 rows (~26 k rows): more pages than the 1 024 waves of the persistent grid on 256 CUs, so waves reuse
    their LDS table across pages, and across the three groups of the 9 queries"""
    g = torch.Generator().manual_seed(1300)
    K, n = 256, 1300
    C = torch.nn.functional.normalize(torch.randn(K, W, generator=g), dim=-1).to(torch.bfloat16)
    lens = torch.randint(1, 41, (n,), generator=g)
    rows = int(lens.sum())
    assert 22_000 < rows < 31_000
    flat = torch.nn.functional.normalize(C[torch.randint(0, K, (rows,), generator=g)].float() + 0.022 * torch.randn(rows, W, generator=g),
                                         dim=-1).to(torch.bfloat16)
    corpus = amd.pack_passages(list(torch.split(flat, lens.tolist())), DEV, batch_size=None, id_base=ID_BASE)
    corpus.clamp0 = (torch.rand(n, generator=g) < 0.5).to(torch.uint8).to(DEV)
    cutoffs, weights = _codec(2)
    rc = amd.ResidualWideCorpus.build(corpus, index=amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV)), bits=2, cutoffs=cutoffs.to(DEV),
                                      weights=weights.to(DEV))
    q_lens = [20, 5, 33, 1, 64, 17, 128, 3, 40]                             # 311 tokens: at least three groups
    qs = [torch.nn.functional.normalize(C[torch.randint(0, K, (t,), generator=g)].float() + 0.1 * torch.randn(t, W, generator=g), dim=-1)
          .to(torch.bfloat16) for t in q_lens]
    pq = amd.pack_queries(qs, DEV)
    got = amd.residual_wide_scores(pq, rc)
    _eq(got, amd.maxsim_scores(pq, rc.decompress()))
    assert bool(torch.isfinite(got).all())


# ---------------------------------------------------------------------------------------------------------------- 6. tail masking
@pytest.mark.parametrize("planted", [False, True], ids=["all-negative", "planted"])
def test_rows_past_the_page_end_are_masked_not_zero_filled(amd, planted):
    qs, ps, winners, rc = _far_case(amd, planted)
    n = len(ps)
    lens = [int(p.shape[0]) for p in ps]
    d_off = np.concatenate([[0], np.cumsum(lens)])
    pq = amd.pack_queries(qs, DEV)
    q_off = pq.offsets_host.numpy()
    rows = int(d_off[-1])
    codes = _u16(rc.codes)[:rows]
    C32, rows32 = rc.centroids.float().cpu().numpy(), torch.cat(ps).float().numpy()
    xhat_bits = wt.decode(C32, codes, wt.encode(rows32, C32, codes, rc.cutoffs.cpu().numpy(), 4), rc.weights.cpu().numpy(), 4, "bf16")
    xhat = wt.from_bits(xhat_bits, "bf16").astype(np.float64)
    Q = torch.cat(qs).double().numpy()
    S = Q @ xhat.T
    # the precondition, on the truth's own decoded rows, before any output is read
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
    got = amd.residual_wide_scores(pq, rc)
    _eq(got, amd.residual_wide_rerank_scores(pq, rc, cand)[0])              # the identity holds here too
    want, tol = wt.maxsim64(Q, q_off, xhat, d_off)
    s = got.double().cpu().numpy()
    empty = np.array(lens) == 0
    assert np.isneginf(s[:, empty]).all()
    err = np.abs(s[:, ~empty] - want[:, ~empty])
    print(f"    {'planted' if planted else 'all-negative'}: largest error {err.max():.3e}, smallest bound {tol[:, ~empty].min():.3e}")
    assert (err <= tol[:, ~empty]).all()                                    # one leaked zero or one lost row is >= 0.05 away


# ---------------------------------------------------------------------------------------------------------------- 7. truth
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_scores_against_the_float64_maxsim_of_the_truths_rows(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    xhat = wt.from_bits(c["xhat_bits"], dt)
    Q = c["pq"].tokens.float().cpu().numpy()[:sum(QUERY_LENS)]
    want, chain = wt.maxsim64(Q, c["pq"].offsets_host.numpy(), xhat, c["d_off"], c["clamp"])
    got = _scan(amd, c).double().cpu().numpy()
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin])                    # an unflagged page without rows: -inf
    assert (got[0][fin[0]] == 0).all()                                      # the query of 0 tokens
    err = np.abs(got[fin] - want[fin])
    tol = RTOL * np.maximum(np.abs(want[fin]), 1.0)
    print(f"    K={K} bits={bits} {dt}: largest error {err.max():.3e} (its tolerance {tol[err.argmax()]:.3e}, the fp32 chain's bound "
          f"{chain[fin][err.argmax()]:.3e})")
    assert (err <= tol).all()


# ---------------------------------------------------------------------------------------------------------------- 8. a bad code
@pytest.mark.parametrize("K,bits,dt,code", [(256, 2, "bf16", 256), (2048, 4, "f16", 2048), (2048, 2, "bf16", 65535)])
def test_a_code_beyond_k_poisons_its_column_only(amd, K, bits, dt, code):
    c = _case(amd, K, bits, dt)
    rc = c["rc"]
    want = _scan(amd, c).cpu()
    page = PAGE_LENS.index(65)
    row = int(c["d_off"][page]) + 40
    codes = rc.codes.clone()
    codes.view(torch.int16)[row] = code if code < 32768 else code - 65536
    bad = amd.ResidualWideCorpus(rc.centroids, codes, rc.residuals, rc.cutoffs, rc.weights, rc.offsets, rc.clamp0, rc.lengths, rc.id_base,
                                 bits)
    got = amd.residual_wide_scores(c["pq"], bad).cpu()
    assert bool(torch.isnan(got[1:, page]).all()) and float(got[0, page]) == 0.0          # (a query of 0 tokens reads no page)
    keep = [p for p in range(len(PAGE_LENS)) if p != page]
    np.testing.assert_array_equal(_bits(got[:, keep]), _bits(want[:, keep]))


# ---------------------------------------------------------------------------------------------------------------- 9. routes
@pytest.mark.parametrize("K,bits,dt", [(256, 2, "bf16"), (2048, 4, "f16")])
def test_the_routes_the_scan_opens(amd, dist, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, dec, pq = c["rc"], c["dec"], c["pq"]                                # mixed query lengths: the reference scans with K1bPF
    n, n_q = len(rc), len(pq)
    r, ref = amd.ShardedRetriever(rc, score_fn=amd.residual_wide_scores), amd.ShardedRetriever(dec)
    for k in (1, 5, n + 3):
        _same(r.search(pq, k), ref.search(pq, k))
    kw = dict(world=1, rank=0, dist=dist, force_collective=True)
    _same(amd.ShardedRetriever(rc, score_fn=amd.residual_wide_scores, **kw).search(pq, 5), amd.ShardedRetriever(dec, **kw).search(pq, 5))
    _same(r.search(c["qs"], 5), ref.search(c["qs"], 5))                     # a host list is packed as for the retriever's own scan
    rng = np.random.default_rng(11)
    shared = rng.random(n) < 0.5
    shared[[0, 3]] = True                                                   # the 0-row page is allowed
    per = rng.random((n_q, n)) < 0.5
    per[2] = False                                                          # a query with no allowed page

    def filters():
        return [amd.PageFilter.from_mask(torch.from_numpy(shared).to(DEV), ID_BASE), amd.PageFilter.from_mask(torch.from_numpy(per).to(DEV), ID_BASE)]

    groups = amd.PageGroups.from_labels(torch.from_numpy(rng.integers(0, 5, n).astype(np.int64) * 7 + 3).to(DEV), ID_BASE)
    cand = torch.stack([torch.from_numpy(rng.permutation(n + 4)[:9] + ID_BASE - 2) for _ in range(n_q)]).to(DEV)

    def same3(got, want):
        assert len(got) == len(want) == 3
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])

    for fa, fb in zip(filters(), filters()):
        for route in ("mask", "list", "auto"):
            _same(r.search(pq, 4, filter=fa, filter_route=route), ref.search(pq, 4, filter=fb, filter_route=route))
        for route in ("mask", "list"):
            same3(r.search(pq, 4, filter=fa, filter_route=route, group_by=groups), ref.search(pq, 4, filter=fb, filter_route=route, group_by=groups))
        _same(r.search(pq, 4, filter=fa, candidates=cand), ref.search(pq, 4, filter=fb, candidates=cand))
        _same(r.search(pq, 4, filter=fa, prefilter=rc.index, n_candidates=6), ref.search(pq, 4, filter=fb, prefilter=rc.index, n_candidates=6))
    same3(r.search(pq, 3, group_by=groups), ref.search(pq, 3, group_by=groups))
    same3(r.search(pq, 3, group_by=groups, prefilter=rc.index, n_candidates=8), ref.search(pq, 3, group_by=groups, prefilter=rc.index, n_candidates=8))
    positives = torch.tensor([[ID_BASE + 2, -1], [ID_BASE + 5, ID_BASE + 11], [-1, -1], [ID_BASE + 7, -1], [ID_BASE + 1, ID_BASE + 9],
                              [ID_BASE + 4, -1], [ID_BASE + 10, ID_BASE + 6]], device=DEV)
    _same(r.mine(pq, positives, 2, max_ratio=0.95), ref.mine(pq, positives, 2, max_ratio=0.95))
    _same(amd.mine_hard_negatives(pq, rc, positives, 2, max_ratio=0.95, skip_top=1),
          amd.mine_hard_negatives(pq, dec, positives, 2, max_ratio=0.95, skip_top=1))
    with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only"):
        r.align(pq, c["all_ids"])
    with pytest.raises(NotImplementedError, match="score_fn=residual_wide_scores"):
        amd.ShardedRetriever(rc).search(pq, k=3)
    with pytest.raises(NotImplementedError, match="width 128"):            # the sibling's scorer: the type refusal
        amd.ShardedRetriever(rc, score_fn=amd.residual_scores).search(pq, k=3)


# ---------------------------------------------------------------------------------------------------------------- 10. capture
def test_captured_scan_replays_the_eager_bits(amd):
    c = _case(amd, 2048, 4, "bf16")
    rc, pq = c["rc"], c["pq"]
    out = torch.zeros((len(pq), len(rc)), dtype=torch.float32, device=DEV)
    eager = amd.residual_wide_scores(pq, rc).clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                     # warm-up on a side stream, as torch.cuda.graph expects
        amd.residual_wide_scores(pq, rc, out=out)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.residual_wide_scores(pq, rc, out=out)
    for _ in range(2):
        out.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        _eq(out, eager)


def test_workspace_does_not_depend_on_the_rows(amd):
    c = _case(amd, 256, 2, "bf16")
    rc, pq = c["rc"], c["pq"]
    n_q = len(pq)
    L = amd._lib.lib()
    assert L.msim_res_wide_scores_workspace_bytes(n_q, 10) == L.msim_res_wide_scores_workspace_bytes(n_q, 100000)
    nbytes = int(L.msim_res_wide_scores_workspace_bytes(n_q, len(rc)))
    assert 0 < nbytes <= 16 + 16 * n_q and nbytes % 16 == 0
    guard = torch.full((nbytes + 512,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = guard[256:256 + nbytes]
    n = len(rc)
    out = torch.empty((n_q, n), dtype=torch.float32, device=DEV)
    rcode = L.msim_res_wide_scores(0, pq.tokens.data_ptr(), pq.offsets.data_ptr(), pq.offsets_host.data_ptr(), n_q, rc.codes.data_ptr(),
                                   rc.residuals.data_ptr(), rc.centroids.data_ptr(), 256, rc.weights.data_ptr(), 2, rc.offsets.data_ptr(),
                                   rc.clamp0.data_ptr(), n, int(rc.codes.shape[0]), W, out.data_ptr(), n, ws.data_ptr(),
                                   amd._lib.current_stream_handle(DEV))
    assert rcode == 0
    torch.cuda.synchronize()
    gh = guard.cpu().numpy()
    assert (gh[:256] == 0xAB).all() and (gh[256 + nbytes:] == 0xAB).all()               # nothing outside the stated bytes is written
    assert int(ws[:4].view(torch.int32).item()) == 0                                     # the status word: no broken invariant
    _eq(out, _scan(amd, c))


# ---------------------------------------------------------------------------------------------------------------- 11. offsets
def test_device_offsets_that_disagree_with_the_host_copy_poison_the_call(amd):
    """The call validates q_off_host; a device q_off that says otherwise is never trusted as an address: every score is NaN, and
    nothing else is written.  The changed lengths stay inside the token matrix."""
    c = _case(amd, 256, 2, "bf16")
    pq, rc = c["pq"], c["rc"]
    n_q, n = len(pq), len(rc)
    off = pq.offsets.clone()
    off[1:-1] = 0                                                           # every query but the last loses its tokens; the last has 227
    bad = amd.PackedQueries(tokens=pq.tokens, offsets=off, offsets_host=pq.offsets_host)
    wide = torch.full((n_q, n + 7), -123.25, dtype=torch.float32, device=DEV)
    amd.residual_wide_scores(bad, rc, out=wide[:, 3:3 + n])
    assert bool(torch.isnan(wide[:, 3:3 + n]).all())
    rest = torch.cat([wide[:, :3], wide[:, 3 + n:]], dim=1).cpu()
    assert bool((rest == -123.25).all())
    off = pq.offsets.clone()
    assert off.tolist() == [0, 0, 1, 17, 34, 66, 99, 227]
    off[6] = 130                                                            # lengths 64 and 97 for 33 and 128: every length in range, three groups for two
    bad =amd.PackedQueries(tokens=pq.tokens, offsets=off, offsets_host=pq.offsets_host)
    assert bool(torch.isnan(amd.residual_wide_scores(bad, rc)).all())
    _eq(amd.residual_wide_scores(pq, rc), _scan(amd, c), "the next call is clean")
