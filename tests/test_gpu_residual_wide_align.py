"""Rows out of a 320-wide residual-compressed shard on the MI355X: msim_res_wide_align_candidates / msim_res_wide_gather_pages,
colpali_amd.residual_wide_align and residual_wide_gather_pages, the dispatch of align / gather_pages on a ResidualWideCorpus and
ShardedRetriever(rc, align_fn=residual_wide_align).

The contract is an identity: residual_wide_align(q, rc, ids) has the bits of align(q, rc.decompress(), ids),
residual_wide_gather_pages(rc, ids) the bytes of gather_pages(rc.decompress(), ids) -- float bit patterns are compared as int32 /
int16, so -0.0, -inf and NaN count.  The numbers are checked on their own as well: best_sim against the float64 MaxSim of
tests/residual_wide_truth.decode within
    320 * 2^-24 * sum_k |q_k xhat_k|            (an fp32 chain of 320 exact products)
per similarity, and best_row against the float64 first arg-max wherever the float64 top-two gap exceeds that bound.
Shapes: a chunk is 16 rows and the loop a two-chunk pipeline, so the pages have 0 .. 100 rows (0, 1, 2, 3 and 7 chunks, every tail
class); queries of 0 .. 128 tokens (the tile edge, the wave's second tile, the last tile); K = 256 and 2048, 2 and 4 bits, bf16 and
f16."""
import numpy as np
import pytest
import torch

from tests import residual_wide_truth as wt
from tests.helpers import SIGN_MARGIN, far_side_axis, far_side_rows

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
W = 320
PAGE_LENS = [0, 1, 15, 16, 17, 33, 100, 32, 2, 48, 0, 31]
QUERY_LENS = [0, 1, 16, 17, 64, 65, 128]
ID_BASE = 1000
CASES = [(k, bits, dt) for k in (256, 2048) for bits in (2, 4) for dt in ("bf16", "f16")]
TORCH_DT = {"bf16": torch.bfloat16, "f16": torch.float16}
NAN16 = {"bf16": 0x7FC0, "f16": 0x7E00}
N_COLS = 7


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()      # must load: no fallback
    return colpali_amd


def _i32(t):
    return t.detach().contiguous().view(torch.int32)


def _i16(t):
    return t.detach().contiguous().view(torch.int16)


def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def _same_alignment(got, want, where=""):
    """best_sim, best_row, ids and sims: the same shapes and the same bits"""
    for name in ("best_sim", "best_row", "ids", "sims"):
        a, b = getattr(got, name), getattr(want, name)
        assert (a is None) == (b is None), where + name
        if a is None:
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, where + name
        if a.dtype == torch.float32:
            a, b = _i32(a), _i32(b)
        assert torch.equal(a, b), where + name


def _codec(bits):
    """given cutoffs and weights (tests/test_gpu_residual_wide.py); 0.0 is a cutoff"""
    nb = 1 << bits
    cut = (torch.arange(1, nb, dtype=torch.float32) - nb // 2) * (0.04 / (nb // 2))
    edges = torch.cat([cut[:1] - 0.025, cut, cut[-1:] + 0.025])
    return cut.contiguous(), ((edges[:-1] + edges[1:]) / 2).contiguous()


def _id_lists(n_pages, n_q, seed):
    """[n_q, 7]: four listed pages (every page is listed by some query), -1, an id off the shard (below and above it) and, in column
    5, column 0 again"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_pages, generator=g).tolist()
    outside = [ID_BASE - 1, ID_BASE + n_pages, 3, 10**12]
    rows = []
    for q in range(n_q):
        p = [ID_BASE + perm[(4 * q + t) % n_pages] for t in range(4)]
        rows.append([p[0], p[1], -1, outside[q % 4], p[2], p[0], p[3]])
    assert {c - ID_BASE for r in rows for c in (r[0], r[1], r[4], r[6])} == set(range(n_pages))
    return torch.tensor(rows, dtype=torch.int64)


_cases = {}


def _case(amd, K, bits, dt):
    """One shard per (K, bits, dtype), built once and left unchanged: given centroids, cutoffs and weights, pages clustered round the
    centroids, clamp0 on a random half, id_base = 1000; the decompressed shard and the reference Alignment over it are computed once."""
    key = (K, bits, dt)
    if key in _cases:
        return _cases[key]
    dtype = TORCH_DT[dt]
    g = torch.Generator().manual_seed(91 * bits + K + (dt == "f16"))
    C = torch.nn.functional.normalize(torch.randn(K, W, generator=g), dim=-1).to(dtype)
    pages = []
    for n in PAGE_LENS:
        near = C[torch.randint(0, K, (n,), generator=g)].float()
        pages.append(torch.nn.functional.normalize(near + 0.022 * torch.randn(n, W, generator=g), dim=-1).to(dtype))
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    clamp = torch.zeros(len(pages), dtype=torch.uint8)
    clamp[torch.randperm(len(pages), generator=g)[: len(pages) // 2]] = 1
    corpus.clamp0 = clamp.to(DEV)
    cutoffs, weights = _codec(bits)
    index = amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV))
    rc = amd.ResidualWideCorpus.build(corpus, index=index, bits=bits, cutoffs=cutoffs.to(DEV), weights=weights.to(DEV))
    qs = [torch.nn.functional.normalize(C[torch.randint(0, K, (n,), generator=g)].float() + 0.06 * torch.randn(n, W, generator=g),
                                        dim=-1).to(dtype) for n in QUERY_LENS]
    qs[0] = torch.zeros(5, W, dtype=dtype)                         # compaction leaves a query of 0 tokens
    pq = amd.pack_queries(qs, DEV, layout="flat")
    assert pq.lengths.tolist() == QUERY_LENS
    ids = _id_lists(len(pages), len(qs), seed=K + bits)
    dec = rc.decompress()
    out = dict(rc=rc, dec=dec, pq=pq, qs=qs, ids=ids, dids=ids.to(DEV), clamp=clamp.numpy().astype(bool), dt=dt, bits=bits, K=K,
               d_off=np.concatenate([[0], np.cumsum(PAGE_LENS)]), want=amd.align(pq, dec, ids.to(DEV), maps=True),
               want_lean=amd.align(pq, dec, ids.to(DEV)))
    _cases[key] = out
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_align_is_bit_identical_to_align_over_the_decompressed_shard(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, dec, pq, dids = c["rc"], c["dec"], c["pq"], c["dids"]
    n_q = len(QUERY_LENS)
    assert set(PAGE_LENS) >= {0, 1, 15, 16, 17, 33, 100} and set(QUERY_LENS) >= {0, 1, 16, 17, 64, 65, 128}
    got = amd.residual_wide_align(pq, rc, dids, maps=True)
    _same_alignment(got, c["want"], "maps: ")
    assert got.id_base == ID_BASE and got.page_lengths.tolist() == PAGE_LENS and got.query_lengths.tolist() == QUERY_LENS
    assert bool(torch.isfinite(got.best_sim[1:, 0]).any()) and int((got.best_row >= 0).sum()) > 0       # not vacuous
    lean = amd.residual_wide_align(pq, rc, dids)
    _same_alignment(lean, c["want_lean"], "no maps: ")
    assert torch.equal(_i32(lean.best_sim), _i32(got.best_sim)) and torch.equal(lean.best_row, got.best_row)
    # the list's corners: one row shared by every query (stride 0), a row stride > m, no column at all
    shared = dids[3:4].expand(n_q, N_COLS)
    assert shared.stride(0) == 0
    _same_alignment(amd.residual_wide_align(pq, rc, shared, maps=True), amd.align(pq, dec, shared, maps=True), "stride 0: ")
    wide = torch.full((n_q, 11), ID_BASE + 9, dtype=torch.int64, device=DEV)
    wide[:, 2:9] = dids
    view = wide[:, 2:9]
    assert view.stride(0) == 11
    _same_alignment(amd.residual_wide_align(pq, rc, view, maps=True), c["want"], "row stride 11: ")
    none = amd.residual_wide_align(pq, rc, dids[:, :0], maps=True)
    assert none.best_sim.shape == (n_q, 0, 128) and none.best_row.shape == (n_q, 0, 128) and none.sims.shape == (n_q, 0, 128, 100)
    # max_rows below one listed page (100 rows): that entry is NaN / -1 in full, its neighbours keep their bits; 50 is no multiple of 4
    # (the non-vector map store)
    for R in (50, 64):
        short = amd.residual_wide_align(pq, rc, dids, maps=True, max_rows=R)
        _same_alignment(short, amd.align(pq, dec, dids, maps=True, max_rows=R), f"max_rows={R}: ")
        plen = torch.tensor(PAGE_LENS)[(c["ids"] - ID_BASE).clamp(0, len(PAGE_LENS) - 1)]
        inside = (c["ids"] >= ID_BASE) & (c["ids"] < ID_BASE + len(PAGE_LENS))
        too_long = (inside & (plen > R)).to(DEV)
        assert int(too_long.sum()) >= 1
        assert bool(torch.isnan(short.best_sim[too_long]).all()) and bool((short.best_row[too_long] == -1).all())
        assert bool(torch.isnan(short.sims[too_long]).all())
        assert torch.equal(_i32(short.best_sim[~too_long]), _i32(got.best_sim[~too_long]))
        assert torch.equal(_i32(short.sims[~too_long]), _i32(got.sims[~too_long][..., :R]))
    # the same entries in another batch (another T) and at other list positions: the bits do not depend on placement
    sub = [5, 2, 3]
    pq2 = amd.pack_queries([c["qs"][i] for i in sub], DEV, layout="flat")
    perm = torch.tensor([6, 0, 3, 5, 1, 4, 2], device=DEV)
    other = amd.residual_wide_align(pq2, rc, dids[sub][:, perm].contiguous(), maps=True)
    T2 = max(QUERY_LENS[i] for i in sub)
    assert other.best_sim.shape == (3, N_COLS, T2)
    assert torch.equal(_i32(other.best_sim), _i32(got.best_sim[sub][:, perm][:, :, :T2]))
    assert torch.equal(other.best_row, got.best_row[sub][:, perm][:, :, :T2])
    assert torch.equal(_i32(other.sims), _i32(got.sims[sub][:, perm][:, :, :T2]))
    # a host list and a dense device box are packed as align packs them
    host = amd.residual_wide_align([c["qs"][3], c["qs"][2]], rc, dids[[3, 2]])
    assert torch.equal(_i32(host.best_sim[0, :, :17]), _i32(got.best_sim[3, :, :17]))
    assert torch.equal(_i32(host.best_sim[1, :, :16]), _i32(got.best_sim[2, :, :16]))
    box = torch.zeros((2, 40, W), dtype=TORCH_DT[dt])
    box[0, :17], box[1, :16] = c["qs"][3], c["qs"][2]
    dense = amd.residual_wide_align(box.to(DEV), rc, dids[[3, 2]])
    assert torch.equal(_i32(dense.best_sim[0, :, :17]), _i32(got.best_sim[3, :, :17]))
    assert torch.equal(dense.best_row[1, :, :16], got.best_row[2, :, :16])


def test_no_query_at_all_returns_before_a_pointer_is_looked_at(amd):
    L = amd._lib.lib()
    assert L.msim_res_wide_align_candidates(0, 0, 0, 0, 0, 0, 0, 0, 0, 256, 0, 2, 0, 0, 5, 0, W, 0, 3, 3, 0, 0, 0, 0, 4, 0) == 0
    assert L.msim_res_wide_gather_pages(0, 0, 0, 0, 256, 0, 2, W, 0, 0, 5, 0, 0, 0, 4, 0, 0, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- 2. the numbers
@pytest.mark.parametrize("K,bits,dt", CASES)
def test_best_sim_and_best_row_against_the_float64_maxsim_of_the_truths_rows(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc = c["rc"]
    rows = sum(PAGE_LENS)
    codes = rc.codes.cpu().view(torch.int16).numpy().view(np.uint16)[:rows]
    xhat_bits = wt.decode(rc.centroids.float().cpu().numpy(), codes, rc.residuals.cpu().numpy()[:rows], rc.weights.cpu().numpy(), bits, dt)
    xhat = wt.from_bits(xhat_bits, dt).astype(np.float64)
    Q = c["pq"].tokens.float().cpu().numpy()[:sum(QUERY_LENS)].astype(np.float64)
    q_off = np.concatenate([[0], np.cumsum(QUERY_LENS)])
    got = amd.residual_wide_align(c["pq"], rc, c["dids"])
    bs, br = got.best_sim.cpu().numpy().astype(np.float64), got.best_row.cpu().numpy()
    checked = rows_checked = 0
    worst = 0.0
    for q in range(len(QUERY_LENS)):
        a, b = q_off[q], q_off[q + 1]
        L = b - a
        for j in range(N_COLS):
            where = f"entry ({q}, {j})"
            gid = int(c["ids"][q, j])
            assert (bs[q, j, L:] == 0.0).all() and (br[q, j, L:] == -1).all(), where
            page = gid - ID_BASE
            if gid < 0 or not 0 <= page < len(PAGE_LENS):
                assert np.isneginf(bs[q, j, :L]).all() and (br[q, j, :L] == -1).all(), where
                continue
            n, flagged = PAGE_LENS[page], bool(c["clamp"][page])
            if n == 0:
                assert (bs[q, j, :L] == (0.0 if flagged else -np.inf)).all() and (br[q, j, :L] == -1).all(), where
                continue
            X = xhat[c["d_off"][page]:c["d_off"][page + 1]]
            S = Q[a:b] @ X.T
            B = 320 * 2.0**-24 * (np.abs(Q[a:b]) @ np.abs(X).T)            # the bound of every similarity
            for i in range(L):
                v, r = bs[q, j, i], int(br[q, j, i])
                M, Bi = S[i].max(), B[i].max()
                if r == -1:                                                # the zero padding row won: under the flag only
                    assert flagged and v == 0.0 and M <= Bi, where
                    continue
                assert 0 <= r < n and not (flagged and M < -Bi), where
                assert abs(v - S[i, r]) <= B[i, r] and abs(v - M) <= Bi, where + f" token {i}: {v} vs {M}"
                worst = max(worst, abs(v - M) / Bi)
                top = np.sort(S[i])[::-1]
                if n == 1 or top[0] - top[1] > Bi:
                    assert r == int(np.argmax(S[i])), where + f" token {i}: row {r}"
                    rows_checked += 1
                checked += 1
    print(f"    K={K} bits={bits} {dt}: {checked} similarities, largest error / bound {worst:.3f}, {rows_checked} rows compared")
    assert checked > 600 and rows_checked > checked // 2


# ---------------------------------------------------------------------------------------------------------------- 3. a bad code
@pytest.mark.parametrize("K,bits,dt,code", [(256, 2, "bf16", 256), (2048, 4, "f16", 2048), (2048, 2, "bf16", 65535), (256, 4, "f16", 65535)])
def test_a_code_beyond_k_is_a_nan_row_and_never_an_address(amd, K, bits, dt, code):
    """The guard, not a fault: the planted code is compared with K and the row read is row 0 of the centroids."""
    c = _case(amd, K, bits, dt)
    rc = c["rc"]
    page = PAGE_LENS.index(48)
    local = 20                                                             # chunk 1 of 3, row 4 of it
    row = int(c["d_off"][page]) + local
    codes = rc.codes.clone()
    codes.view(torch.int16)[row] = code if code < 32768 else code - 65536
    bad = amd.ResidualWideCorpus(rc.centroids, codes, rc.residuals, rc.cutoffs, rc.weights, rc.offsets, rc.clamp0, rc.lengths, rc.id_base,
                                 bits)
    dec = bad.decompress()
    assert (_i16(dec.blob[row]).cpu().numpy().view(np.uint16) == NAN16[dt]).all()
    got = amd.residual_wide_align(c["pq"], bad, c["dids"], maps=True)
    want = amd.align(c["pq"], dec, c["dids"], maps=True)
    for a, b in ((got.best_sim, want.best_sim), (got.sims, want.sims)):
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(_i32(torch.nan_to_num(a, nan=3.0)), _i32(torch.nan_to_num(b, nan=3.0)))
    assert torch.equal(got.best_row, want.best_row) and torch.equal(got.ids, want.ids)
    lists = (c["ids"] == ID_BASE + page).to(DEV)
    assert int(lists.sum()) >= 1
    sims = got.sims.cpu()
    for q, j in lists.nonzero().tolist():                                   # NaN in the row's column for every token, there alone
        assert bool(torch.isnan(sims[q, j, :QUERY_LENS[q], local]).all()), (q, j)
        assert not bool(torch.isnan(torch.cat([sims[q, j, :, :local], sims[q, j, :, local + 1:]], dim=1)).any()), (q, j)
    good = c["want"]                                                        # every other entry keeps its bits
    assert torch.equal(_i32(got.best_sim[~lists]), _i32(good.best_sim[~lists])) and torch.equal(_i32(got.sims[~lists]), _i32(good.sims[~lists]))
    # the gather: the NaN row of the decoder, every other byte as before
    ids = torch.tensor([[ID_BASE + page, -1], [ID_BASE + 3, ID_BASE + page]], dtype=torch.int64, device=DEV)
    box, lens = amd.residual_wide_gather_pages(bad, ids)
    wbox, wlens = amd.gather_pages(dec, ids)
    assert torch.equal(_i16(box), _i16(wbox)) and torch.equal(lens, wlens)
    assert bool((_i16(box[0, 0, local]).cpu().numpy().view(np.uint16) == NAN16[dt]).all())
    clean, _ = amd.residual_wide_gather_pages(rc, ids)
    keep = torch.ones(100, dtype=torch.bool)
    keep[local] = False
    assert torch.equal(_i16(box[:, :, keep.to(DEV)]), _i16(clean[:, :, keep.to(DEV)]))


# ---------------------------------------------------------------------------------------------------------------- 4. tail masking
FAR_LENS = [17, 33, 0, 1, 16, 33, 17]
FAR_WINNERS = {5: 0, 6: 15}                                                 # elsewhere the planted row is the page's LAST row


def _far_case(amd, planted, dtype, seed=29):
    """Every similarity negative (tests/helpers.py): queries at +0.7 u, page rows at -0.7 u.  The codec decodes the rows exactly: the
    weights table is all zeros and every page row is a copy of a centroid -- 250 far-side centroids, plus 6 on the queries' side for
    the planted winners.  planted: one +0.7 u row per page, at its last row (the pages of 17 and 33 rows: row 0 of the last chunk,
    whose other 15 rows re-read it) except the two pages of FAR_WINNERS.  Without the mask a zero-filled tail row (0 > every
    similarity) would win every token of the all-negative pages, and the duplicates of a planted last row would fill the map's
    columns past the page's end."""
    g = torch.Generator().manual_seed(seed)
    u = far_side_axis(W, g)
    C = torch.cat([far_side_rows(250, u, -1, g, dtype), far_side_rows(6, u, +1, g, dtype)])
    qs = [far_side_rows(n, u, +1, g, dtype) for n in (1, 17, 65, 128)]
    ps, winners = [], []
    for c, n in enumerate(FAR_LENS):
        p = C[torch.randint(0, 250, (n,), generator=g)].clone()
        w = -1
        if planted and n:
            w = FAR_WINNERS.get(c, n - 1)
            p[w] = C[250 + int(torch.randint(0, 6, (1,), generator=g))]
        ps.append(p)
        winners.append(w)
    corpus = amd.pack_passages(ps, DEV, batch_size=None, id_base=ID_BASE)
    cutoffs = torch.tensor([-0.5, 0.0, 0.5], device=DEV)
    weights = torch.zeros(4, device=DEV)
    rc = amd.ResidualWideCorpus.build(corpus, index=amd.CentroidWideIndex.build(corpus, centroids=C.to(DEV)), bits=2, cutoffs=cutoffs,
                                      weights=weights)
    return qs, ps, winners, rc


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("planted", [False, True], ids=["all-negative", "planted"])
def test_rows_past_the_page_end_are_masked_not_zero_filled(amd, planted, dt):
    qs, ps, winners, rc = _far_case(amd, planted, TORCH_DT[dt])
    n = len(ps)
    assert FAR_LENS[0] == 17 and FAR_LENS[1] == 33 and (not planted or (winners[0], winners[1]) == (16, 32))
    d_off = np.concatenate([[0], np.cumsum(FAR_LENS)])
    rows = int(d_off[-1])
    codes = rc.codes.cpu().view(torch.int16).numpy().view(np.uint16)[:rows]
    xhat_bits = wt.decode(rc.centroids.float().cpu().numpy(), codes, rc.residuals.cpu().numpy()[:rows], rc.weights.cpu().numpy(), 2, dt)
    np.testing.assert_array_equal(xhat_bits, torch.cat(ps).view(torch.int16).numpy().view(np.uint16))      # decoded rows ARE the rows
    xhat = wt.from_bits(xhat_bits, dt).astype(np.float64)
    Q = torch.cat(qs).double().numpy()
    S = Q @ xhat.T
    # the precondition, on the float64 truth of the decoded rows, before any output is read
    for c in range(n):
        if not FAR_LENS[c]:
            continue
        page = S[:, d_off[c]:d_off[c + 1]]
        if planted:
            w = winners[c]
            assert (page.argmax(axis=1) == w).all() and page[:, w].min() >= SIGN_MARGIN
            assert np.delete(page, w, axis=1).max(initial=-1.0) <= -SIGN_MARGIN
        else:
            assert page.max(axis=1).max() <= -SIGN_MARGIN                  # every per-token maximum
    pq = amd.pack_queries(qs, DEV, layout="flat")
    ids = (torch.arange(n, device=DEV) + ID_BASE).expand(len(qs), n)
    got = amd.residual_wide_align(pq, rc, ids, maps=True)
    _same_alignment(got, amd.align(pq, rc.decompress(), ids, maps=True))
    bs, br, sims = got.best_sim.cpu().numpy().astype(np.float64), got.best_row.cpu().numpy(), got.sims.cpu().numpy()
    q_off = np.concatenate([[0], np.cumsum([int(q.shape[0]) for q in qs])])
    for q in range(len(qs)):
        a, b = q_off[q], q_off[q + 1]
        for c in range(n):
            if not FAR_LENS[c]:
                assert np.isneginf(bs[q, c, :b - a]).all() and (br[q, c, :b - a] == -1).all()
                continue
            page = S[a:b, d_off[c]:d_off[c + 1]]
            bound = 320 * 2.0**-24 * (np.abs(Q[a:b]) @ np.abs(xhat[d_off[c]:d_off[c + 1]]).T).max(axis=1)
            assert (np.abs(bs[q, c, :b - a] - page.max(axis=1)) <= bound).all(), (q, c)      # a leaked zero is >= 0.05 away
            if planted:
                assert (br[q, c, :b - a] == winners[c]).all(), (q, c)
            else:
                assert (bs[q, c, :b - a] <= -SIGN_MARGIN / 2).all(), (q, c)
            assert np.isneginf(sims[q, c, :, FAR_LENS[c]:]).all()           # the columns past the page's end, the padded chunk rows included


# ---------------------------------------------------------------------------------------------------------------- 5. gather
def _gather_ids():
    """[4, 3]: listed pages with the 0-row page (slot 0) and the 100-row page among them, -1, ids below and above the shard"""
    ids = torch.tensor([[6, 0, 3], [-1 - ID_BASE, 9, 5], [7, ID_BASE + 10**9, 8], [-2 * ID_BASE + 3, 1, 11]], dtype=torch.int64) + ID_BASE
    assert int(ids[1, 0]) == -1 and int(ids[3, 0]) == 3 - ID_BASE
    return ids


@pytest.mark.parametrize("K,bits,dt", CASES)
def test_gather_has_the_bytes_of_gather_pages_over_the_decompressed_shard(amd, K, bits, dt):
    c = _case(amd, K, bits, dt)
    rc, dec = c["rc"], c["dec"]
    ids = _gather_ids()
    dids = ids.to(DEV)
    for pad_to in (None, 100, 120, 0):                                      # the longest listed page, equal, above, nothing
        shape = (4, 3, 100 if pad_to is None else pad_to, W)
        out = torch.full(shape, 7.0, dtype=TORCH_DT[dt], device=DEV)        # a nonzero pattern: every byte is written
        box, lens = amd.residual_wide_gather_pages(rc, dids, pad_to, out=out)
        wbox, wlens = amd.gather_pages(dec, dids, pad_to)
        assert box.data_ptr() == out.data_ptr() and box.shape == shape and box.dtype == TORCH_DT[dt] and lens.dtype == torch.int32
        assert torch.equal(_i16(box), _i16(wbox)) and torch.equal(lens, wlens)
        if pad_to != 0:
            hbox, hlens = amd.residual_wide_gather_pages(rc, ids, pad_to)   # host ids: checked against the lengths, then the same call
            assert torch.equal(_i16(hbox), _i16(box)) and torch.equal(hlens, lens)
    box, lens = amd.residual_wide_gather_pages(rc, dids)
    assert lens.cpu().tolist() == [[100, 0, 16], [0, 48, 33], [32, 0, 2], [0, 1, 31]]
    assert float(box[0, 0].float().abs().max()) > 0 and not bool(box[0, 1].any()) and not bool(box[1, 0].any()) and not bool(box[0, 2, 16:].any())
    assert not bool(box[2, 1].any()) and not bool(box[3, 0].any())          # off the shard, above and below
    # below the longest listed page: device ids truncate (and say so in lengths), host ids raise
    for pad_to in (40, 33, 1):
        out = torch.full((4, 3, pad_to, W), -3.0, dtype=TORCH_DT[dt], device=DEV)
        box, lens = amd.residual_wide_gather_pages(rc, dids, pad_to, out=out)
        wbox, wlens = amd.gather_pages(dec, dids, pad_to)
        assert torch.equal(_i16(box), _i16(wbox)) and torch.equal(lens, wlens) and int(lens.max()) == pad_to
        with pytest.raises(ValueError, match="pad_to"):
            amd.residual_wide_gather_pages(rc, ids, pad_to)
    # out=: the wrong shape, dtype or layout is refused
    out = torch.full((4, 3, 120, W), 7.0, dtype=TORCH_DT[dt], device=DEV)
    for wrong in (out[:, :, :100], out.float(), out.transpose(0, 1)):
        with pytest.raises(ValueError):
            amd.residual_wide_gather_pages(rc, dids, 120, out=wrong)
    # a scalar list and the dispatch of gather_pages on the container
    one, one_len = amd.gather_pages(rc, dids[0, 0])
    assert one.shape == (100, W) and int(one_len) == 100 and torch.equal(_i16(one), _i16(amd.gather_pages(dec, dids[0, 0])[0]))


# ---------------------------------------------------------------------------------------------------------------- 6. routing
def test_align_and_gather_pages_dispatch_and_the_retriever_opts_in(amd):
    c = _case(amd, 256, 4, "bf16")
    rc, pq, dids = c["rc"], c["pq"], c["dids"]
    _same_alignment(amd.align(pq, rc, dids, maps=True), c["want"], "align(rc): ")
    _same_alignment(amd.align(pq, rc, dids, maps=True, max_rows=64), amd.align(pq, c["dec"], dids, maps=True, max_rows=64), "align(rc, max_rows): ")
    box, lens = amd.gather_pages(rc, dids, 50)
    wbox, wlens = amd.gather_pages(c["dec"], dids, 50)
    assert torch.equal(_i16(box), _i16(wbox)) and torch.equal(lens, wlens)
    for r in (amd.ShardedRetriever(rc), amd.ShardedRetriever(rc, score_fn=amd.residual_wide_scores)):
        with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only") as e:
            r.align(pq, dids)
        assert "score_fn=residual_wide_scores" in str(e.value) and "align_fn=residual_align" not in str(e.value)
    r = amd.ShardedRetriever(rc, align_fn=amd.residual_wide_align, force_collective=True)
    ref = amd.ShardedRetriever(c["dec"], force_collective=True)
    _same_alignment(r.align(pq, dids, maps=True), ref.align(pq, dids, maps=True), "retriever: ")
    _same_alignment(r.align(c["qs"][1:4], dids[1:4]), ref.align(c["qs"][1:4], dids[1:4]), "retriever, host list: ")
    # the sibling classes refuse each other, naming the width
    g = torch.Generator().manual_seed(3)
    C128 = torch.nn.functional.normalize(torch.randn(256, 128, generator=g), dim=-1).to(torch.bfloat16)
    narrow_pages = amd.pack_passages([C128[:5].clone(), C128[5:8].clone()], DEV, batch_size=None, id_base=ID_BASE)
    narrow = amd.ResidualCorpus.build(narrow_pages, index=amd.CentroidIndex.build(narrow_pages, centroids=C128.to(DEV)), bits=2)
    q128 = amd.pack_queries([C128[:4].clone()], DEV, layout="flat")
    one = torch.tensor([[ID_BASE]], dtype=torch.int64, device=DEV)
    with pytest.raises(NotImplementedError, match="width 320"):
        amd.residual_wide_align(q128, narrow, one)
    with pytest.raises(NotImplementedError, match="width 320"):
        amd.residual_wide_gather_pages(narrow, one)
    with pytest.raises(NotImplementedError, match="width 128"):
        amd.residual_align(pq, rc, dids)
    # Alignment.similarity_maps works on the result
    al = amd.residual_wide_align(pq, rc, dids, maps=True)
    q, j = next((q, j) for q in (4, 5, 6) for j in (0, 1, 4, 6) if PAGE_LENS[int(c["ids"][q, j]) - ID_BASE] > 0)
    n = PAGE_LENS[int(c["ids"][q, j]) - ID_BASE]
    maps = al.similarity_maps(q, j, (n, 1))
    assert maps.shape == (QUERY_LENS[q], n, 1) and torch.equal(_i32(maps[:, :, 0]), _i32(c["want"].sims[q, j, :QUERY_LENS[q], :n]))


def test_mined_negatives_are_gathered_without_a_decompressed_shard(amd):
    c = _case(amd, 256, 2, "bf16")
    rc, dec = c["rc"], c["dec"]
    pq = amd.pack_queries(c["qs"], DEV)
    positives = torch.tensor([[ID_BASE + 2, -1], [ID_BASE + 5, ID_BASE + 11], [-1, -1], [ID_BASE + 7, -1], [ID_BASE + 1, ID_BASE + 9],
                              [ID_BASE + 4, -1], [ID_BASE + 10, ID_BASE + 6]], device=DEV)
    results = []
    for corpus in (rc, dec):                                                # ragged queries: both scans run the flat kernel
        neg_s, neg_i = amd.mine_hard_negatives(pq, corpus, positives, 3)
        box, blens = amd.gather_pages(corpus, neg_i)
        results.append((neg_s, neg_i, box, blens))
    neg_i = results[0][1]
    assert bool((neg_i[1:] >= 0).any()) and neg_i.shape == (len(QUERY_LENS), 3) and results[0][2].shape == (len(QUERY_LENS), 3, 100, W)
    assert float(results[0][2].float().abs().max()) > 0
    for a, b in zip(*results):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


# ---------------------------------------------------------------------------------------------------------------- 7. capture
def test_captured_calls_replay_the_eager_bits(amd):
    c = _case(amd, 2048, 4, "bf16")
    rc, pq, dids = c["rc"], c["pq"], c["dids"]
    gids = _gather_ids().to(DEV)

    def fn():
        al = amd.residual_wide_align(pq, rc, dids, maps=True)
        box, lens = amd.residual_wide_gather_pages(rc, gids, 60)
        return al.best_sim, al.best_row, al.sims, box, lens

    want = (c["want"].best_sim, c["want"].best_row, c["want"].sims, *amd.gather_pages(c["dec"], gids, 60))
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
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(captured, want):
            assert got.shape == ref.shape and torch.equal(_bytes(got), _bytes(ref))
