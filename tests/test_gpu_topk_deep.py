"""GPU: the deep top-k (1024 < k <= 8192, msim_topk_deep_f32) behind `topk`, bit-exact against the oracle ranking
(oracle/topk_oracle.py: score descending, id ascending) -- at the edges of k and n in both launch forms, on every kind of row, with
every radix digit deciding, with explicit ids whose high bytes decide, against the k <= 1024 kernels on the same matrices, as the
in-place message of `shard_topk`, captured in a graph, past 2^32 bytes, and through every route of `search` that selects.
Every comparison is on ids and score bits."""
import numpy as np
import pytest
import torch

from oracle import topk_oracle

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _bits(x):
    return (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, dtype=np.float32)).view(np.int32)


def _same(got, want):
    """(scores, ids) against (scores, ids): ids first (the clearer message), then the score bits"""
    np.testing.assert_array_equal(got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else got[1],
                                  want[1].cpu().numpy() if isinstance(want[1], torch.Tensor) else want[1])
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]))


def _split(amd, n_q, n, k):
    """the plan's launch form for implicit ids: split rows count into a workspace, one workgroup per row needs none"""
    return amd._lib.lib().msim_topk_deep_workspace_bytes(n_q, n, k) > 0


def _check(amd, s, k, id_base=1000, ids=None):
    got = amd.topk(s.to(DEV), k, id_base, None if ids is None else ids.to(DEV))
    assert got[0].shape == got[1].shape == (s.shape[0], k)
    _same(got, topk_oracle.topk(s.numpy(), k, id_base, None if ids is None else ids.numpy()))


# --------------------------------------------------------------------------------------------------------- edges of k and n
EDGES = [(1, 1025, 1025), (2, 1500, 1025), (3, 8192, 8192), (2, 8193, 8192), (1, 5000, 8192), (1, 1, 2000), (2, 0, 1100),
         (4, 125000, 4096), (300, 20000, 2048)]


@pytest.mark.parametrize("n_q,n,k", EDGES)
def test_edges_of_k_and_n(amd, n_q, n, k):
    g = torch.Generator().manual_seed(n + k)
    s = (torch.randn(n_q, n, generator=g) * 8).round() / 8            # T always sits inside a crowded bucket
    _check(amd, s, k)


def test_both_launch_forms_are_reached(amd):
    forms = [_split(amd, *c) for c in EDGES]
    assert forms == [False] * 7 + [True, False]
    assert _split(amd, 2, 40001, 3000) and _split(amd, 5, 33000, 2500) and _split(amd, 3, 40000, 3000)
    assert not _split(amd, 8600, 125000, 1100)


def test_rows_off_the_16_byte_grid(amd):
    g = torch.Generator().manual_seed(40001)
    wide = ((torch.randn(2, 40003, generator=g) * 8).round() / 8).to(DEV)
    view = wide[:, :40001]                                            # ld = 40003: row 1 starts 12 bytes off the grid
    assert view.stride(0) == 40003
    _same(amd.topk(view, 3000, 1000), topk_oracle.topk(view.cpu().numpy(), 3000, 1000))
    ids = torch.arange(40003, dtype=torch.int64).flip(0).repeat(2, 1).to(DEV)[:, :40001]
    _same(amd.topk(view, 3000, 0, ids), topk_oracle.topk(view.cpu().numpy(), 3000, 0, ids.cpu().numpy()))


# ---------------------------------------------------------------------------------------------------------------- data kinds
def test_every_kind_of_row(amd):
    n_q, n, k = 5, 33000, 2500
    g = torch.Generator().manual_seed(7)
    kinds = {}
    kinds["constant"] = torch.full((n_q, n), 3.25)                    # ids decide everything: the first k columns win
    kinds["ascending"] = torch.arange(n, dtype=torch.float32).repeat(n_q, 1) + torch.arange(n_q, dtype=torch.float32)[:, None]
    kinds["descending"] = -torch.arange(n, dtype=torch.float32).repeat(n_q, 1)
    s = torch.randn(n_q, n, generator=g)
    s[0, :] = float("-inf")                                           # a row of all -inf: the first k ids, each with -inf
    s[1, 2000:] = float("-inf")                                       # fewer than k finite scores: -inf entries with their real ids
    s[2, ::3] = float("-inf")
    kinds["inf"] = s
    z = torch.randn(n_q, n, generator=g)
    z[0, 1200:] = torch.where(torch.arange(n - 1200) % 2 == 0, 0.0, -0.0)    # T = 0: zeros of both signs on both sides of the cut
    z[1] = torch.where(torch.arange(n) % 2 == 0, 0.0, -0.0)
    z[2, :] = -z[2].abs()
    z[2, 5::7] = -0.0
    z[2, 6::7] = 0.0
    kinds["zeros"] = z
    e = torch.randn(n_q, n, generator=g)
    e[0, ::5] = 3.0e38
    e[1, ::5] = -3.0e38
    e[2, ::2] = 3.0e38
    e[2, 1::2] = -3.0e38
    kinds["extremes"] = e
    magnitudes = torch.randint(1, 1 << 14, (n_q, n), generator=g).numpy().astype(np.uint32)      # subnormal bit patterns, many ties
    sub = torch.from_numpy(magnitudes.view(np.float32).copy())
    sub[:, ::2] = -sub[:, ::2]
    kinds["subnormal"] = sub
    assert float(sub.abs().max()) < 1.2e-38 and float(sub.abs().max()) > 0
    assert _split(amd, n_q, n, k)
    for name, rows in kinds.items():
        got = amd.topk(rows.to(DEV), k, 1000)
        want = topk_oracle.topk(rows.numpy(), k, 1000)
        np.testing.assert_array_equal(got[1].cpu().numpy(), want[1], err_msg=name)
        np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg=name)
        # ... and the same rows through the other launch form (many rows: one workgroup each)
        many = rows.repeat(26, 1)
        assert not _split(amd, many.shape[0], n, k)
        got = amd.topk(many.to(DEV), k, 1000)
        for rep in (0, 25):
            np.testing.assert_array_equal(got[1][rep * n_q:(rep + 1) * n_q].cpu().numpy(), want[1], err_msg=name)
            np.testing.assert_array_equal(_bits(got[0][rep * n_q:(rep + 1) * n_q]), _bits(want[0]), err_msg=name)
    c = amd.topk(kinds["constant"].to(DEV), k, 1000)[1].cpu()
    assert torch.equal(c, torch.arange(1000, 1000 + k).repeat(n_q, 1))


@pytest.mark.parametrize("n,k", [(4096, 1500), (4096, 2049), (16384, 2049)])
def test_every_digit_decides(amd, n, k):
    """scores whose bit patterns differ in one byte only, and their negatives: a pass that drops or misorders a digit changes the set"""
    rng = np.random.default_rng(n + k)
    rows = []
    for step in (1, 1 << 8, 1 << 16):
        bits = (0x3F800000 + np.arange(n, dtype=np.int64) * step).astype(np.uint32)
        assert int(bits.max()) < 0x7F800000
        for sign in (0, 0x80000000):
            rows.append(rng.permutation(bits | np.uint32(sign)).view(np.float32))
    s = torch.from_numpy(np.stack(rows))
    assert _split(amd, 6, n, k) == (n == 16384)
    _check(amd, s, k)


# -------------------------------------------------------------------------------------------------------------- explicit ids
@pytest.mark.parametrize("n_q,n,k", [(3, 6000, 1100), (2, 65536, 8192), (200, 9000, 4096)])
def test_explicit_ids(amd, n_q, n, k):
    g = torch.Generator().manual_seed(n_q + n)
    s = (torch.randn(n_q, n, generator=g) * 8).round() / 8
    base = torch.stack([torch.randperm(n, generator=g) for _ in range(n_q)])
    ids = base + torch.where(base % 3 == 0, 1 << 32, 0) + torch.where(base % 5 == 0, 1 << 40, 0)    # the high id digits decide
    ids[torch.rand(n_q, n, generator=g) < 0.1] = -1                                               # no entry
    s[0, :] = 0.75                                                    # ties resolved by id, not by column
    # row 1: the ties at T differ in the top id byte only; k - 64 entries rank above them, so 64 of the 128 get in
    s[1, :] = -5.0
    s[1, : k - 64] = 9.0
    s[1, k - 64: k + 64] = 2.5
    ids[1] = base[1] + (1 << 20)
    ids[1, k - 64: k + 64] = (torch.randperm(128, generator=g) << 56) + 7
    _check(amd, s, k, 0, ids)


def test_a_listed_twice_entry_may_appear_twice(amd):
    """the same (score, id) more than once at the threshold: interchangeable entries, the count is what matters"""
    s = torch.full((1, 3000), 1.0)
    ids = torch.arange(3000, dtype=torch.int64).reshape(1, 3000) // 3
    _check(amd, s, 1100, 0, ids)


# ------------------------------------------------------------------------------------------------------------ old against new
def _abi(amd, entry, ws_bytes, s, ids, k, id_base):
    from colpali_amd import _lib

    n_q, n = s.shape
    out_s = torch.empty((n_q, k), dtype=torch.float32, device=DEV)
    out_i = torch.empty((n_q, k), dtype=torch.int64, device=DEV)
    ws = _lib.workspace(ws_bytes(n_q, n, k), DEV)
    rc = entry(_lib.ptr(s), _lib.ptr(ids), n_q, n, s.stride(0), k, id_base, _lib.ptr(out_s), _lib.ptr(out_i), _lib.ptr(ws),
               _lib.current_stream_handle(DEV))
    _lib.check(rc, "top-k")
    torch.cuda.synchronize()
    return out_s, out_i


@pytest.mark.parametrize("k", [1, 10, 256, 1024])
def test_the_old_entry_and_the_new_agree(amd, k):
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(k)
    s = ((torch.randn(4, 125000, generator=g) * 8).round() / 8).to(DEV)
    e = ((torch.randn(7, 5000, generator=g) * 8).round() / 8).to(DEV)
    ids = torch.stack([torch.randperm(5000, generator=g) for _ in range(7)]) + (1 << 33)
    ids[torch.rand(7, 5000, generator=g) < 0.1] = -1
    ids = ids.to(DEV)
    for scores, idl, base in ((s, None, 1000), (e, ids, 0)):
        old = _abi(amd, L.msim_topk_f32, L.msim_topk_workspace_bytes, scores, idl, k, base)
        new = _abi(amd, L.msim_topk_deep_f32, L.msim_topk_deep_workspace_bytes, scores, idl, k, base)
        _same(new, old)


def test_refusal_above_the_limit(amd):
    s = torch.zeros(2, 9000, device=DEV)
    with pytest.raises(NotImplementedError, match="8192"):
        amd.topk(s, 8193)


# ---------------------------------------------------------------------------------------------- in-place message and merge
class _FakeDist:
    """Stands in for torch.distributed inside one process: rank r's message is whatever virtual shard r produced."""

    def __init__(self, messages, me):
        self.messages, self.me = messages, me

    def all_gather_into_tensor(self, out, mine, group=None):
        self.messages[self.me] = mine.clone()
        out.copy_(torch.cat([m.reshape(-1) for m in self.messages]))


def test_shard_topk_writes_a_deep_message_in_place(amd):
    g = torch.Generator().manual_seed(21)
    n_q, n, k, world = 4, 9000, 2048, 3
    s = ((torch.randn(n_q, n, generator=g) * 8).round() / 8).to(DEV)
    full = amd.topk(s, k)
    _same(full, topk_oracle.topk(s.cpu().numpy(), k))
    nbytes = (n_q * k * 4 + 7) // 8 * 8 + n_q * k * 8
    messages = [torch.zeros(nbytes, dtype=torch.uint8, device=DEV) for _ in range(world)]
    spans = [amd.shard_range(n, world, r) for r in range(world)]
    for r, (lo, hi) in enumerate(spans):
        amd.shard_topk(s[:, lo:hi], k, lo, world, _FakeDist(messages, r))
    for r, (lo, hi) in enumerate(spans):
        _same(amd.shard_topk(s[:, lo:hi], k, lo, world, _FakeDist(messages, r)), full)      # the merge row: world x k explicit ids


# -------------------------------------------------------------------------------------------------------------------- capture
def test_a_captured_deep_topk_follows_the_scores(amd):
    g = torch.Generator().manual_seed(31)
    first, second, third = ((torch.randn(3, 40000, generator=g) * 8).round() / 8 for _ in range(3))
    assert _split(amd, 3, 40000, 3000)                                # the form that counts into its workspace
    s = first.to(DEV)
    amd.topk(s, 3000)                                                 # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = amd.topk(s, 3000, 1000)
    for data in (second, third):
        s.copy_(data)                                                 # in place: the graph holds the tensor's address
        graph.replay()
        torch.cuda.synchronize()
        _same(out, topk_oracle.topk(data.numpy(), 3000, 1000))


# ------------------------------------------------------------------------------------------------------------ past 2^32 bytes
def test_a_matrix_past_4_gib(amd):
    n_q, n, k = 8600, 125000, 1100
    assert n_q * n * 4 > 1 << 32
    torch.manual_seed(5)
    s = torch.randn(n_q, n, device=DEV)
    s.mul_(8).round_().div_(8)
    got_s, got_i = amd.topk(s, k, 1000)
    rows = [0, 4300, 8599]
    want = topk_oracle.topk(s[rows].cpu().numpy(), k, 1000)
    _same((got_s[rows], got_i[rows]), want)


# --------------------------------------------------------------------------------------------------------------------- routes
N_PAGES, ID_BASE = 3000, 100


def _unit(g, *shape):
    return torch.nn.functional.normalize(torch.randn(*shape, 128, generator=g), dim=-1).to(torch.bfloat16)


@pytest.fixture(scope="module")
def route(amd):
    g = torch.Generator().manual_seed(60)
    rows = _unit(g, N_PAGES, 8)
    pages = [rows[i] for i in range(N_PAGES)]
    corpus = amd.pack_passages(pages, DEV, batch_size=None, id_base=ID_BASE)
    q = _unit(g, 6, 16).to(DEV)
    return corpus, amd.Fp4Index.build(corpus), q, pages


def _ids_of(scores, k, id_base=ID_BASE, ids=None, no_page=False):
    """the oracle's selection of a device score matrix, as a device id list (-1 wherever the score is -inf when `no_page`)"""
    s, i = topk_oracle.topk(scores.cpu().numpy(), k, id_base, None if ids is None else ids.cpu().numpy())
    if no_page:
        i = np.where(np.isneginf(s), -1, i)
    return torch.from_numpy(i).to(DEV)


def test_search_deep_k(amd, route):
    corpus, _, q, _ = route
    r = amd.ShardedRetriever(corpus)
    _same(r.search(q, k=2500), topk_oracle.topk(amd.maxsim_scores(q, corpus).cpu().numpy(), 2500, ID_BASE))


def test_search_deep_candidate_list(amd, route):
    corpus, idx, q, _ = route
    r = amd.ShardedRetriever(corpus)
    want = amd.rerank(q, corpus, _ids_of(amd.fp4_scores(q, idx), 1500), 5)
    _same(r.search(q, k=5, prefilter=idx, n_candidates=1500), want)
    # candidates=: a caller's own deep list, and a deep k behind it
    lst = _ids_of(amd.fp4_scores(q, idx), 2600)
    s = amd.rerank(q, corpus, lst)                                    # (k=None: the scores, aligned with the list)
    _same(r.search(q, k=2200, candidates=lst), topk_oracle.topk(s.cpu().numpy(), 2200, 0, lst.cpu().numpy()))


def _cascade(amd, q, shard, first_scores, first_base, idx, m1, m2, k):
    c1 = _ids_of(first_scores, m1, first_base)
    fine_s, fine_i = amd.fp4_rerank_scores(q, idx, c1)
    c2 = _ids_of(fine_s, m2, 0, fine_i, no_page=True)
    return amd.rerank(q, shard, c2, k)


def test_search_three_stages(amd, route):
    corpus, idx, q, _ = route
    fde = amd.FdeIndex.build(corpus)
    r = amd.ShardedRetriever(corpus)
    want = _cascade(amd, q, corpus, amd.fde_scores(q, fde), ID_BASE, idx, 2800, 1200, 5)
    _same(r.search(q, k=5, prefilter=fde, n_candidates=2800, refine=idx, n_refine=1200), want)


@pytest.mark.parametrize("first", ["packed", "int8", "binary", "centroid"])
def test_search_every_other_first_stage(amd, route, first):
    corpus, _, q, pages = route
    if first == "packed":
        pre = amd.pack_passages([p.float().mean(0, keepdim=True).to(torch.bfloat16) for p in pages], DEV, batch_size=None, id_base=ID_BASE)
        coarse = amd.maxsim_scores(q, pre)
    elif first == "int8":
        pre = amd.Int8Index.build(corpus)
        coarse = amd.int8_scores(q, pre)
    elif first == "binary":
        pre = amd.BinaryIndex.build(corpus)
        coarse = amd.binary_scores(q, pre)
    else:
        pre = amd.CentroidIndex.build(corpus, n_centroids=256, iters=2)
        coarse = amd.centroid_scores(q, pre)
    want = amd.rerank(q, corpus, _ids_of(coarse, 1500), 5)
    _same(amd.ShardedRetriever(corpus).search(q, k=5, prefilter=pre, n_candidates=1500), want)


def test_search_a_residual_shard(amd, route):
    corpus, idx, q, _ = route
    rc = amd.ResidualCorpus.build(corpus, bits=2, n_centroids=256, iters=2)
    r = amd.ShardedRetriever(rc)
    want = _cascade(amd, q, rc, amd.centroid_scores(q, rc.index), ID_BASE, idx, 2800, 1200, 5)
    _same(r.search(q, k=5, prefilter=rc.index, n_candidates=2800, refine=idx, n_refine=1200), want)


def test_search_a_live_shard(amd, route):
    corpus, _, q, _ = route
    live = amd.LiveCorpus.from_packed(corpus, 64, 4)
    g = torch.Generator().manual_seed(61)
    dead = (torch.randperm(N_PAGES, generator=g)[:400] + ID_BASE).tolist()
    live.delete(dead)
    s, i = live.search(q, k=2700, prefilter=live.fp4_index(), n_candidates=2700)
    i = i.cpu().numpy()
    assert ((i >= 0).sum(1) == 2600).all() and (i[:, 2600:] == -1).all() and np.isneginf(s.cpu().numpy()[:, 2600:]).all()
    assert not np.isin(i, dead).any()
    # every live page was listed and reranked: the scan's scores of the live pages, in the project's order
    full = amd.maxsim_scores(q, corpus).cpu().numpy()
    full[:, np.asarray(dead) - ID_BASE] = -np.inf
    ws, wi = topk_oracle.topk(full, 2700, ID_BASE)
    wi = np.where(np.isneginf(ws), -1, wi)
    np.testing.assert_array_equal(i, wi)
    np.testing.assert_array_equal(_bits(s), _bits(ws))


def test_search_the_filter_mask_route(amd, route):
    corpus, _, q, _ = route
    g = torch.Generator().manual_seed(62)
    allowed = torch.rand(N_PAGES, generator=g) < 0.3
    assert 0 < int(allowed.sum()) < 1200
    flt = amd.PageFilter.from_mask(allowed.to(DEV), ID_BASE)
    s, i = amd.ShardedRetriever(corpus).search(q, k=1200, filter=flt, filter_route="mask")
    full = amd.maxsim_scores(q, corpus).cpu().numpy()
    full[:, ~allowed.numpy()] = -np.inf
    ws, wi = topk_oracle.topk(full, 1200, ID_BASE)
    wi = np.where(np.isneginf(ws), -1, wi)
    assert (i.cpu().numpy()[np.isneginf(s.cpu().numpy())] == -1).all()
    _same((s, i), (ws, wi))
