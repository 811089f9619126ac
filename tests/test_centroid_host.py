"""The centroid-code index without a GPU: the truth (tests/centroid_truth.py) against hand-worked cases, the constructor's and the
ABI's argument checks (no device work), and ShardedRetriever.search(prefilter=<CentroidIndex>) plumbing with the truth injected as
centroid_score_fn."""
import numpy as np
import pytest
import torch

from tests import centroid_truth as ct

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def _e(k, n=4, scale=1.0):
    C = np.zeros((n, 128), np.float32)
    C[np.arange(n), k] = scale
    return C


def test_truth_codes_by_hand():
    C = np.zeros((4, 128), np.float32)
    C[0, 0], C[1, 1], C[2, 1], C[3, 2] = 1, 1, 1, -1                  # centroids 1 and 2 are equal
    rows = np.zeros((5, 128), np.float32)
    rows[0, 0] = 2                                                     # e0 -> 0
    rows[1, 1] = 0.5                                                   # e1 -> 1: the lower of the two equal centroids
    rows[2, 2] = -3                                                    # -e2 -> 3
    rows[3, :3] = [0.25, 0.5, -0.125]                                  # sims 0.25, 0.5, 0.5, 0.125 -> 1
    # row 4 is zero: every similarity is 0, the lowest id wins
    np.testing.assert_array_equal(ct.codes(rows, C), np.array([0, 1, 3, 1, 0], np.uint16))
    assert ct.codes(rows, C).dtype == np.uint16
    np.testing.assert_array_equal(ct.encode_slack(rows[:1], C), [128 * 2.0**-23 * 2])


def test_truth_table_rounds_to_fp32_then_fp16():
    C = np.zeros((2, 128), np.float32)
    C[0, 0], C[1, 0], C[1, 1] = 1, 1 + 2.0**-10, 2.0**-13
    q = np.zeros((1, 128), np.float32)
    q[0, 0], q[0, 1] = 1, 1
    S = ct.table(q, C)
    assert S.dtype == np.float16 and S.shape == (1, 2)
    assert S[0, 0] == 1 and S[0, 1] == np.float16(1 + 2.0**-10)         # 1 + 2^-10 + 2^-13 rounds down to the fp16 grid


def test_truth_scores_by_hand():
    # table of 3 tokens x 4 centroids, all values exact in fp16
    S = np.array([[0.5, -0.25, 0.125, -1.0],
                  [-0.5, -0.25, -0.125, -2.0],
                  [1.0, 2.0, -4.0, 0.25]], np.float16)
    page_codes = np.array([0, 1, 3, 3, 2, 1, 1], np.uint16)
    d_off = np.array([0, 2, 2, 4, 7])                                   # pages: {0, 1}, {}, {3, 3}, {2, 1, 1}
    q_off = np.array([0, 2, 2, 3])                                      # queries: tokens {0, 1}, {}, {2}
    got = ct.scores(S, q_off, page_codes, d_off)
    want = np.array([[0.5 - 0.25, -np.inf, -1.0 - 2.0, 0.125 - 0.125],
                     [0.0, -np.inf, 0.0, 0.0],                            # a query of 0 tokens: 0 against every page that has rows
                     [2.0, -np.inf, 0.25, 2.0]], np.float32)
    np.testing.assert_array_equal(got, want)
    clamped = ct.scores(S, q_off, page_codes, d_off, clamp0=np.array([1, 1, 1, 0], np.uint8))
    want_c = want.copy()
    want_c[0, 0] = 0.5                                                  # max(-0.25, 0) = 0
    want_c[0, 2] = 0.0                                                  # both maxima negative
    np.testing.assert_array_equal(clamped, want_c)                     # the empty page stays -inf, flagged or not
    np.testing.assert_array_equal(ct.scores64(np.zeros((3, 128)), np.zeros((4, 128)), q_off, page_codes, d_off)[:, 1], [-np.inf] * 3)


def test_truth_all_negative_table_and_broken_code():
    S = -np.array([[0.5, 0.25], [1.0, 2.0]], np.float16)
    d_off = np.array([0, 1, 3])
    q_off = np.array([0, 2])
    got = ct.scores(S, q_off, np.array([0, 1, 0], np.uint16), d_off)
    np.testing.assert_array_equal(got, np.array([[-1.5, -0.25 - 1.0]], np.float32))          # never 0: maxima start at -inf
    flagged = ct.scores(S, q_off, np.array([0, 1, 0], np.uint16), d_off, clamp0=np.array([0, 1], np.uint8))
    np.testing.assert_array_equal(flagged, np.array([[-1.5, 0.0]], np.float32))
    broken = ct.scores(S, q_off, np.array([0, 2, 0], np.uint16), d_off)
    assert broken[0, 0] == np.float32(-1.5) and np.isnan(broken[0, 1])


def test_truth_sum_is_sequential_float32():
    S = np.array([[2048.0], [0.5], [0.5], [0.5], [0.5]], np.float16)[:, :1]
    S = np.concatenate([S, S], axis=1)
    got = ct.scores(S, np.array([0, 5]), np.array([0], np.uint16), np.array([0, 1]))
    assert got[0, 0] == np.float32(2050.0)
    big = np.array([[2.0**15], [2.0**-9], [2.0**-9]], np.float16)
    got = ct.scores(np.concatenate([big, big], axis=1), np.array([0, 3]), np.array([1], np.uint16), np.array([0, 1]))
    assert got[0, 0] == np.float32(2.0**15)                             # (2^15 + 2^-9) rounds back twice: a pairwise sum would not


def _index(shard, K=256, seed=5):
    from colpali_amd import CentroidIndex

    g = torch.Generator().manual_seed(seed)
    C = torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).to(torch.bfloat16)
    codes = ct.codes(shard.blob.float().numpy(), C.float().numpy())
    return CentroidIndex(C, torch.from_numpy(codes), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(), shard.id_base)


def _truth_fn(queries, index):
    qb = [x.float().numpy() for x in queries]
    S = ct.table(np.concatenate(qb), index.centroids.float().numpy())
    q_off = np.cumsum([0] + [len(x) for x in qb])
    c0 = None if index.clamp0 is None else index.clamp0.numpy()
    return torch.from_numpy(ct.scores(S, q_off, index.codes.numpy(), index.offsets.numpy(), c0))


def _shard(n=5, id_base=7, seed=0):
    import colpali_amd

    g = torch.Generator().manual_seed(seed)
    return colpali_amd.pack_passages([torch.randn(3 + i, 128, generator=g).to(torch.bfloat16) for i in range(n)], torch.device("cpu"),
                                     batch_size=None, id_base=id_base)


def test_constructor_validation():
    import colpali_amd

    shard = _shard()
    idx = _index(shard)
    assert len(idx) == 5 and idx.id_base == 7 and idx.n_centroids == 256 and idx.device.type == "cpu"
    assert idx.nbytes >= 256 * 256 + 2 * int(shard.blob.shape[0])
    C, codes, off, lens = idx.centroids, idx.codes, idx.offsets, idx.lengths
    with pytest.raises(ValueError):
        colpali_amd.CentroidIndex(C, codes.to(torch.int32), off, None, lens)
    with pytest.raises(ValueError):
        colpali_amd.CentroidIndex(C, codes.reshape(-1, 1), off, None, lens)
    with pytest.raises(ValueError):
        colpali_amd.CentroidIndex(C, codes, off[:-1], None, lens)
    with pytest.raises(ValueError):
        colpali_amd.CentroidIndex(C, codes, off.to(torch.int64), None, lens)
    with pytest.raises(ValueError):
        colpali_amd.CentroidIndex(C, codes, off, torch.zeros(4, dtype=torch.uint8), lens)
    for k in (0, 128, 300, 2304, 4096):                                # K outside the rule
        with pytest.raises(ValueError):
            colpali_amd.CentroidIndex(torch.zeros(k, 128, dtype=torch.bfloat16), codes, off, None, lens)
    with pytest.raises(NotImplementedError):                           # fp32 centroids
        colpali_amd.CentroidIndex(C.float(), codes, off, None, lens)
    with pytest.raises(NotImplementedError):                           # width 320
        colpali_amd.CentroidIndex(torch.zeros(256, 320, dtype=torch.bfloat16), codes, off, None, lens)


def test_cpu_devices_are_refused():
    import colpali_amd
    from colpali_amd import centroid

    shard = _shard()
    idx = _index(shard)
    with pytest.raises(RuntimeError):
        colpali_amd.CentroidIndex.build(shard, centroids=idx.centroids)
    with pytest.raises(RuntimeError):
        colpali_amd.train_centroids(shard, 256)
    with pytest.raises(RuntimeError):
        colpali_amd.centroid_scores([torch.randn(4, 128).to(torch.bfloat16)], idx)
    for k in (100, 255, 2049, 4096):
        with pytest.raises(ValueError):
            colpali_amd.train_centroids(shard, k)
        with pytest.raises(ValueError):
            centroid._check_k(k)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()

    def enc(dtype=0, x=FAKE, off=FAKE, n=3, rows=40, dim=128, longest=20, c=FAKE, k=256, codes=FAKE, status=None):
        return L.msim_cent_encode_docs(dtype, x, off, n, rows, dim, longest, c, k, codes, status, None)

    def tab(dtype=0, x=FAKE, qo=FAKE, n_q=4, q_rows=40, maxq=32, dim=128, c=FAKE, k=256, table=FAKE):
        return L.msim_cent_table(dtype, x, qo, n_q, q_rows, maxq, dim, c, k, table, None)

    def score(table=FAKE, qo=FAKE, n_q=4, q_rows=40, maxq=32, k=256, codes=FAKE, do=FAKE, c0=None, n_d=10, d_rows=90, out=FAKE, ld=10):
        return L.msim_cent_scores(table, qo, n_q, q_rows, maxq, k, codes, do, c0, n_d, d_rows, out, ld, None)

    # nothing to do: 0 before any pointer is looked at
    assert enc(n=0) == 0 and enc(n=0, x=None, off=None, c=None, codes=None) == 0 and enc(longest=0, x=None, off=None, c=None) == 0
    assert tab(n_q=0) == 0 and tab(n_q=0, x=None, qo=None, c=None, table=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, table=None, codes=None, out=None) == 0
    assert L.msim_cent_table_bytes(3, 33, 512) == 3 * 2 * 512 * 64 and L.msim_cent_table_bytes(2, 0, 256) == 2 * 256 * 64
    for kw in (dict(n=-1), dict(rows=-1), dict(longest=-1), dict(x=None), dict(off=None), dict(c=None), dict(codes=None), dict(k=0),
               dict(k=128), dict(k=300), dict(k=2304), dict(x=FAKE + 8), dict(c=FAKE + 8), dict(codes=FAKE + 2), dict(off=FAKE + 2),
               dict(status=FAKE + 2)):
        assert enc(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(q_rows=-1), dict(maxq=-1), dict(x=None), dict(qo=None), dict(c=None), dict(table=None), dict(k=4096),
               dict(k=257), dict(x=FAKE + 2), dict(table=FAKE + 8), dict(qo=FAKE + 1)):
        assert tab(**kw) == EINVAL, kw
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(k=1000), dict(table=None), dict(qo=None),
               dict(codes=None), dict(do=None), dict(out=None), dict(table=FAKE + 8), dict(codes=FAKE + 2), dict(out=FAKE + 2),
               dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
    # fp32, other widths and queries above 128 tokens are not served
    assert enc(dtype=2) == EUNSUPPORTED and tab(dtype=2) == EUNSUPPORTED and enc(dtype=7) == EUNSUPPORTED
    assert enc(dim=320) == EUNSUPPORTED and tab(dim=320) == EUNSUPPORTED and enc(dim=64) == EUNSUPPORTED
    assert tab(maxq=129) == EUNSUPPORTED and score(maxq=129) == EUNSUPPORTED
    assert score(d_rows=2**31 - 1) == EUNSUPPORTED


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd

    shard = _shard()
    calls = []
    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), centroid_score_fn=lambda q, i: calls.append("cent"),
                                     int8_score_fn=lambda q, i: calls.append("i8"), rerank_fn=lambda q, c, x: calls.append("rr"))
    q = torch.randn(2, 4, 128).to(torch.bfloat16)
    for idx in (_index(_shard(n=4)), _index(_shard(id_base=6))):       # the count check: another count, another id_base
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    for m in (None, 0, -2):
        with pytest.raises(ValueError, match="n_candidates"):
            r.search(q, prefilter=_index(shard), n_candidates=m)
    with pytest.raises(ValueError, match="n_candidates goes with prefilter"):
        r.search(q, n_candidates=3)
    with pytest.raises(ValueError, match="prefilter must be .*CentroidIndex"):
        r.search(q, prefilter=torch.zeros(5, dtype=torch.uint16), n_candidates=3)
    with pytest.raises(ValueError, match="either candidates= or prefilter="):
        r.search(q, prefilter=_index(shard), n_candidates=3, candidates=torch.zeros(2, 3, dtype=torch.int64))
    assert calls == []


def test_search_with_a_stand_in_stage_one():
    """One process, the truth as stage 1 and a float32 full scan as stage 2: the hook is called with the index, its top m go to the
    rerank, and the result is the rerank's top k."""
    import colpali_amd
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    g = torch.Generator().manual_seed(3)
    docs = [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16)
            for n in torch.randint(0, 30, (23,), generator=g).tolist()]
    shard = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None, id_base=4)
    idx = _index(shard)
    q = torch.nn.functional.normalize(torch.randn(3, 6, 128, generator=g), dim=-1).to(torch.bfloat16)
    seen = []

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < full.shape[1])
        got = torch.gather(full, 1, d.clamp(0, full.shape[1] - 1))
        seen.append(candidates.clone())
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    def cent_fn(queries, index):
        assert index is idx
        return _truth_fn(queries, index)

    r = colpali_amd.ShardedRetriever(shard, score_fn=score_fn, select=topk_oracle.torch_select, rerank_fn=rerank_fn,
                                     centroid_score_fn=cent_fn)
    k, m = 4, 9
    s, i = r.search(q, k=k, prefilter=idx, n_candidates=m)
    _, coarse = topk_oracle.topk(_truth_fn(q, idx).numpy(), m, 4)
    np.testing.assert_array_equal(seen[0].numpy(), coarse)
    rs, ri = rerank_fn(q, shard, torch.from_numpy(coarse))
    ws, wi = topk_oracle.topk(rs.numpy(), k, 0, ri.numpy())
    np.testing.assert_array_equal(i.numpy(), wi)
    np.testing.assert_array_equal(s.numpy(), ws)


def test_exports():
    import colpali_amd

    for name in ("CentroidIndex", "centroid_scores", "train_centroids"):
        assert name in colpali_amd.__all__ and hasattr(colpali_amd, name)
    assert colpali_amd._lib.ABI_VERSION == 22                           # additions only: the ABI version stays
