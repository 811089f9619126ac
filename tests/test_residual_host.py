"""The residual-compressed corpus without a GPU: the numpy truth of the codec (tests/residual_truth.py) on hand-computed cases,
`train_residual_codec` on clustered synthetic residuals, the refusals of the Python layer and of the C ABI (before any device work),
the `nbytes` arithmetic and the routing of `create_plaid_index`."""
import re
import os

import numpy as np
import pytest
import torch

from tests import residual_truth as rt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------------ the truth
@pytest.mark.parametrize("bits", [2, 4])
def test_pack_unpack_round_trip(bits):
    rng = np.random.default_rng(bits)
    b = rng.integers(0, 1 << bits, size=(37, 128))
    packed = rt.pack(b, bits)
    assert packed.shape == (37, 16 * bits) and packed.dtype == np.uint8
    np.testing.assert_array_equal(rt.unpack(packed, bits), b)
    # the little-endian bit string: bit i of the row is bit i % 8 of byte i // 8
    bitstring = np.unpackbits(packed, axis=1, bitorder="little")
    for k in (0, 1, 7, 8, 63, 127):
        field = sum(bitstring[:, k * bits + i].astype(np.int64) << i for i in range(bits))
        np.testing.assert_array_equal(field, b[:, k])
    # 8 consecutive dimensions are one little-endian 16- / 32-bit field
    words = packed.view("<u2" if bits == 2 else "<u4")
    for chunk in (0, 5, 15):
        want = sum(b[:, 8 * chunk + j] << (j * bits) for j in range(8))
        np.testing.assert_array_equal(words[:, chunk].astype(np.int64), want)


def test_hand_computed_pack_and_decode():
    b = np.zeros((1, 128), dtype=np.int64)
    b[0, :4] = [0, 1, 2, 3]
    assert rt.pack(b, 2)[0, 0] == 0xE4 and not rt.pack(b, 2)[0, 1:].any()
    b4 = np.zeros((1, 128), dtype=np.int64)
    b4[0, :3] = [0x5, 0xA, 0xF]
    assert list(rt.pack(b4, 4)[0, :3]) == [0xA5, 0x0F, 0x00]

    C = np.stack([np.full(128, 1.0, np.float32), np.full(128, 0.5, np.float32)])
    w = np.array([-0.5, -0.25, 0.25, 0.5], dtype=np.float32)
    got = rt.decode(C, [1], rt.pack(b, 2), w, 2, "bf16")
    assert list(got[0, :5]) == [0x0000, 0x3E80, 0x3F40, 0x3F80, 0x0000]           # 0.5 - 0.5, 0.25, 0.75, 1.0, 0.5 - 0.5
    got16 = rt.decode(C, [1], rt.pack(b, 2), w, 2, "f16")
    assert list(got16[0, :4]) == [0x0000, 0x3400, 0x3A00, 0x3C00]
    # one rounding to nearest even: around 1.0 a bfloat16 ulp is 2^-7
    w_r = np.array([2.0**-9, 2.0**-8, 3 * 2.0**-8, 2.0**-7], dtype=np.float32)
    got = rt.decode(C, [0], rt.pack(b, 2), w_r, 2, "bf16")
    assert list(got[0, :4]) == [0x3F80, 0x3F80, 0x3F82, 0x3F81]                    # below half, a tie to even (down), a tie to even (up), exact
    # no renormalisation: the decoded row is not a unit row, and stays that way
    assert float(np.linalg.norm(rt.from_bits(got, "bf16"))) > 11.0
    # a code >= K: NaN, and never an index
    assert (rt.decode(C, [2], rt.pack(b, 2), w, 2, "bf16") == 0x7FC0).all()
    assert (rt.decode(C, [65535], rt.pack(b, 2), w, 2, "f16") == 0x7E00).all()


def test_a_value_equal_to_a_cutoff_goes_to_the_upper_bucket():
    cut = np.array([-0.25, 0.0, 0.25], dtype=np.float32)
    C = np.zeros((1, 128), dtype=np.float32)
    rows = np.zeros((1, 128), dtype=np.float32)
    rows[0, :7] = [-0.3, -0.25, -0.125, 0.0, 0.125, 0.25, 1.0]
    rows[0, 7] = np.nextafter(np.float32(0.25), np.float32(0))
    b = rt.buckets(rows, C, [0], cut)
    assert list(b[0, :8]) == [0, 1, 1, 2, 2, 3, 3, 2]
    # the residual is ONE float32 subtraction: 1 - 2^-25 is a tie that rounds to 1.0, which equals the cutoff (float64 would stay below)
    C[0, 8] = 2.0**-25
    rows[0, 8] = 1.0
    assert rt.buckets(rows, C, [0], np.array([0.5, 1.0, 2.0], dtype=np.float32))[0, 8] == 2
    # a code >= K: all-zero buckets
    assert not rt.buckets(rows, C, [1], cut).any()
    cut4 = np.linspace(-0.7, 0.7, 15).astype(np.float32)
    rows4 = np.tile(cut4, 9)[:128].reshape(1, 128).astype(np.float32)
    np.testing.assert_array_equal(rt.buckets(rows4, np.zeros((1, 128), np.float32), [0], cut4)[0, :15], np.arange(1, 16))


# ------------------------------------------------------------------------------------------------------------------ training
def _clustered_residuals(seed, s=4096):
    """residuals of rows drawn round a few centroids: a mixture of a tight and a wide Gaussian, not centred"""
    g = torch.Generator().manual_seed(seed)
    tight = torch.randn(s, 128, generator=g) * 0.02
    wide = torch.randn(s, 128, generator=g) * 0.08 + 0.01
    pick = torch.rand(s, 1, generator=g) < 0.7
    return torch.where(pick, tight, wide)


@pytest.mark.parametrize("bits", [2, 4])
def test_train_residual_codec(bits):
    from colpali_amd import train_residual_codec

    e = _clustered_residuals(bits)
    cutoffs, weights = train_residual_codec(e, bits)
    nb = 1 << bits
    assert cutoffs.shape == (nb - 1,) and weights.shape == (nb,) and cutoffs.dtype == weights.dtype == torch.float32
    c, w = cutoffs.numpy(), weights.numpy()
    assert (np.diff(c) >= 0).all()                                         # non-decreasing
    assert (w[1:] >= c).all() and (w[:-1] <= c).all()                      # every weight within its bucket's cutoffs
    # the cutoffs are the j / 2^bits quantiles of all sampled values
    srt = np.sort(e.numpy().reshape(-1))
    np.testing.assert_array_equal(c, srt[[j * srt.size // nb for j in range(1, nb)]])
    # the weights are the bucket means
    b = rt.buckets(e.numpy(), np.zeros((1, 128), np.float32), np.zeros(len(e), np.int64), c)
    for k in range(nb):
        np.testing.assert_allclose(w[k], e.numpy()[b == k].astype(np.float64).mean(), rtol=1e-6, atol=1e-9)
    # the codec beats the centroid alone
    err = float(((e.numpy() - w[b]) ** 2).sum(axis=1).mean())
    base = float((e.numpy() ** 2).sum(axis=1).mean())
    print(f"bits={bits}: mean |e - w[b]|^2 = {err:.4e}, mean |e|^2 = {base:.4e}")
    assert err < base
    # reproducible
    c2, w2 = train_residual_codec(e.clone(), bits)
    assert torch.equal(c2, cutoffs) and torch.equal(w2, weights)


def test_train_residual_codec_empty_bucket_takes_the_midpoint():
    from colpali_amd import train_residual_codec

    e = torch.zeros(8, 128)
    e[:4] = 1.0                                                            # two values only: the sorted halves are 0 .. 0, 1 .. 1
    cutoffs, weights = train_residual_codec(e, 2)
    assert cutoffs.tolist() == [0.0, 1.0, 1.0]
    # buckets: value 0 -> 1 (0 <= 0), value 1 -> 3; bucket 0 is empty below its one cutoff, bucket 2 is empty between 1 and 1
    assert weights.tolist() == [0.0, 0.0, 1.0, 1.0]


def test_train_residual_codec_refusals():
    from colpali_amd import train_residual_codec

    e = torch.zeros(4, 128)
    for bits in (0, 1, 3, 8, 2.0, True):
        with pytest.raises(ValueError):
            train_residual_codec(e, bits)
    for bad in (torch.zeros(4, 64), torch.zeros(128), torch.zeros(4, 128, dtype=torch.float64), torch.zeros(0, 128)):
        with pytest.raises(ValueError):
            train_residual_codec(bad, 2)


# ------------------------------------------------------------------------------------------------------------------ the container
def _host_rc(amd, bits=2, k=256, lens=(3, 0, 5), dtype=torch.bfloat16, clamp=True, stored_bits="same", **over):
    rows = sum(lens)
    lengths = torch.tensor(lens, dtype=torch.int64)
    off = torch.zeros(len(lens) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lengths, 0).to(torch.int32)
    parts = dict(centroids=torch.zeros(k, 128, dtype=dtype), codes=torch.zeros(rows, dtype=torch.int16).view(torch.uint16),
                 residuals=torch.zeros(rows, 16 * bits, dtype=torch.uint8), cutoffs=torch.zeros((1 << bits) - 1),
                 weights=torch.zeros(1 << bits), offsets=off, clamp0=torch.zeros(len(lens), dtype=torch.uint8) if clamp else None,
                 lengths=lengths, id_base=7, bits=bits if stored_bits == "same" else stored_bits)
    parts.update(over)
    return amd.ResidualCorpus(**parts)


def test_container_attributes_and_nbytes():
    import colpali_amd as amd

    for bits, k, clamp in ((2, 256, True), (4, 2048, False)):
        rc = _host_rc(amd, bits, k, clamp=clamp)
        assert len(rc) == 3 and rc.bits == bits and rc.id_base == 7 and rc.device.type == "cpu" and rc.n_centroids == k
        want = k * 256 + 8 * (2 + 16 * bits) + 4 * ((1 << bits) - 1) + 4 * (1 << bits) + 4 * 4 + (3 if clamp else 0)
        assert rc.nbytes == want
        # .index is a view over the same tensors, not a copy
        assert isinstance(rc.index, amd.CentroidIndex)
        assert rc.index.codes.data_ptr() == rc.codes.data_ptr() and rc.index.centroids.data_ptr() == rc.centroids.data_ptr()
        assert rc.index.offsets.data_ptr() == rc.offsets.data_ptr() and len(rc.index) == 3 and rc.index.id_base == 7
    # the table of the issue: 2 + 32 and 2 + 64 bytes per row
    assert 2 + 16 * 2 == 34 and 2 + 16 * 4 == 66


def test_container_refusals():
    import colpali_amd as amd

    for bits in (1, 3, 8, None, 2.0):
        with pytest.raises(ValueError):
            _host_rc(amd, stored_bits=bits)
    with pytest.raises(ValueError):
        _host_rc(amd, residuals=torch.zeros(8, 64, dtype=torch.uint8))                      # 4-bit rows in a 2-bit corpus
    with pytest.raises(ValueError):
        _host_rc(amd, residuals=torch.zeros(7, 32, dtype=torch.uint8))
    with pytest.raises(ValueError):
        _host_rc(amd, residuals=torch.zeros(8, 32, dtype=torch.int8))
    with pytest.raises(ValueError):
        _host_rc(amd, cutoffs=torch.zeros(4))
    with pytest.raises(ValueError):
        _host_rc(amd, weights=torch.zeros(4, dtype=torch.float64))
    with pytest.raises(ValueError):
        _host_rc(amd, k=100)                                                                 # the centroid index's own rule
    with pytest.raises(NotImplementedError):
        _host_rc(amd, dtype=torch.float32)
    with pytest.raises(ValueError):
        _host_rc(amd, codes=torch.zeros(8, dtype=torch.int16))
    # a CPU container is refused by everything that runs a kernel: the GPU-only error, no quiet fall-back
    rc = _host_rc(amd)
    q = [torch.zeros(4, 128, dtype=torch.bfloat16)]
    with pytest.raises(RuntimeError):
        amd.residual_rerank_scores(q, rc, torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError):
        rc.decompress()
    with pytest.raises(ValueError):
        amd.residual_rerank_scores(q, rc.index, torch.zeros(1, 2, dtype=torch.int64))       # not a ResidualCorpus
    corpus = amd.pack_passages([torch.zeros(4, 128, dtype=torch.bfloat16)], torch.device("cpu"), batch_size=None)
    for bits in (3, 8):
        with pytest.raises(ValueError):
            amd.ResidualCorpus.build(corpus, bits=bits)
    with pytest.raises(RuntimeError):
        amd.ResidualCorpus.build(corpus, bits=2)


def test_retriever_refuses_the_routes_that_need_rows():
    import colpali_amd as amd

    rc = _host_rc(amd)
    r = amd.ShardedRetriever(rc)
    assert r._rerank is amd.residual_rerank_scores
    assert amd.ShardedRetriever(rc, rerank_fn=max)._rerank is max                           # an injected one is kept
    packed = amd.pack_passages([torch.zeros(4, 128, dtype=torch.bfloat16)], torch.device("cpu"), batch_size=None)
    assert amd.ShardedRetriever(packed)._rerank is amd.retrieval.rerank_scores             # nothing changes for a PackedCorpus
    q = [torch.zeros(4, 128, dtype=torch.bfloat16)]
    for call in (lambda: r.search(q, k=2), lambda: r.search(q, k=2, filter=object()), lambda: r.search(q, k=2, group_by=object()),
                 lambda: r.align(q, torch.zeros(1, 1, dtype=torch.int64)), lambda: r.mine(q, None, 2)):
        with pytest.raises(NotImplementedError, match="ResidualCorpus"):
            call()
    with pytest.raises(NotImplementedError):
        amd.rerank(q, rc, torch.zeros(1, 2, dtype=torch.int64), ref_rounding=True)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _cand_call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
               n_d=10, d_rows=100, dim=128, cand=FAKE, m=4, ld_cand=4, out=FAKE, ld=4, ws=FAKE):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return L.msim_res_candidates(dtype, qt, q_off, oh.ctypes.data, n_q, codes, res, C, K, w, bits, d_off, None, n_d, d_rows, dim, cand, m,
                                 ld_cand, 0, out, ld, None, ws, None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_res_candidates_workspace_bytes(0, 5, 10) == 0
    assert L.msim_res_candidates_workspace_bytes(3, 0, 10) == 0
    assert L.msim_res_candidates_workspace_bytes(-1, 5, 10) == 0
    w = L.msim_res_candidates_workspace_bytes(1000, 100, 125000)
    assert w > 0 and w % 16 == 0
    assert _cand_call(L, n_q=0) == 0 and _cand_call(L, m=0) == 0                # nothing to do: no pointer is looked at
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(d_rows=-1), dict(qt=None), dict(q_off=None), dict(d_off=None),
               dict(cand=None), dict(out=None), dict(ws=None), dict(codes=None), dict(res=None), dict(C=None), dict(w=None),
               dict(qt=FAKE + 8), dict(res=FAKE + 8), dict(C=FAKE + 2), dict(ws=FAKE + 4), dict(codes=FAKE + 1), dict(ld_cand=3),
               dict(ld=3), dict(q_off_host=[1, 3, 7]), dict(q_off_host=[0, 5, 3]), dict(K=100), dict(K=4096)):
        assert _cand_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=320), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8),
               dict(q_off_host=[0, 3, 3 + 129])):
        assert _cand_call(L, **kw) == EUNSUPPORTED, kw

    def enc(dtype=0, d=FAKE, n_rows=10, dim=128, codes=FAKE, C=FAKE, K=256, cut=FAKE, bits=2, res=FAKE):
        return L.msim_res_encode_docs(dtype, d, n_rows, dim, codes, C, K, cut, bits, res, None)

    def dec(dtype=0, codes=FAKE, res=FAKE, n_rows=10, row0=0, row1=10, C=FAKE, K=256, w=FAKE, bits=4, dim=128, out=FAKE):
        return L.msim_res_decode_rows(dtype, codes, res, n_rows, row0, row1, C, K, w, bits, dim, out, None)

    assert enc(n_rows=0) == 0 and dec(row0=4, row1=4) == 0
    for kw in (dict(n_rows=-1), dict(d=None), dict(codes=None), dict(C=None), dict(cut=None), dict(res=None), dict(d=FAKE + 8),
               dict(res=FAKE + 4), dict(K=300)):
        assert enc(**kw) == EINVAL, kw
    for kw in (dict(row0=-1), dict(row0=5, row1=4), dict(row1=11), dict(out=None), dict(w=None), dict(out=FAKE + 8), dict(K=0)):
        assert dec(**kw) == EINVAL, kw
    for fn in (enc, dec):
        for kw in (dict(dtype=2), dict(dim=320), dict(bits=3), dict(bits=0)):
            assert fn(**kw) == EUNSUPPORTED, (fn.__name__, kw)


def test_header_states_the_codec():
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    for name in ("msim_res_encode_docs", "msim_res_decode_rows", "msim_res_candidates"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert re.search(r"\bsize_t\s+msim_res_candidates_workspace_bytes\s*\(\s*int n_q,\s*int m,\s*int n_d\s*\)\s*;", header)
    assert "no renormalisation" in header and "little-endian" in header


# ------------------------------------------------------------------------------------------------------------------ routing
def test_create_plaid_index_routing(monkeypatch):
    import colpali_amd as amd
    from colpali_amd import corpus as corpus_mod
    from colpali_amd import retrieval, scoring

    calls = []
    cpu = torch.device("cpu")
    monkeypatch.setattr(scoring, "_require_gpu", lambda device: cpu)
    real_pack = corpus_mod.pack_passages
    monkeypatch.setattr(corpus_mod, "pack_passages", lambda ps, dev, batch_size=128, id_base=0: real_pack(ps, cpu, batch_size, id_base))

    def fake_build(corpus, bits=2, **kw):
        calls.append((bits, kw))
        return _host_rc(amd, bits=bits)

    monkeypatch.setattr(retrieval.ResidualCorpus, "build", staticmethod(fake_build))
    ps = [torch.zeros(4, 128, dtype=torch.bfloat16), torch.zeros(2, 128, dtype=torch.bfloat16)]
    exact = amd.create_plaid_index(ps)                                     # nbits=None: today's exact index, no codec built
    assert type(exact) is amd.ExactMaxSimIndex and not calls
    assert isinstance(exact.retriever.shard, amd.PackedCorpus)
    assert type(amd.create_plaid_index(ps, "cpu", nbits=None)) is amd.ExactMaxSimIndex and not calls
    for nbits in (2, 4):
        idx = amd.create_plaid_index(ps, nbits=nbits, n_centroids=512, n_candidates=77)
        assert type(idx) is amd.ResidualMaxSimIndex and idx.n_candidates == 77
        assert isinstance(idx.retriever.shard, amd.ResidualCorpus) and idx.retriever.shard.bits == nbits
        assert calls[-1] == (nbits, {"n_centroids": 512})
    for bad in (0, 1, 3, 8, True, "2"):
        with pytest.raises(ValueError):
            amd.create_plaid_index(ps, nbits=bad)
    with pytest.raises(ValueError):
        amd.create_plaid_index([], nbits=2)
