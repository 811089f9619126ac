"""The compressed shard at width 320 without a GPU: the numpy truth (tests/residual_wide_truth.py) on hand-computed cases, the
refusals of the C ABI (before any device work) and of the Python layer, the header, and the two new file kinds."""
import os
import re

import numpy as np
import pytest
import torch

from tests import residual_wide_truth as wt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
W = 320
NEW_ENTRIES = ("msim_cent_wide_encode_docs", "msim_cent_wide_table", "msim_res_wide_encode_docs", "msim_res_wide_decode_rows",
               "msim_res_wide_candidates")


# ------------------------------------------------------------------------------------------------------------------ the truth
@pytest.mark.parametrize("bits", [2, 4])
def test_pack_unpack_round_trip(bits):
    rng = np.random.default_rng(bits)
    b = rng.integers(0, 1 << bits, size=(37, W))
    packed = wt.pack(b, bits)
    assert packed.shape == (37, 40 * bits) and packed.dtype == np.uint8
    np.testing.assert_array_equal(wt.unpack(packed, bits), b)
    bitstring = np.unpackbits(packed, axis=1, bitorder="little")           # bit i of the row is bit i % 8 of byte i // 8
    for k in (0, 1, 7, 8, 127, 128, 255, 256, 319):
        field = sum(bitstring[:, k * bits + i].astype(np.int64) << i for i in range(bits))
        np.testing.assert_array_equal(field, b[:, k])
    words = packed.view("<u2" if bits == 2 else "<u4")                     # 8 consecutive dimensions: one 16- / 32-bit field
    assert words.shape == (37, 40)
    for chunk in (0, 15, 16, 31, 32, 39):
        want = sum(b[:, 8 * chunk + j] << (j * bits) for j in range(8))
        np.testing.assert_array_equal(words[:, chunk].astype(np.int64), want)


def test_hand_computed_pack_and_decode():
    b = np.zeros((1, W), dtype=np.int64)
    b[0, :4] = [0, 1, 2, 3]
    b[0, 316:] = [3, 2, 1, 0]
    p2 = wt.pack(b, 2)
    assert p2.shape == (1, 80) and p2[0, 0] == 0xE4 and p2[0, 79] == 0x1B and not p2[0, 1:79].any()
    C = np.stack([np.full(W, 1.0, np.float32), np.full(W, 0.5, np.float32)])
    w = np.array([-0.5, -0.25, 0.25, 0.5], dtype=np.float32)
    got = wt.decode(C, [1], p2, w, 2, "bf16")
    assert got.shape == (1, W) and list(got[0, :5]) == [0x0000, 0x3E80, 0x3F40, 0x3F80, 0x0000]
    assert list(got[0, 316:]) == [0x3F80, 0x3F40, 0x3E80, 0x0000]
    assert (wt.decode(C, [2], p2, w, 2, "bf16") == 0x7FC0).all() and (wt.decode(C, [65535], p2, w, 2, "f16") == 0x7E00).all()
    rows = np.stack([np.full(W, 0.5, np.float32), np.full(W, 0.75, np.float32)])
    cut = np.array([-0.25, 0.0, 0.25], dtype=np.float32)
    assert (wt.buckets(rows, C, [1, 1], cut) == np.array([[2], [3]])).all()        # e == 0.0 and e == 0.25 sit ON a cutoff: the upper bucket
    assert (wt.buckets(rows, C, [1, 2], cut)[1] == 0).all()                        # a code >= K: all-zero buckets


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _cand_call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
               n_d=10, d_rows=100, dim=W, cand=FAKE, m=4, ld_cand=4, out=FAKE, ld=4, ws=FAKE, entry="msim_res_wide_candidates"):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return getattr(L, entry)(dtype, qt, q_off, oh.ctypes.data, n_q, codes, res, C, K, w, bits, d_off, None, n_d, d_rows, dim, cand, m,
                             ld_cand, 0, out, ld, None, ws, None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    # ---- the rerank
    ws_bytes = L.msim_res_wide_candidates_workspace_bytes
    assert ws_bytes(0, 5, 10) == 0 and ws_bytes(3, 0, 10) == 0 and ws_bytes(-1, 5, 10) == 0
    w = ws_bytes(1000, 100, 125000)
    assert w > 0 and w % 16 == 0 and w == ws_bytes(1000, 100, 1) == ws_bytes(1000, 100, 2**31 - 1)     # no row count goes in
    assert _cand_call(L, n_q=0) == 0 and _cand_call(L, m=0) == 0                # nothing to do: no pointer is looked at
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(d_rows=-1), dict(qt=None), dict(q_off=None), dict(d_off=None),
               dict(cand=None), dict(out=None), dict(ws=None), dict(codes=None), dict(res=None), dict(C=None), dict(w=None),
               dict(qt=FAKE + 8), dict(res=FAKE + 8), dict(C=FAKE + 2), dict(ws=FAKE + 4), dict(codes=FAKE + 1), dict(ld_cand=3),
               dict(ld=3), dict(q_off_host=[1, 3, 7]), dict(q_off_host=[0, 5, 3]), dict(K=100), dict(K=0), dict(K=4096)):
        assert _cand_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=128), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8),
               dict(q_off_host=[0, 3, 3 + 129]), dict(d_rows=1 << 31)):
        assert _cand_call(L, **kw) == EUNSUPPORTED, kw

    # ---- the codec
    def enc(dtype=0, d=FAKE, n_rows=10, dim=W, codes=FAKE, C=FAKE, K=256, cut=FAKE, bits=2, res=FAKE):
        return L.msim_res_wide_encode_docs(dtype, d, n_rows, dim, codes, C, K, cut, bits, res, None)

    def dec(dtype=0, codes=FAKE, res=FAKE, n_rows=10, row0=0, row1=10, C=FAKE, K=256, w=FAKE, bits=4, dim=W, out=FAKE):
        return L.msim_res_wide_decode_rows(dtype, codes, res, n_rows, row0, row1, C, K, w, bits, dim, out, None)

    assert enc(n_rows=0) == 0 and dec(row0=4, row1=4) == 0
    for kw in (dict(n_rows=-1), dict(d=None), dict(codes=None), dict(C=None), dict(cut=None), dict(res=None), dict(d=FAKE + 8),
               dict(res=FAKE + 4), dict(codes=FAKE + 1), dict(K=100), dict(K=0), dict(K=4096)):
        assert enc(**kw) == EINVAL, kw
    for kw in (dict(row0=-1), dict(row0=5, row1=4), dict(row1=11), dict(n_rows=-1), dict(out=None), dict(w=None), dict(codes=None),
               dict(res=None), dict(C=None), dict(out=FAKE + 8), dict(C=FAKE + 8), dict(K=100), dict(K=0), dict(K=4096)):
        assert dec(**kw) == EINVAL, kw
    for fn in (enc, dec):
        for kw in (dict(dtype=2), dict(dim=128), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8), dict(bits=0)):
            assert fn(**kw) == EUNSUPPORTED, (fn.__name__, kw)
    big = (2**31 - 1) * 256 // 40 + 1                                       # more 40-lane rows than one launch has blocks for
    assert enc(n_rows=big) == EUNSUPPORTED and dec(n_rows=big, row1=big) == EUNSUPPORTED

    # ---- the centroid index
    def cenc(dtype=0, x=FAKE, off=FAKE, n=3, rows=40, dim=W, longest=20, c=FAKE, k=256, codes=FAKE, status=None):
        return L.msim_cent_wide_encode_docs(dtype, x, off, n, rows, dim, longest, c, k, codes, status, None)

    def tab(dtype=0, x=FAKE, qo=FAKE, n_q=4, q_rows=40, maxq=32, dim=W, c=FAKE, k=256, table=FAKE):
        return L.msim_cent_wide_table(dtype, x, qo, n_q, q_rows, maxq, dim, c, k, table, None)

    assert cenc(n=0) == 0 and cenc(n=0, x=None, off=None, c=None, codes=None) == 0 and cenc(longest=0, x=None, off=None, c=None) == 0
    assert tab(n_q=0) == 0 and tab(n_q=0, x=None, qo=None, c=None, table=None) == 0
    for kw in (dict(n=-1), dict(rows=-1), dict(longest=-1), dict(x=None), dict(off=None), dict(c=None), dict(codes=None), dict(k=0),
               dict(k=100), dict(k=4096), dict(x=FAKE + 8), dict(c=FAKE + 8), dict(codes=FAKE + 2), dict(off=FAKE + 2),
               dict(status=FAKE + 2)):
        assert cenc(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(q_rows=-1), dict(maxq=-1), dict(x=None), dict(qo=None), dict(c=None), dict(table=None), dict(k=4096),
               dict(k=100), dict(k=0), dict(x=FAKE + 2), dict(table=FAKE + 8), dict(qo=FAKE + 1)):
        assert tab(**kw) == EINVAL, kw
    for fn in (cenc, tab):
        for kw in (dict(dtype=2), dict(dtype=7), dict(dim=128), dict(dim=64)):
            assert fn(**kw) == EUNSUPPORTED, (fn.__name__, kw)
    assert tab(maxq=129) == EUNSUPPORTED
    assert cenc(longest=65535 * 128 + 1) == EUNSUPPORTED                    # more 128-row blocks than the grid's second dimension


def test_the_128_entries_still_refuse_width_320():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_cent_encode_docs(0, FAKE, FAKE, 3, 40, W, 20, FAKE, 256, FAKE, None, None) == EUNSUPPORTED
    assert L.msim_cent_table(0, FAKE, FAKE, 4, 40, 32, W, FAKE, 256, FAKE, None) == EUNSUPPORTED
    assert L.msim_res_encode_docs(0, FAKE, 10, W, FAKE, FAKE, 256, FAKE, 2, FAKE, None) == EUNSUPPORTED
    assert L.msim_res_decode_rows(0, FAKE, FAKE, 10, 0, 10, FAKE, 256, FAKE, 2, W, FAKE, None) == EUNSUPPORTED
    assert _cand_call(L, entry="msim_res_candidates") == EUNSUPPORTED and _cand_call(L, entry="msim_res_candidates", dim=128) not in (0, EUNSUPPORTED)
    oh = np.array([0, 3, 7], dtype=np.int32)
    assert L.msim_res_scores(0, FAKE, FAKE, oh.ctypes.data, 2, FAKE, FAKE, FAKE, 256, FAKE, 2, FAKE, None, 10, 100, W, FAKE, 10, FAKE,
                             None) == EUNSUPPORTED
    assert L.msim_fwd_candidates(0, FAKE, FAKE, oh.ctypes.data, 2, FAKE, FAKE, None, 10, W, FAKE, 4, 4, 0, FAKE, 4, None, 0, FAKE,
                                 None) == EUNSUPPORTED


def test_header_declares_every_new_entry():
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert re.search(r"\bsize_t\s+msim_res_wide_candidates_workspace_bytes\s*\(\s*int n_q,\s*int m,\s*int n_d\s*\)\s*;", header)
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    block = header[header.index("THE COMPRESSED SHARD AT WIDTH 320"):header.index("int msim_cent_wide_encode_docs(")]
    for words in ("no renormalisation", "little-endian", "80 bytes per row at 2 bits, 160 at 4", "p = 0, 1, 2", "never zero-filled",
                  "lowest k wins"):
        assert words in block, words


# ------------------------------------------------------------------------------------------------------------------ the classes
def _host_parts(bits=2, k=256, lens=(3, 0, 5), dtype=torch.bfloat16, clamp=True, width=W, **over):
    rows = sum(lens)
    lengths = torch.tensor(lens, dtype=torch.int64)
    off = torch.zeros(len(lens) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(lengths, 0).to(torch.int32)
    g = torch.Generator().manual_seed(5)
    parts = dict(centroids=torch.randn(k, width, generator=g).to(dtype),
                 codes=torch.randint(0, k, (rows,), generator=g).to(torch.int16).view(torch.uint16),
                 residuals=torch.randint(0, 256, (rows, width // 8 * bits), generator=g).to(torch.uint8),
                 cutoffs=torch.linspace(-0.1, 0.1, (1 << bits) - 1), weights=torch.linspace(-0.2, 0.2, 1 << bits), offsets=off,
                 clamp0=torch.zeros(len(lens), dtype=torch.uint8) if clamp else None, lengths=lengths, id_base=7, bits=bits)
    parts.update(over)
    return parts


def _host_rc(amd, **kw):
    return amd.ResidualWideCorpus(**_host_parts(**kw))


def test_container_attributes_and_constructor_validation():
    import colpali_amd as amd

    for bits in (2, 4):
        rc = _host_rc(amd, bits=bits)
        assert rc.width == W and rc.WIDTH == W and rc.bits == bits and rc.dtype == torch.bfloat16 and len(rc) == 3 and rc.n_centroids == 256
        assert rc.id_base == 7 and rc.device == torch.device("cpu") and rc.residuals.shape == (8, 40 * bits)
        assert type(rc.index) is amd.CentroidWideIndex and rc.index.codes is rc.codes and rc.index.centroids is rc.centroids
        assert rc.nbytes == 256 * 640 + 8 * (2 + 40 * bits) + 4 * ((2 << bits) - 1) + 4 * 4 + 3
        assert rc.index.nbytes == 256 * 640 + 8 * 2 + 4 * 4 + 3
    # siblings, not parent and child
    assert not isinstance(_host_rc(amd), amd.ResidualCorpus) and not isinstance(_host_rc(amd).index, amd.CentroidIndex)
    assert not issubclass(amd.ResidualWideCorpus, amd.ResidualCorpus) and not issubclass(amd.CentroidWideIndex, amd.CentroidIndex)
    p = _host_parts()
    bad = [dict(residuals=torch.zeros(8, 32, dtype=torch.uint8)),             # the 128-wide row size
           dict(residuals=torch.zeros(8, 160, dtype=torch.uint8)),            # the 4-bit row size under bits=2
           dict(residuals=torch.zeros(7, 80, dtype=torch.uint8)), dict(residuals=torch.zeros(8, 80, dtype=torch.int8)),
           dict(residuals=torch.zeros(8, 160, dtype=torch.uint8)[:, ::2]), dict(codes=p["codes"].view(torch.int16)),
           dict(codes=p["codes"].reshape(2, 4)), dict(cutoffs=torch.zeros(2)), dict(weights=torch.zeros(3)),
           dict(cutoffs=torch.zeros(3, dtype=torch.float64)), dict(offsets=p["offsets"].to(torch.int64)), dict(offsets=p["offsets"][:-1]),
           dict(clamp0=torch.zeros(4, dtype=torch.uint8)), dict(centroids=torch.zeros(100, W, dtype=torch.bfloat16)),
           dict(centroids=torch.zeros(4096, W, dtype=torch.bfloat16)), dict(bits=3), dict(bits=True), dict(bits=8)]
    for over in bad:
        with pytest.raises(ValueError):
            _host_rc(amd, **over)
    for over in (dict(centroids=torch.zeros(256, 128, dtype=torch.bfloat16)), dict(centroids=torch.zeros(256, W, dtype=torch.float32))):
        with pytest.raises(NotImplementedError):
            _host_rc(amd, **over)
    with pytest.raises(ValueError, match="live on"):                         # a device mismatch
        _host_rc(amd, residuals=torch.zeros(8, 80, dtype=torch.uint8, device="meta"))
    # the 128 classes keep refusing width 320
    with pytest.raises(NotImplementedError):
        amd.CentroidIndex(p["centroids"], p["codes"], p["offsets"], None, p["lengths"])
    with pytest.raises((NotImplementedError, ValueError)):
        amd.ResidualCorpus(**p)
    idx = amd.CentroidWideIndex(p["centroids"], p["codes"], p["offsets"], None, p["lengths"], 3)
    assert idx.WIDTH == W and idx.id_base == 3 and idx.clamp0 is None and len(idx) == 3
    # the codec trainer: the width is named, and a sample of the other width is refused as before
    s = torch.randn(50, W)
    cut, w = amd.train_residual_codec(s, 2, width=W)
    assert cut.shape == (3,) and w.shape == (4,)
    for call in (lambda: amd.train_residual_codec(s, 2), lambda: amd.train_residual_codec(torch.randn(50, 128), 2, width=W),
                 lambda: amd.train_residual_codec(torch.randn(50, 64), 2, width=64)):
        with pytest.raises(ValueError):
            call()
    for name in ("CentroidWideIndex", "ResidualWideCorpus", "centroid_wide_scores", "residual_wide_rerank_scores"):
        assert name in amd.__all__ and hasattr(amd, name) and name in amd.__doc__


def test_refusals_that_need_no_device():
    import colpali_amd as amd

    rc = _host_rc(amd)
    q = [torch.zeros(4, W, dtype=torch.bfloat16)]
    cand = torch.zeros(1, 2, dtype=torch.int64)
    # a CPU container is refused by everything that runs a kernel: the GPU-only error, no quiet fall-back
    for call in (lambda: amd.residual_wide_rerank_scores(q, rc, cand), lambda: rc.decompress(), lambda: amd.centroid_wide_scores(q, rc.index),
                 lambda: amd.rerank(q, rc, cand)):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        amd.residual_wide_rerank_scores(q, rc.index, cand)                   # not a ResidualWideCorpus
    with pytest.raises(NotImplementedError):
        amd.rerank(q, rc, cand, ref_rounding=True)
    corpus = amd.pack_passages([torch.zeros(4, W, dtype=torch.bfloat16)], torch.device("cpu"), batch_size=None)
    for bits in (3, 8):
        with pytest.raises(ValueError):
            amd.ResidualWideCorpus.build(corpus, bits=bits)
    with pytest.raises(RuntimeError):
        amd.ResidualWideCorpus.build(corpus, bits=2)
    # what exists at width 128 only refuses the wide classes by type, naming the width
    for call in (lambda: amd.residual_rerank_scores(q, rc, cand), lambda: amd.residual_scores(q, rc), lambda: amd.residual_align(q, rc, cand),
                 lambda: amd.residual_gather_pages(rc, cand), lambda: amd.centroid_scores(q, rc.index),
                 lambda: amd.LiveResidualCorpus.like(rc, 10, 4), lambda: amd.LiveResidualCorpus.from_residual(rc, 10, 4)):
        with pytest.raises(NotImplementedError, match="width 128"):
            call()
    # the retriever: the wide rerank by default, an injected one kept, the scanning routes and align refused
    r = amd.ShardedRetriever(rc)
    assert r._rerank is amd.residual_wide_rerank_scores and amd.ShardedRetriever(rc, rerank_fn=max)._rerank is max
    for call in (lambda: r.search(q, k=2), lambda: r.search(q, k=2, filter=object()), lambda: r.search(q, k=2, group_by=object()),
                 lambda: r.align(q, cand), lambda: r.mine(q, None, 2)):
        with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only"):
            call()
    # prefilter= and the shard's width
    packed = amd.pack_passages([torch.zeros(n, W, dtype=torch.bfloat16) for n in (3, 0, 5)], torch.device("cpu"), batch_size=None, id_base=7)
    narrow = amd.pack_passages([torch.zeros(n, 128, dtype=torch.bfloat16) for n in (3, 0, 5)], torch.device("cpu"), batch_size=None, id_base=7)
    p128 = _host_parts(width=128)
    idx128 = amd.CentroidIndex(p128["centroids"], p128["codes"], p128["offsets"], None, p128["lengths"], 7)
    calls = []
    hooks = dict(score_fn=lambda q, c: calls.append("score"), centroid_score_fn=lambda q, i: calls.append("cent"),
                 centroid_wide_score_fn=lambda q, i: calls.append("centw"), rerank_fn=lambda q, c, x: calls.append("rr"))
    with pytest.raises(ValueError, match="the shard is 320 wide: a 320-wide shard takes a CentroidWideIndex"):
        amd.ShardedRetriever(packed, **hooks).search(q, prefilter=idx128, n_candidates=2)
    with pytest.raises(ValueError, match="the shard is 128 wide: a 320-wide shard takes a CentroidWideIndex"):
        amd.ShardedRetriever(narrow, **hooks).search(q, prefilter=rc.index, n_candidates=2)
    with pytest.raises(ValueError, match="prefilter must be .*CentroidWideIndex"):
        amd.ShardedRetriever(packed, **hooks).search(q, prefilter=torch.zeros(5), n_candidates=2)
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------ the file kinds
@pytest.mark.parametrize("kind", ["ResidualWideCorpus", "CentroidWideIndex"])
def test_both_kinds_save_verify_and_load_on_the_host(tmp_path, kind):
    import colpali_amd as amd

    rc = _host_rc(amd, bits=4, lens=(3, 0, 5, 40))
    obj = rc if kind == "ResidualWideCorpus" else rc.index
    path = str(tmp_path / "x.msim")
    obj.save(path, chunk_bytes=4096)
    header = amd.verify_file(path)
    assert header["kind"] == kind
    names = {"centroids", "codes", "offsets", "clamp0", "lengths"} | ({"residuals", "cutoffs", "weights"} if obj is rc else set())
    assert {e["name"] for e in header["tensors"]} == names
    back = amd.load(path, "cpu")
    assert type(back) is type(obj) and back.id_base == 7 and len(back) == 4
    for name in names:
        a, b = getattr(back, name), getattr(obj, name)
        assert a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), name
    part = type(obj).load(path, "cpu", pages=(2, 4))
    assert part.id_base == 9 and part.lengths.tolist() == [5, 40] and part.offsets.tolist() == [0, 5, 45]
    assert torch.equal(part.codes.view(torch.int16), obj.codes.view(torch.int16)[3:48])
    other = amd.ResidualCorpus if obj is rc else amd.CentroidIndex
    with pytest.raises(amd.ShardFileError, match="not a"):
        other.load(path, "cpu")
    entry = next(e for e in header["tensors"] if e["name"] == "centroids")
    with open(path, "r+b") as f:                                             # one flipped byte in the second chunk of the centroids
        f.seek(entry["offset"] + 4096 + 17)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 0x01]))
    for call in (lambda: amd.verify_file(path), lambda: amd.load(path, "cpu")):
        with pytest.raises(amd.ShardFileError, match="'centroids', chunk 1"):
            call()
