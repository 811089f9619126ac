"""K1s over the 13-bit image of a bf16 corpus (PackedCorpus.pack13): every score must carry the bits of the plain path.

The reference of every comparison is `maxsim_scores` on the same blob with packing off (COLPALI_AMD_PACK13=0, a second corpus
object without an image); nothing is compared to the code under test.  Each packed scan first checks that the corpus really
holds an image, so a silent decline cannot pass for parity.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EDGE_LENS = [1, 31, 32, 33, 64, 1000]
# bf16 patterns the code cannot hold: +0, -0, a denormal, 2^-32, 2.0, inf, NaN
BAD_BITS = [0x0000, 0x8000, 0x0001, 0x2F80, 0x4000, 0x7F80, 0x7FC0]


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()  # must load: no fallback
    return colpali_amd


def _rows(g, lens):
    rows = torch.nn.functional.normalize(torch.randn(max(sum(lens), 1), 128, generator=g), dim=-1).to(torch.bfloat16)
    return [t.clone() for t in rows[: sum(lens)].split(lens)]


def _representable(u):
    e = (u.astype(np.uint32) >> 7) & 0xFF
    return (e >= 96) & (e <= 127)


def _doc_flags(ps):
    return np.array([0 if p.numel() == 0 or _representable(p.view(torch.int16).numpy().view(np.uint16)).all() else 1 for p in ps],
                    dtype=np.uint8)


def _plant(p, bits, row=0, col=5):
    p.view(torch.int16)[row, col] = int(np.array(bits, dtype=np.uint16).view(np.int16))


def _plain(amd, monkeypatch, q, corpus, **kw):
    """the reference: the same blob through the plain path"""
    bare = dataclasses.replace(corpus, _pack13=None, _pack13_note=None)
    with monkeypatch.context() as m:
        m.setenv("COLPALI_AMD_PACK13", "0")
        out = amd.maxsim_scores(q, bare, **kw).cpu()
    assert bare._pack13 is None
    return out


def _packed(amd, q, corpus, **kw):
    assert corpus.pack13() and corpus._pack13 is not None
    out = amd.maxsim_scores(q, corpus, **kw).cpu()
    assert corpus._pack13 is not None
    return out


def _same_bits(a, b):
    ai, bi = a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)
    return bool(((ai == bi) | (torch.isnan(a) & torch.isnan(b))).all())


def _dense(g, n_q, lq):
    return torch.nn.functional.normalize(torch.randn(n_q, lq, 128, generator=g), dim=-1).to(torch.bfloat16).to(DEV).contiguous()


def _ragged(amd, g, n_q, max_tokens):
    """n_q queries of uneven lengths, at most max_tokens tokens in all"""
    lens = [max(1, (max_tokens // n_q) - (i % 3)) for i in range(n_q)]
    lens[0] += max_tokens - sum(lens)
    return amd.pack_queries(_rows(g, lens), DEV, compact=False)


@pytest.fixture(scope="module")
def edge_docs():
    g = torch.Generator().manual_seed(1313)
    lens = EDGE_LENS * 6 + [7, 96, 129, 500]                    # 40 documents: the headline's plan (4 x 32) runs one round of waves
    perm = torch.randperm(len(lens), generator=g).tolist()
    return _rows(g, [lens[i] for i in perm])


def test_encode_decode_flags_and_list(amd):
    from colpali_amd.corpus import pack13_decode

    g = torch.Generator().manual_seed(1)
    lens = EDGE_LENS + [0, 5, 40] + EDGE_LENS + [200] * 30       # 45 documents, two of them flagged below: under 5 %
    ps = _rows(g, lens)
    _plant(ps[5], 0x0000, row=999, col=127)
    _plant(ps[8], 0x7FC0, row=39, col=0)
    corpus = amd.pack_passages(ps, DEV, batch_size=None)
    assert corpus.pack13()
    img = corpus._pack13
    want_flags = _doc_flags(ps)
    assert want_flags[5] == 1 and want_flags[8] == 1
    assert np.array_equal(img.flagged.cpu().numpy(), want_flags)
    want_ids = np.nonzero(want_flags)[0].astype(np.int32)
    assert img.n_flagged == len(want_ids)
    assert np.array_equal(img.ids.cpu().numpy(), want_ids)
    back = pack13_decode(corpus).cpu().view(torch.int16)
    blob = corpus.blob.cpu().view(torch.int16)
    off = corpus.offsets.cpu().numpy()
    for c in range(len(ps)):
        if not want_flags[c]:
            assert torch.equal(back[off[c]:off[c + 1]], blob[off[c]:off[c + 1]]), c
    corpus.drop_pack13()
    assert corpus._pack13 is None


@pytest.mark.parametrize("n_q", [1, 2, 3, 4, 5, 6, 7, 8])
def test_units_1_to_8_dense_and_ragged(amd, monkeypatch, edge_docs, n_q):
    g = torch.Generator().manual_seed(100 + n_q)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    qd = _dense(g, n_q, 16)                                      # n_q units of 16 tokens: msim_fwd
    assert torch.equal(_packed(amd, qd, corpus), _plain(amd, monkeypatch, qd, corpus))
    qr = _ragged(amd, g, n_q, 16 * n_q - 3)                      # the flat layout: msim_fwd_ragged
    assert torch.equal(_packed(amd, qr, corpus), _plain(amd, monkeypatch, qr, corpus))


def test_headline_plan_four_queries_of_32(amd, monkeypatch, edge_docs):
    g = torch.Generator().manual_seed(432)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    assert len(corpus) == 40
    q = _dense(g, 4, 32)
    assert torch.equal(_packed(amd, q, corpus), _plain(amd, monkeypatch, q, corpus))


def test_fewer_documents_than_waves_and_an_empty_document(amd, monkeypatch):
    g = torch.Generator().manual_seed(7)
    for lens in ([33, 1000, 31], [33, 0, 64], [0, 32], [1]):
        corpus = amd.pack_passages(_rows(g, lens), DEV, batch_size=None)
        for q in (_dense(g, 4, 32), _dense(g, 1, 16)):
            assert _same_bits(_packed(amd, q, corpus), _plain(amd, monkeypatch, q, corpus)), lens


# the only test that reaches the list-driven launch of the raw K1s: every unit count it is built for (1..8), and the headline plan
@pytest.mark.parametrize("n_q,lq", [(4, 32)] + [(n, 16) for n in range(1, 9)])
def test_flagged_documents_are_scored_from_the_blob(amd, monkeypatch, n_q, lq):
    g = torch.Generator().manual_seed(99)
    lens = ([64, 33, 200] * 60)[: 160]
    ps = _rows(g, lens)
    where = [3, 20, 41, 77, 100, 130, 159]                       # distinct documents, unflagged ones between them
    for doc, bits in zip(where, BAD_BITS):
        _plant(ps[doc], bits, row=lens[doc] - 1, col=(7 * doc) % 128)
    want_flags = _doc_flags(ps)
    assert all(want_flags[d] for d in where)
    corpus = amd.pack_passages(ps, DEV, batch_size=None)
    q = _dense(g, n_q, lq)
    got = _packed(amd, q, corpus)
    assert np.array_equal(corpus._pack13.flagged.cpu().numpy(), want_flags)
    assert corpus._pack13.n_flagged == int(want_flags.sum()) <= 0.05 * len(ps)
    want = _plain(amd, monkeypatch, q, corpus)
    assert _same_bits(got, want)


def test_all_similarities_negative(amd, monkeypatch, edge_docs):
    g = torch.Generator().manual_seed(5)
    ps = [p.abs() for p in edge_docs]
    corpus = amd.pack_passages(ps, DEV, batch_size=None)
    q = -_dense(g, 4, 32).abs()
    want = _plain(amd, monkeypatch, q, corpus)
    assert bool((want < 0).all())
    assert torch.equal(_packed(amd, q, corpus), want)


def test_clamp0(amd, monkeypatch, edge_docs):
    g = torch.Generator().manual_seed(6)
    ps = [p.abs() for p in edge_docs]
    corpus = amd.pack_passages(ps, DEV, batch_size=4)            # shorter passages of a block see the reference's zero padding
    assert corpus.clamp0 is not None and bool(corpus.clamp0.any()) and not bool(corpus.clamp0.all())
    q = -_dense(g, 3, 32).abs()
    want = _plain(amd, monkeypatch, q, corpus)
    assert bool((want == 0).any()) and bool((want < 0).any())
    assert torch.equal(_packed(amd, q, corpus), want)


def test_ref_rounding(amd, monkeypatch, edge_docs):
    g = torch.Generator().manual_seed(8)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    for q in (_dense(g, 4, 32), _ragged(amd, g, 5, 70)):
        want = _plain(amd, monkeypatch, q, corpus, ref_rounding=True)
        assert not torch.equal(want, _plain(amd, monkeypatch, q, corpus))
        assert torch.equal(_packed(amd, q, corpus, ref_rounding=True), want)


# ---- the host rules: asserted on the corpus' field, never by timing
def test_second_scan_builds_and_in_place_change_drops(amd, monkeypatch, edge_docs):
    monkeypatch.delenv("COLPALI_AMD_PACK13", raising=False)
    g = torch.Generator().manual_seed(9)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    q = _dense(g, 4, 32)
    want = _plain(amd, monkeypatch, q, corpus)
    first = amd.maxsim_scores(q, corpus).cpu()
    assert corpus._pack13 is None                                # a corpus scanned once never pays
    second = amd.maxsim_scores(q, corpus).cpu()
    assert corpus._pack13 is not None
    assert torch.equal(first, want) and torch.equal(second, want)
    corpus.blob.add_(corpus.blob)                                # in place: same storage, new version
    want2 = _plain(amd, monkeypatch, q, corpus)
    assert not torch.equal(want2, want)
    third = amd.maxsim_scores(q, corpus).cpu()
    assert corpus._pack13 is None                                # the stale image is gone; this state has been seen once
    fourth = amd.maxsim_scores(q, corpus).cpu()
    assert corpus._pack13 is not None
    assert torch.equal(third, want2) and torch.equal(fourth, want2)


def test_k1b_scans_never_build(amd, monkeypatch, edge_docs):
    monkeypatch.delenv("COLPALI_AMD_PACK13", raising=False)
    g = torch.Generator().manual_seed(10)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    q = _dense(g, 9, 32)                                         # nine queries: K1b
    for _ in range(3):
        amd.maxsim_scores(q, corpus)
    assert corpus._pack13 is None and corpus._pack13_note is None


def test_too_many_flagged_declines(amd, monkeypatch):
    monkeypatch.delenv("COLPALI_AMD_PACK13", raising=False)
    g = torch.Generator().manual_seed(11)
    ps = _rows(g, [40] * 10)
    _plant(ps[4], 0x0000)                                        # one of ten documents: 10 %
    corpus = amd.pack_passages(ps, DEV, batch_size=None)
    assert corpus.pack13() is False and corpus._pack13 is None
    q = _dense(g, 4, 32)
    want = _plain(amd, monkeypatch, q, corpus)
    for _ in range(3):
        assert torch.equal(amd.maxsim_scores(q, corpus).cpu(), want)
        assert corpus._pack13 is None


def test_environment_switch(amd, monkeypatch, edge_docs):
    g = torch.Generator().manual_seed(12)
    q = _dense(g, 4, 32)
    corpus = amd.pack_passages(edge_docs, DEV, batch_size=None)
    monkeypatch.setenv("COLPALI_AMD_PACK13", "0")
    assert corpus.pack13() is False
    for _ in range(3):
        want = amd.maxsim_scores(q, corpus).cpu()
        assert corpus._pack13 is None
    monkeypatch.setenv("COLPALI_AMD_PACK13", "1")
    fresh = amd.pack_passages(edge_docs, DEV, batch_size=None)
    got = amd.maxsim_scores(q, fresh).cpu()                      # builds on the first scan
    assert fresh._pack13 is not None
    assert torch.equal(got, want)
