"""The 2-slot ring forms of K1s13 and K1s (5-8 query units): the slab body issues the next slab's eight LDS-DMA requests while it
works on the current one (K1s13: one pinned in front of every (NU / 2)th MFMA; maxsim_stream.hip, ORDER).

Whatever the order, the ring can go wrong where a wave carries it from one document to the next, where a request is dead, where
documents are skipped and where a document is shorter than the ring.  The pack13 tests score 40 documents -- one round of waves, no
wave ever carries its ring over a document boundary -- so the corpora here are sized from the device: more than two rounds of waves.

Yardstick of every case: the CPU oracle (oracle/maxsim_oracle), called as tests/test_gpu_parity.py calls it, with that file's
tolerance |got - truth| <= 1e-5 * max(|truth|, 1); the literal REF_BF16 case is held against the oracle's literal tier, with that
bound and with the one the parity file sets for the tier (one bf16 ulp, more than 90 % equal).  The plain path is code under test as
well (the same ring), so it is not the reference; the packed scan and the plain path must additionally agree bit for bit, as a
consistency condition between the two forms.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import maxsim_oracle as mo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
RTOL = 1e-5
LEN_CYCLE = [0, 1, 31, 32, 33, 64, 65, 96]          # empty, one slab with a tail of 1 / 31 rows, exact multiples, one-row tails
BLOCK = 128                                          # the reference's passage block: every document shorter than 96 rows is clamped at 0
# (n_q, lq): 5, 6, 7 and 8 units of 16 tokens, the headline's 4 x 32, and a ragged batch of three queries (below)
DENSE = [(5, 16), (6, 16), (7, 16), (8, 16), (4, 32)]


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()  # must load: no fallback
    return colpali_amd


@pytest.fixture(scope="module")
def gw():
    """waves of one launch of the 2-slot forms: two workgroups of four waves per CU"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 2 * 4


def _rows(g, lens):
    rows = torch.nn.functional.normalize(torch.randn(max(sum(lens), 1), 128, generator=g), dim=-1).to(torch.bfloat16)
    return [t.clone() for t in rows[: sum(lens)].split(lens)]


def _queries(g, n_q, lq):
    return [q.clone() for q in torch.nn.functional.normalize(torch.randn(n_q, lq, 128, generator=g), dim=-1).to(torch.bfloat16)]


def _ragged_queries(g):
    return _rows(g, [50, 7, 40])                     # 97 tokens: 7 units, the queries' borders inside units


def _plant_zero(p, row, col):
    p.view(torch.int16)[row, col] = 0                # 0x0000: a value the 13-bit code cannot hold


def _doc_flags(ps):
    """1 = the document holds a bf16 value the 13-bit code cannot hold (exponent outside 96..127): scored from the blob.  A few of
    the random rows' 21 million values are that small by themselves."""
    def bad(p):
        e = (p.view(torch.int16).numpy().view(np.uint16).astype(np.uint32) >> 7) & 0xFF
        return bool(((e < 96) | (e > 127)).any())
    return np.array([1 if p.numel() and bad(p) else 0 for p in ps], dtype=np.uint8)


@pytest.fixture(scope="module")
def docs(gw):
    """2 GW + 37 documents: every wave walks two or three of them, of every length of the cycle"""
    g = torch.Generator().manual_seed(2024)
    n_d = 2 * gw + 37
    return _rows(g, [LEN_CYCLE[i % len(LEN_CYCLE)] for i in range(n_d)])


@pytest.fixture(scope="module")
def docs_flagged(docs, gw):
    """the same corpus with an exact zero in documents c, c + GW, c + 2 GW (one wave skips three in a row), in the last document and
    at the front.  Document 0 is the cycle's empty one and has no value to replace (the producer skips it for having no slab), so
    the zero at the front goes into document 1: the first document of its wave, skipped by the prologue's request."""
    ps = [p.clone() for p in docs]
    c = 13                                           # 64 rows, like c + GW and c + 2 GW (GW is a multiple of 8)
    where = [1, c, c + gw, c + 2 * gw, len(ps) - 1]
    assert len(ps) - 1 > c + 2 * gw and ps[0].shape[0] == 0
    for k, d in enumerate(where):
        assert ps[d].shape[0] > 0
        _plant_zero(ps[d], ps[d].shape[0] - 1, (17 * k + 5) % 128)
    return ps, where


_oracle_cache = {}


def _oracle(key, qs, ps, mode="f32"):
    """computed once per (corpus, queries, mode) and shared"""
    if key not in _oracle_cache:
        out = mo.score_multi_vector([q.float().numpy() for q in qs], [p.float().numpy() for p in ps], batch_size=BLOCK, mode=mode)
        out.setflags(write=False)
        _oracle_cache[key] = out
    return _oracle_cache[key]


def _err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))


def _both_paths(amd, monkeypatch, qs, ps, **kw):
    """(packed scan, plain path on a bare copy of the corpus), both as CPU tensors; the packed scan only counts if an image exists"""
    q = amd.pack_queries(qs, DEV)
    corpus = amd.pack_passages(ps, DEV, batch_size=BLOCK)
    assert corpus.pack13() and corpus._pack13 is not None
    packed = amd.maxsim_scores(q, corpus, **kw).cpu()
    assert corpus._pack13 is not None
    bare = dataclasses.replace(corpus, _pack13=None, _pack13_note=None)
    with monkeypatch.context() as m:
        m.setenv("COLPALI_AMD_PACK13", "0")
        plain = amd.maxsim_scores(q, bare, **kw).cpu()
    assert bare._pack13 is None
    return packed, plain, corpus


def _check(packed, plain, want):
    e_packed, e_plain = _err(packed.numpy(), want), _err(plain.numpy(), want)
    print(f"max rel err vs oracle: packed {e_packed:.3e}, plain {e_plain:.3e}")
    assert e_packed <= RTOL and e_plain <= RTOL
    assert torch.equal(packed.view(torch.int32), plain.view(torch.int32))


def _case_queries(case):
    g = torch.Generator().manual_seed(500 + 31 * case)
    return _ragged_queries(g) if case == len(DENSE) else _queries(g, *DENSE[case])


@pytest.mark.parametrize("case", range(len(DENSE) + 1), ids=[f"{n}x{l}" for n, l in DENSE] + ["ragged3"])
def test_more_than_two_rounds_of_waves(amd, monkeypatch, docs, case):
    qs = _case_queries(case)
    n_tok = sum(q.shape[0] for q in qs)
    assert 65 <= n_tok <= 128                        # 5-8 units: the 2-slot ring
    packed, plain, _ = _both_paths(amd, monkeypatch, qs, docs)
    _check(packed, plain, _oracle(("docs", case), qs, docs))


@pytest.mark.parametrize("case", range(len(DENSE) + 1), ids=[f"{n}x{l}" for n, l in DENSE] + ["ragged3"])
def test_skipped_documents_and_the_list_launch(amd, monkeypatch, docs_flagged, case):
    ps, where = docs_flagged
    qs = _case_queries(case)
    packed, plain, corpus = _both_paths(amd, monkeypatch, qs, ps)
    flagged = corpus._pack13.flagged.cpu().numpy()
    assert np.array_equal(flagged, _doc_flags(ps)) and all(flagged[d] for d in where)
    assert corpus._pack13.n_flagged == int(flagged.sum()) >= len(where)     # both the packed scan and the list launch ran
    _check(packed, plain, _oracle(("flagged", case), qs, ps))


@pytest.mark.parametrize("case", range(len(DENSE) + 1), ids=[f"{n}x{l}" for n, l in DENSE] + ["ragged3"])
def test_three_documents_most_requests_dead(amd, monkeypatch, case):
    g = torch.Generator().manual_seed(77)
    ps = _rows(g, [33, 1, 96])
    qs = _case_queries(case)
    packed, plain, _ = _both_paths(amd, monkeypatch, qs, ps)
    _check(packed, plain, _oracle(("three", case), qs, ps))


def test_clamp0_decides_at_eight_units(amd, monkeypatch, docs):
    """all similarities negative: every clamped document scores exactly 0, every unclamped one (96 rows) below 0"""
    g = torch.Generator().manual_seed(900)
    ps = [p.abs() for p in docs]
    qs = [-q.abs() for q in _queries(g, 4, 32)]
    packed, plain, corpus = _both_paths(amd, monkeypatch, qs, ps)
    assert corpus.clamp0 is not None and bool(corpus.clamp0.any()) and not bool(corpus.clamp0.all())
    want = _oracle(("clamp", 0), qs, ps)
    assert bool((want == 0).any()) and bool((want < 0).any())
    _check(packed, plain, want)


def test_ref_rounding_at_eight_units(amd, monkeypatch, docs):
    """the literal tier (ref_rounding=True: the reference's bf16 roundings of the token maxima and of the sum) against the oracle's
    literal tier: within 1e-5 like every case here, and within the bound tests/test_gpu_parity.py sets for the tier"""
    g = torch.Generator().manual_seed(901)
    qs = _queries(g, 4, 32)
    packed, plain, _ = _both_paths(amd, monkeypatch, qs, docs, ref_rounding=True)
    want = _oracle(("ref", 0), qs, docs, mode="bf16ref")
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 1e-3))) - 7)
    for got in (packed.numpy(), plain.numpy()):
        print(f"literal tier: max |got - want| / ulp {float(np.max(np.abs(got - want) / ulp)):.3f}, equal {float(np.mean(got == want)):.4f}")
        assert _err(got, want) <= RTOL
        assert np.all(np.abs(got - want) <= ulp) and np.mean(got == want) > 0.9
    assert torch.equal(packed.view(torch.int32), plain.view(torch.int32))
