"""K1s13's operand decode and the priority turns of its 2-slot forms (maxsim_stream13.hip: DECODE, PRIO): the scores of the packed
scan carry the bits of the raw K1s scan whatever bf16 pattern the image holds, and the decode is right on its own account.

Two witnesses.  (1) The raw K1s scan of the same blob (COLPALI_AMD_PACK13=0 on a corpus object without an image): bit equality,
over every representable pattern -- both signs, exponent fields 96..127, all mantissas -- at every unit count and with enough
documents that every wave of a full grid scores several, and over documents long enough that a 5-8-unit wave passes its priority
swap (every 32 slabs).  (2) Arithmetic that
needs no other kernel: 128 one-hot query tokens make every product exact, so token k's maximum over a document is max_r D[r, k] and a
score is the fp32 sum of 32 such maxima.
"""
import dataclasses

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 130]
N_DOCS = 13 * 539                       # 7007 documents: a full grid of the 2-slot forms is 2048 waves
ZERO_DOCS = [1, 14, 500, 1003, 2222, 3456, 4100, 5555, 6001, 6999, 7005]        # +0.0 / -0.0 planted: flagged, scored from the blob


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()  # must load: no fallback
    return colpali_amd


def _patterns(g, rows):
    """[rows, 128] bf16 drawn from the whole set the 13-bit code holds: sign, exponent field 96..127, 7 mantissa bits"""
    sign = torch.randint(0, 2, (rows, 128), generator=g, dtype=torch.int32)
    exp = torch.randint(96, 128, (rows, 128), generator=g, dtype=torch.int32)
    man = torch.randint(0, 128, (rows, 128), generator=g, dtype=torch.int32)
    bits = ((sign << 15) | (exp << 7) | man).numpy().astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)


def _corpus(amd, blob, lens):
    from colpali_amd.corpus import PackedCorpus

    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return PackedCorpus(blob=blob.to(DEV).contiguous(), offsets=torch.from_numpy(off.astype(np.int32)).to(DEV), clamp0=None,
                        lengths=torch.tensor(lens, dtype=torch.int64))


@pytest.fixture(scope="module")
def every_pattern(amd):
    """(corpus with its image, the planted documents' flags, a clamp0 mask): built once, never changed"""
    g = torch.Generator().manual_seed(1300)
    lens = (LENS * (N_DOCS // len(LENS)))[:N_DOCS]
    blob = _patterns(g, sum(lens))
    off = np.concatenate([[0], np.cumsum(lens)])
    raw = blob.view(torch.int16)
    flags = np.zeros(N_DOCS, dtype=np.uint8)
    for i, c in enumerate(ZERO_DOCS):
        assert lens[c] > 0
        raw[int(off[c]) + (i * 7) % lens[c], (i * 37) % 128] = 0 if i % 2 else -32768          # +0.0 / -0.0
        flags[c] = 1
    corpus = _corpus(amd, blob, lens)
    assert corpus.pack13() and corpus._pack13 is not None
    assert np.array_equal(corpus._pack13.flagged.cpu().numpy(), flags)
    clamp = (torch.rand(N_DOCS, generator=g) < 0.5).to(torch.uint8).to(DEV)
    return corpus, flags, clamp


def _plain(amd, monkeypatch, q, corpus):
    """the witness: the same blob through the raw K1s"""
    bare = dataclasses.replace(corpus, _pack13=None, _pack13_note=None)
    with monkeypatch.context() as m:
        m.setenv("COLPALI_AMD_PACK13", "0")
        out = amd.maxsim_scores(q, bare)
    assert bare._pack13 is None
    return out


def _packed(amd, q, corpus):
    assert corpus._pack13 is not None
    out = amd.maxsim_scores(q, corpus)
    assert corpus._pack13 is not None
    return out


def _ragged_queries(amd, g, n_q, total):
    """n_q queries of uneven lengths, `total` tokens in all, every query at least one"""
    lens = [1] * n_q
    for t in range(total - n_q):
        lens[(t * t + t // 3) % n_q] += 1
    assert sum(lens) == total and min(lens) >= 1
    rows = torch.nn.functional.normalize(torch.randn(total, 128, generator=g), dim=-1).to(torch.bfloat16)
    return amd.pack_queries([t.clone() for t in rows.split(lens)], DEV, compact=False)


@pytest.mark.parametrize("nu", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_operand_bit_position(amd, monkeypatch, every_pattern, nu):
    corpus, _flags, clamp = every_pattern
    g = torch.Generator().manual_seed(1310 + nu)
    for total in (16 * nu, 16 * nu - 5, 16 * (nu - 1) + 1):
        q = _ragged_queries(amd, g, min(nu, total), total)           # 1..8 queries
        unclamped = None
        for mask in (None, clamp):
            c = dataclasses.replace(corpus, clamp0=mask)             # the same blob, offsets and image
            assert c._pack13 is corpus._pack13 and c.pack13()
            got, want = _packed(amd, q, c), _plain(amd, monkeypatch, q, c)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (nu, total, mask is not None)
            if mask is None:
                unclamped = want
            else:
                assert not torch.equal(want, unclamped)              # the mask reaches the kernels


@pytest.mark.parametrize("nu", [5, 8])
def test_priority_swaps_inside_long_documents(amd, monkeypatch, nu):
    """The 2-slot forms swap the priority of a SIMD's two waves every 32 consumed slabs: documents of 33 slabs (the last one half
    full), more of them than a full grid has waves, so every wave passes the swap and some pass it twice.  Patterns made on the device."""
    g = torch.Generator(device=DEV).manual_seed(1330 + nu)
    n_docs, rows = 2100, 32 * 32 + 16
    bits = ((torch.randint(0, 2, (n_docs * rows, 128), generator=g, device=DEV, dtype=torch.int32) << 15)
            | (torch.randint(96, 128, (n_docs * rows, 128), generator=g, device=DEV, dtype=torch.int32) << 7)
            | torch.randint(0, 128, (n_docs * rows, 128), generator=g, device=DEV, dtype=torch.int32))
    blob = (bits - ((bits >> 15) << 16)).to(torch.int16).view(torch.bfloat16)            # the low 16 bits, as they stand
    del bits
    corpus = _corpus(amd, blob, [rows] * n_docs)
    assert corpus.pack13() and corpus._pack13 is not None and corpus._pack13.n_flagged == 0
    q = _ragged_queries(amd, torch.Generator().manual_seed(nu), 4, 16 * nu - 3)
    got, want = _packed(amd, q, corpus), _plain(amd, monkeypatch, q, corpus)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_one_hot_tokens_read_the_column_maxima(amd):
    """No cancellation in the token sum: documents of 15 rows and more, so that the 32 maxima of a score share a sign (all but a
    2^-15 share of them, and those of the smallest magnitudes).  The kernel's sum is six fp32 additions deep (four tokens per lane, then
    three levels across eight lanes): 6 * 2^-24 = 3.6e-7 relative to a sum of like-signed terms, inside the 1e-6 asked for."""
    g = torch.Generator().manual_seed(1320)
    lens = [15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 130] * 200       # 2200 documents: more than the 2048 waves of a full grid
    blob = _patterns(g, sum(lens))
    q = torch.eye(128, dtype=torch.float32).view(4, 32, 128).to(torch.bfloat16).to(DEV).contiguous()
    starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
    for b in (blob, -blob):                                          # negated: the largest value of a column is the smallest magnitude under a set sign bit
        col_max = np.maximum.reduceat(b.float().numpy(), starts, axis=0)                     # [docs, 128], exact
        want = col_max.astype(np.float64).reshape(len(lens), 4, 32).sum(axis=2).T         # [4, docs]
        corpus = _corpus(amd, b, lens)
        assert corpus.pack13() and corpus._pack13 is not None and corpus._pack13.n_flagged == 0
        got = _packed(amd, q, corpus).cpu().numpy().astype(np.float64)
        err = np.abs(got - want) / np.abs(want)
        print(f"one-hot tokens: max relative error {err.max():.3e}")
        assert float(err.max()) <= 1e-6


def test_decode_kernel_still_returns_the_blob(amd, every_pattern):
    from colpali_amd.corpus import pack13_decode

    corpus, flags, _clamp = every_pattern
    keep = torch.repeat_interleave(torch.from_numpy(flags == 0), corpus.lengths).to(DEV)
    back = pack13_decode(corpus).view(torch.int16)
    assert int(keep.sum()) > 0.99 * keep.numel()
    assert torch.equal(back[keep], corpus.blob.view(torch.int16)[keep])
