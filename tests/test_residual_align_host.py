"""Rows out of a residual-compressed shard without a GPU: the header and the binding of msim_res_align_candidates and
msim_res_gather_pages, their refusals before any device work, the retriever's and the live shard's routing with an injected stand-in
for the kernel, and the Python-side refusals that need no device."""
import os
import re

import pytest
import torch

from tests.test_live_residual_host import _codec, _hooks, _page
from tests.test_residual_scan_host import _shards

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _align_call(L, dtype=0, qt=FAKE, q_off=FAKE, n_q=2, q_rows=7, T=5, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
                clamp=None, n_d=10, d_rows=100, dim=128, cand=FAKE, m=3, ld=3, id_base=0, bs=FAKE, br=FAKE, sims=None, R=20):
    return L.msim_res_align_candidates(dtype, qt, q_off, n_q, q_rows, T, codes, res, C, K, w, bits, d_off, clamp, n_d, d_rows, dim, cand, m,
                                       ld, id_base, bs, br, sims, R, None)


def _gather_call(L, dtype=0, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, dim=128, d_rows=100, d_off=FAKE, n_d=10, id_base=0,
                 ids=FAKE, n_slots=6, pad=20, out=FAKE, lengths=FAKE):
    return L.msim_res_gather_pages(dtype, codes, res, C, K, w, bits, dim, d_rows, d_off, n_d, id_base, ids, n_slots, pad, out, lengths, None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    # nothing to do: 0 before any pointer or format is looked at
    assert _align_call(L, n_q=0) == 0 and _align_call(L, m=0) == 0 and _gather_call(L, n_slots=0) == 0
    assert _align_call(L, n_q=0, qt=None, cand=None, bs=None, C=None, K=100, bits=3, dim=7) == 0
    assert _gather_call(L, n_slots=0, ids=None, out=None, lengths=None, C=None, K=100, bits=3) == 0
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(T=-1), dict(R=-1), dict(qt=None),
               dict(q_off=None), dict(codes=None), dict(res=None), dict(C=None), dict(w=None), dict(d_off=None), dict(cand=None),
               dict(bs=None), dict(br=None), dict(qt=FAKE + 8), dict(C=FAKE + 8), dict(res=FAKE + 4), dict(codes=FAKE + 1), dict(w=FAKE + 2),
               dict(q_off=FAKE + 2), dict(d_off=FAKE + 2), dict(cand=FAKE + 4), dict(bs=FAKE + 2), dict(br=FAKE + 1), dict(sims=FAKE + 2),
               dict(ld=2)):
        assert _align_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=320), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8), dict(K=100), dict(K=0),
               dict(K=4096), dict(K=300), dict(T=129), dict(d_rows=1 << 31)):
        assert _align_call(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_slots=-1), dict(n_d=-1), dict(d_rows=-1), dict(pad=-1), dict(ids=None), dict(lengths=None), dict(d_off=None),
               dict(codes=None), dict(res=None), dict(C=None), dict(w=None), dict(out=None), dict(out=FAKE + 8), dict(C=FAKE + 8),
               dict(res=FAKE + 2), dict(codes=FAKE + 1), dict(w=FAKE + 2), dict(ids=FAKE + 4), dict(d_off=FAKE + 2), dict(lengths=FAKE + 2)):
        assert _gather_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dim=320), dict(bits=3), dict(K=100), dict(K=4096), dict(d_rows=1 << 31), dict(pad=1 << 31),
               dict(n_slots=1 << 31)):
        assert _gather_call(L, **kw) == EUNSUPPORTED, kw


def test_header_and_binding():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"\bint\s+msim_res_align_candidates\s*\(\s*int dtype,", header)
    assert re.search(r"\bint\s+msim_res_gather_pages\s*\(\s*int dtype,", header)
    text = " ".join(header.split()).replace(" * ", " ")
    for phrase in ("exactly the bits msim_align_candidates gives the same queries and list over the output of msim_res_decode_rows",
                   "exactly the bytes msim_gather_pages (row_bytes 256) gives the same ids over that decoded output",
                   "Every byte of out is written", "hipGraph-capturable"):
        assert phrase in text, phrase
    assert "rc.decompress(ids)" not in header
    L = colpali_amd._lib.lib()
    assert len(L.msim_res_align_candidates.argtypes) == 26 and len(L.msim_res_gather_pages.argtypes) == 18
    assert L.msim_abi_version() == 22 == colpali_amd._lib.ABI_VERSION
    for name in ("residual_align", "residual_gather_pages"):
        assert callable(getattr(colpali_amd, name)) and name in colpali_amd.__all__
    assert colpali_amd.residual_align in colpali_amd.retrieval._KERNELS


# ------------------------------------------------------------------------------------------------------------------ routing
class AlignStub:
    """stands in for residual_align: records what it was handed"""

    def __init__(self):
        self.calls = []

    def __call__(self, queries, corpus, ids, maps=False):
        import colpali_amd as amd

        self.calls.append((queries, corpus, ids.clone(), maps))
        n_q, m = ids.shape
        return amd.Alignment(torch.zeros(n_q, m, 1), torch.zeros(n_q, m, 1, dtype=torch.int32), ids.clone())


def test_the_retriever_refuses_by_default_and_hands_an_injected_align_the_queries():
    amd, g, packed, rc, q, labels = _shards()
    cand = torch.tensor([[100, 105, -1], [101, 999, 107], [122, 100, 100], [103, 104, 3]])
    for r in (amd.ShardedRetriever(rc), amd.ShardedRetriever(rc, score_fn=lambda *a: None)):      # the scan's opt-in does not open align
        with pytest.raises(NotImplementedError, match="ResidualCorpus") as e:
            r.align(q, cand)
        assert "score_fn=residual_scores" in str(e.value) and "align_fn=residual_align" in str(e.value)
    stub = AlignStub()
    out = amd.ShardedRetriever(rc, align_fn=stub).align(q, cand, maps=True)
    (queries, corpus, ids, maps), = stub.calls
    assert queries is q and corpus is rc and torch.equal(ids, cand) and maps is True and torch.equal(out.ids, cand)
    # the kernel itself is a hook the retriever packs for: with host queries and no GPU the packer, not the refusal, answers
    r = amd.ShardedRetriever(rc, align_fn=amd.residual_align)
    assert r._align is amd.residual_align
    with pytest.raises(RuntimeError):
        r.align(q, cand)
    with pytest.raises(ValueError, match="maps=True"):
        amd.ShardedRetriever(rc, world=2, rank=0, dist=object(), align_fn=stub).align(q, cand, maps=True)


def test_the_live_shard_maps_deleted_ids_to_minus_one_before_the_align():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(3)
    C, cut, w = _codec(g, 2)
    stub = AlignStub()
    live = amd.LiveResidualCorpus(C, cut, w, 2, 60, 8, id_base=40, align_fn=stub, **_hooks())
    ids = live.add([_page(g, n) for n in (3, 5, 1, 4, 2)])
    assert ids.tolist() == [40, 41, 42, 43, 44]
    live.delete([41, 43])
    q = [_page(g, 4), _page(g, 2)]
    lists = torch.tensor([[40, 41, 42, 43], [44, 45, -1, 39]])
    for state in ("deleted", "compacted"):
        live.align(q, lists, maps=(state == "compacted"))
        queries, corpus, seen, maps = stub.calls[-1]
        assert queries is q and isinstance(corpus, amd.ResidualCorpus) and len(corpus) == 5 and corpus.id_base == 40, state
        assert seen.tolist() == [[40, -1, 42, -1], [44, -1, -1, -1]] and maps is (state == "compacted"), state
        live.compact()
    assert corpus.lengths.tolist() == [3, 0, 1, 0, 2]
    # the default hook is the kernel
    assert amd.LiveResidualCorpus(C, cut, w, 2, 20, 4)._align_fn is amd.residual_align


# ------------------------------------------------------------------------------------------------------------------ refusals in Python
def _host_packed(amd, lens, dtype=torch.bfloat16, width=128):
    off = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32)
    return amd.PackedQueries(tokens=torch.zeros(max(int(off[-1]), 1), width, dtype=dtype), offsets=off, offsets_host=off.clone())


def test_python_refusals_that_need_no_device():
    amd, g, packed, rc, q, labels = _shards()
    ids = torch.zeros((len(q), 2), dtype=torch.int64) + 100
    for fn in (amd.residual_align, amd.align):                            # align dispatches on the container
        with pytest.raises(NotImplementedError, match="width 128"):       # width 320
            fn(torch.zeros(4, 6, 320, dtype=torch.bfloat16), rc, ids)
        with pytest.raises(RuntimeError, match="one dtype"):              # fp32 queries against a bf16 shard; f16 against bf16
            fn(q.float(), rc, ids)
        with pytest.raises(RuntimeError, match="one dtype"):
            fn(q.to(torch.float16), rc, ids)
        with pytest.raises(ValueError, match="max_rows"):
            fn(q, rc, ids, max_rows=-1)
        with pytest.raises(NotImplementedError, match="at most 128 tokens"):
            fn(_host_packed(amd, [3, 129, 4, 1]), rc, ids)
        pq = _host_packed(amd, [3, 128, 4, 0])
        for wrong in (ids.to(torch.int32), ids[0], ids[:3], ids.tolist()):   # dtype, rank, number of rows, not a tensor
            with pytest.raises(ValueError, match="ids"):
                fn(pq, rc, wrong)
        with pytest.raises(RuntimeError, match="MI355X"):                  # everything checks out: the kernel needs its device
            fn(pq, rc, ids)
    with pytest.raises(ValueError, match="ResidualCorpus"):
        amd.residual_align(q, packed, ids)
    for fn in (amd.residual_gather_pages, amd.gather_pages):
        with pytest.raises(ValueError, match="pad_to"):
            fn(rc, ids, -1)
        with pytest.raises(ValueError, match="int64"):
            fn(rc, ids.to(torch.int32))
        longest = int(rc.lengths.max())
        with pytest.raises(ValueError, match=f"pad_to={longest - 1}"):    # host ids are checked against the lengths
            fn(rc, torch.arange(100, 100 + len(rc)), longest - 1)
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(rc, ids)
    with pytest.raises(ValueError, match="ResidualCorpus"):
        amd.residual_gather_pages(packed, ids)
