"""Rows out of a 320-wide residual-compressed shard without a GPU: the header and the binding of msim_res_wide_align_candidates and
msim_res_wide_gather_pages, their refusals before any device work, the routing of align / gather_pages / ShardedRetriever(align_fn=)
with stand-ins for the kernels, and the Python-side refusals that need no device."""
import os
import re

import pytest
import torch

from tests.test_residual_align_host import AlignStub
from tests.test_residual_scan_host import _shards as _narrow_shards
from tests.test_residual_wide_scan_host import _shards

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
W = 320


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def _align_call(L, dtype=0, qt=FAKE, q_off=FAKE, n_q=2, q_rows=7, T=5, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, d_off=FAKE,
                clamp=None, n_d=10, d_rows=100, dim=W, cand=FAKE, m=3, ld=3, id_base=0, bs=FAKE, br=FAKE, sims=None, R=20,
                entry="msim_res_wide_align_candidates"):
    return getattr(L, entry)(dtype, qt, q_off, n_q, q_rows, T, codes, res, C, K, w, bits, d_off, clamp, n_d, d_rows, dim, cand, m, ld,
                             id_base, bs, br, sims, R, None)


def _gather_call(L, dtype=0, codes=FAKE, res=FAKE, C=FAKE, K=256, w=FAKE, bits=2, dim=W, d_rows=100, d_off=FAKE, n_d=10, id_base=0,
                 ids=FAKE, n_slots=6, pad=20, out=FAKE, lengths=FAKE, entry="msim_res_wide_gather_pages"):
    return getattr(L, entry)(dtype, codes, res, C, K, w, bits, dim, d_rows, d_off, n_d, id_base, ids, n_slots, pad, out, lengths, None)


def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    # nothing to do: 0 before any pointer or format is looked at
    assert _align_call(L, n_q=0) == 0 and _align_call(L, m=0) == 0 and _gather_call(L, n_slots=0) == 0
    assert _align_call(L, n_q=0, qt=None, cand=None, bs=None, C=None, K=100, bits=3, dim=7) == 0
    assert _align_call(L, m=0, qt=None, cand=None, bs=None, C=None, K=100, bits=3, dim=7) == 0
    assert _gather_call(L, n_slots=0, ids=None, out=None, lengths=None, C=None, K=100, bits=3, dim=7) == 0
    # negative sizes, null and misaligned pointers (Qt, centroids, residuals, out: 16; cand / ids: 8; codes: 2; the rest: 4), ld_cand < m,
    # and a centroid count outside 256 .. 2048 or no multiple of 256: the code the format check of every msim_res_wide_* entry gives it
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(T=-1), dict(R=-1), dict(qt=None),
               dict(q_off=None), dict(codes=None), dict(res=None), dict(C=None), dict(w=None), dict(d_off=None), dict(cand=None),
               dict(bs=None), dict(br=None), dict(qt=FAKE + 8), dict(C=FAKE + 8), dict(res=FAKE + 4), dict(codes=FAKE + 1), dict(w=FAKE + 2),
               dict(q_off=FAKE + 2), dict(d_off=FAKE + 2), dict(cand=FAKE + 4), dict(bs=FAKE + 2), dict(br=FAKE + 1), dict(sims=FAKE + 2),
               dict(ld=2), dict(K=100), dict(K=0), dict(K=4096), dict(K=300), dict(K=-256)):
        assert _align_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=128), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8), dict(T=129),
               dict(d_rows=1 << 31), dict(n_q=1 << 16, m=1 << 15, ld=1 << 15)):
        assert _align_call(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_slots=-1), dict(n_d=-1), dict(d_rows=-1), dict(pad=-1), dict(ids=None), dict(lengths=None), dict(d_off=None),
               dict(codes=None), dict(res=None), dict(C=None), dict(w=None), dict(out=None), dict(out=FAKE + 8), dict(C=FAKE + 8),
               dict(res=FAKE + 2), dict(codes=FAKE + 1), dict(w=FAKE + 2), dict(ids=FAKE + 4), dict(d_off=FAKE + 2), dict(lengths=FAKE + 2),
               dict(K=100), dict(K=0), dict(K=4096), dict(K=300)):
        assert _gather_call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=128), dict(dim=64), dict(bits=1), dict(bits=3), dict(bits=8), dict(d_rows=1 << 31),
               dict(pad=1 << 31), dict(n_slots=1 << 31)):
        assert _gather_call(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    # the two 128-wide entries keep refusing width 320
    assert _align_call(L, entry="msim_res_align_candidates") == EUNSUPPORTED
    assert _gather_call(L, entry="msim_res_gather_pages") == EUNSUPPORTED


def test_header_and_binding():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"\bint\s+msim_res_wide_align_candidates\s*\(\s*int dtype,", header)
    assert re.search(r"\bint\s+msim_res_wide_gather_pages\s*\(\s*int dtype,", header)
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    block = header[header.index("ROWS OUT OF THE COMPRESSED SHARD AT WIDTH 320"):header.index("int msim_res_wide_align_candidates(")]
    text = " ".join(block.split()).replace(" * ", " ")
    for phrase in ("exactly the bits msim_align_candidates (dim 320) gives the same queries and list over the output of "
                   "msim_res_wide_decode_rows", "exactly the bytes msim_gather_pages (row_bytes 640) gives the same ids over that decoded output",
                   "Every byte of out is written", "hipGraph-capturable", "a K outside that range is MSIM_EINVAL", "-inf / 0.0 / NaN / -1"):
        assert phrase in text, phrase
    L = colpali_amd._lib.lib()
    assert L.msim_res_wide_align_candidates.argtypes == L.msim_res_align_candidates.argtypes
    assert L.msim_res_wide_gather_pages.argtypes == L.msim_res_gather_pages.argtypes
    assert len(L.msim_res_wide_align_candidates.argtypes) == 26 and len(L.msim_res_wide_gather_pages.argtypes) == 18
    assert L.msim_abi_version() == 22 == colpali_amd._lib.ABI_VERSION
    for name in ("residual_wide_align", "residual_wide_gather_pages"):
        assert callable(getattr(colpali_amd, name)) and name in colpali_amd.__all__ and name in colpali_amd.__doc__
    assert colpali_amd.residual_wide_align in colpali_amd.retrieval._KERNELS
    assert colpali_amd.ResidualWideCorpus._ALIGN == "msim_res_wide_align_candidates"
    assert colpali_amd.ResidualWideCorpus._GATHER == "msim_res_wide_gather_pages"


# ------------------------------------------------------------------------------------------------------------------ routing
def test_align_and_gather_pages_dispatch_on_the_container(monkeypatch):
    amd, g, packed, rc, q, labels = _shards()
    ids = torch.zeros((len(q), 2), dtype=torch.int64) + 100
    seen = []
    monkeypatch.setattr(amd.residual_wide, "residual_wide_align", lambda *a, **kw: seen.append(("align", a, kw)) or "aligned")
    monkeypatch.setattr(amd.residual_wide, "residual_wide_gather_pages", lambda *a: seen.append(("gather", a)) or "gathered")
    assert amd.align(q, rc, ids, maps=True, max_rows=9) == "aligned"
    assert amd.gather_pages(rc, ids, 12, None) == "gathered"
    (_, a, kw), (_, b) = seen
    assert a[0] is q and a[1] is rc and a[2] is ids and kw == dict(maps=True, max_rows=9)
    assert b[0] is rc and b[1] is ids and b[2] == 12 and b[3] is None
    # a 128-wide shard does not come here
    namd, _, _, narrow, nq, _ = _narrow_shards()
    with pytest.raises(RuntimeError, match="MI355X"):
        amd.align(nq, narrow, ids)
    with pytest.raises(RuntimeError, match="MI355X"):
        amd.gather_pages(narrow, ids)
    assert len(seen) == 2


def test_the_retriever_refuses_by_default_and_hands_an_injected_align_the_queries():
    amd, g, packed, rc, q, labels = _shards()
    cand = torch.tensor([[100, 105, -1], [101, 999, 107], [122, 100, 100], [103, 104, 3]])
    for r in (amd.ShardedRetriever(rc), amd.ShardedRetriever(rc, score_fn=amd.residual_wide_scores),
              amd.ShardedRetriever(rc, score_fn=lambda *a: None)):        # the scan's opt-in does not open align
        with pytest.raises(NotImplementedError, match="ResidualWideCorpus.*width 128 only") as e:
            r.align(q, cand)
        assert "score_fn=residual_wide_scores" in str(e.value) and "align_fn=residual_align" not in str(e.value)
        assert "align_fn=residual_wide_align" in str(e.value)              # the hook that exists at this width
    stub = AlignStub()
    out = amd.ShardedRetriever(rc, align_fn=stub).align(q, cand, maps=True)
    (queries, corpus, ids, maps), = stub.calls
    assert queries is q and corpus is rc and torch.equal(ids, cand) and maps is True and torch.equal(out.ids, cand)
    # the kernel itself is a hook the retriever packs for: with host queries and no GPU the packer, not the refusal, answers
    r = amd.ShardedRetriever(rc, align_fn=amd.residual_wide_align)
    assert r._align is amd.residual_wide_align
    with pytest.raises(RuntimeError):
        r.align(q, cand)
    # the 128 hook keeps refusing the wide shard, by its type
    with pytest.raises(NotImplementedError, match="width 128"):
        amd.ShardedRetriever(rc, align_fn=amd.residual_align).align(amd.PackedQueries(
            tokens=torch.zeros(4, W, dtype=torch.bfloat16), offsets=torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32),
            offsets_host=torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32)), cand)
    with pytest.raises(ValueError, match="maps=True"):
        amd.ShardedRetriever(rc, world=2, rank=0, dist=object(), align_fn=stub).align(q, cand, maps=True)


# ------------------------------------------------------------------------------------------------------------------ refusals in Python
def _host_packed(amd, lens, dtype=torch.bfloat16, width=W):
    off = torch.tensor([sum(lens[:i]) for i in range(len(lens) + 1)], dtype=torch.int32)
    return amd.PackedQueries(tokens=torch.zeros(max(int(off[-1]), 1), width, dtype=dtype), offsets=off, offsets_host=off.clone())


def test_python_refusals_that_need_no_device():
    amd, g, packed, rc, q, labels = _shards()
    ids = torch.zeros((len(q), 2), dtype=torch.int64) + 100
    for fn in (amd.residual_wide_align, amd.align):                       # align dispatches on the container
        with pytest.raises(NotImplementedError, match="width 320"):       # width 128
            fn(torch.zeros(4, 6, 128, dtype=torch.bfloat16), rc, ids)
        with pytest.raises(RuntimeError, match="one dtype"):              # fp32 queries against a bf16 shard; f16 against bf16
            fn(q.float(), rc, ids)
        with pytest.raises(RuntimeError, match="one dtype"):
            fn(q.to(torch.float16), rc, ids)
        with pytest.raises(ValueError, match="max_rows"):
            fn(q, rc, ids, max_rows=-1)
        with pytest.raises(NotImplementedError, match="at most 128 tokens"):
            fn(_host_packed(amd, [3, 129, 4, 1]), rc, ids)
        pq = _host_packed(amd, [3, 128, 4, 0])
        for wrong in (ids.to(torch.int32), ids[0], ids[:3], ids.tolist(), ids.to("meta")):   # dtype, rank, rows, not a tensor, device
            with pytest.raises(ValueError, match="ids"):
                fn(pq, rc, wrong)
        with pytest.raises(RuntimeError, match="MI355X"):                  # everything checks out: the kernel needs its device
            fn(pq, rc, ids)
    # an fp32 shard cannot be built; fp32 queries AND an fp32-typed container are a format the kernels do not have
    f32 = amd.ResidualWideCorpus.__new__(amd.ResidualWideCorpus)
    f32.__dict__.update(rc.__dict__)
    f32.centroids = rc.centroids.float()
    with pytest.raises(NotImplementedError, match="bfloat16 / float16 embeddings of width 320"):
        amd.residual_wide_align(q.float(), f32, ids)
    # the sibling class and a plain corpus
    _, _, npacked, narrow, nq, _ = _narrow_shards()
    for call in (lambda: amd.residual_wide_align(nq, narrow, ids), lambda: amd.residual_wide_gather_pages(narrow, ids)):
        with pytest.raises(NotImplementedError, match="ResidualWideCorpus exists at width 320 only"):
            call()
    for call in (lambda: amd.residual_align(q, rc, ids), lambda: amd.residual_gather_pages(rc, ids)):
        with pytest.raises(NotImplementedError, match="width 128"):
            call()
    with pytest.raises(ValueError, match="ResidualWideCorpus"):
        amd.residual_wide_align(q, packed, ids)
    for fn in (amd.residual_wide_gather_pages, amd.gather_pages):
        with pytest.raises(ValueError, match="pad_to"):
            fn(rc, ids, -1)
        with pytest.raises(ValueError, match="int64"):
            fn(rc, ids.to(torch.int32))
        with pytest.raises(ValueError, match="int64"):
            fn(rc, ids.tolist())
        with pytest.raises(ValueError, match="different devices"):
            fn(rc, ids.to("meta"))
        longest = int(rc.lengths.max())
        with pytest.raises(ValueError, match=f"pad_to={longest - 1}"):    # host ids are checked against the lengths
            fn(rc, torch.arange(100, 100 + len(rc)), longest - 1)
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(rc, ids)
    with pytest.raises(ValueError, match="ResidualWideCorpus"):
        amd.residual_wide_gather_pages(packed, ids)
