"""Every refusal of the FP4 index family, word for word, without a GPU: both widths (128: Fp4Index, msim_f4_* / msim_f6_*; 320:
Fp4WideIndex, msim_f4w_* / msim_f6w_*) and both query codes (e2m1, e2m3).

The ABI cases call every encode, scores, scores_plan, candidates and candidates_plan entry with one bad argument at a time --
negative size, wrong width, wrong dtype, null pointer, misalignment, short leading dimension, too many tokens, too large a launch
-- on fake pointers, so nothing touches a device; the Python cases do the same for the class constructors, `build`, the scoring
functions, the quantizers and the rerank functions.  Return code (exception type) and the full text are compared with
tests/golden/fp4_family_refusals.json, which was recorded from the library and the modules as they stood BEFORE the host layer
of the two widths was folded into one (colpali_amd/_fp4_family.py, csrc/abi_fp4_family.hpp): the fold changes no refusal."""
import importlib
import json
import os

import pytest
import torch

FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fp4_family_refusals.json")
WIDTHS, CODES = (128, 320), ("e2m1", "e2m3")
CPU = torch.device("cpu")

ENTRIES = {
    (128, "e2m1"): dict(encode="msim_f4_encode_rows", scores="msim_f4_scores", candidates="msim_f4_candidates"),
    (128, "e2m3"): dict(encode="msim_f6_encode_rows", scores="msim_f4_scores_q6", candidates="msim_f4_candidates_q6"),
    (320, "e2m1"): dict(encode="msim_f4w_encode_rows", scores="msim_f4w_scores", candidates="msim_f4w_candidates"),
    (320, "e2m3"): dict(encode="msim_f6w_encode_rows", scores="msim_f4w_scores_q6", candidates="msim_f4w_candidates_q6"),
}
PLANS = {128: dict(scores_plan="msim_f4_scores_plan", candidates_plan="msim_f4_candidates_plan"),
         320: dict(scores_plan="msim_f4w_scores_plan", candidates_plan="msim_f4w_candidates_plan")}
NAMES = {   # width -> (module, class, scores, scores_from_codes, rerank, {code: quantizer}, {code: (e2m3 scores, e2m3 rerank)})
    128: ("fp4_index", "Fp4Index", "fp4_scores", "fp4_scores_from_codes", "fp4_rerank_scores",
          {"e2m1": "fp4_quantize_queries", "e2m3": "fp6_quantize_queries"}, ("fp6_scores", "fp6_rerank_scores")),
    320: ("fp4_wide_index", "Fp4WideIndex", "fp4_wide_scores", "fp4_wide_scores_from_codes", "fp4_wide_rerank_scores",
          {"e2m1": "fp4_wide_quantize_queries", "e2m3": "fp6_wide_quantize_queries"}, ("fp6_wide_scores", "fp6_wide_rerank_scores")),
}


def _defaults(kind, w):
    """the good arguments of an entry, in its argument order"""
    scan = dict(q=FAKE, qs=FAKE + 1, qo=FAKE, n_q=4, q_rows=40, maxq=32, d4=FAKE, ds=FAKE + 5, do=FAKE, c0=None, n_d=10, d_rows=90, dim=w)
    return {"encode": dict(dtype=0, x=FAKE, n=40, dim=w, codes=FAKE, scales=FAKE + 3, stream=None),
            "scores": dict(scan, out=FAKE, ld=10, stream=None),
            "scores_plan": dict(n_q=4, maxq=32, n_d=10, d_rows=90, plan=FAKE),
            "candidates": dict(scan, cand=FAKE, m=6, ld_cand=6, id_base=0, out=FAKE, ld=6, ids=FAKE, stream=None),
            "candidates_plan": dict(n_q=4, maxq=32, m=6, plan=FAKE)}[kind]


def _bad(kind, w):
    """one bad argument (or one bad pair) at a time; the first three of `encode`, `scores` and `candidates` are good and empty"""
    other = 448 - w
    nulls = lambda *names: [{n: None} for n in names]
    return {
        "encode": [dict(n=0), dict(n=0, x=None, codes=None, scales=None), dict(n=-1), dict(dim=other), dict(dim=64), dict(dim=w // 2),
                   dict(dtype=2), dict(dtype=7), *nulls("x", "codes", "scales"), dict(x=FAKE + 8), dict(codes=FAKE + 4), dict(n=1 << 40)],
        "scores": [dict(n_q=0), dict(n_d=0, q=None, d4=None, out=None), dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1),
                   dict(maxq=-1), dict(dim=other), dict(dim=64), *nulls("q", "qs", "qo", "d4", "ds", "do", "out"), dict(q=FAKE + 4),
                   dict(d4=FAKE + 8), dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9), dict(maxq=(1 << 20) + 1)],
        "scores_plan": [dict(n_q=-1), dict(maxq=-1), dict(n_d=-1), dict(d_rows=-1), dict(maxq=(1 << 20) + 1), dict(plan=None)],
        "candidates": [dict(n_q=0), dict(m=0, ld_cand=0, ld=0), dict(m=0, q=None, qo=None, do=None, cand=None, out=None), dict(n_q=-1),
                       dict(n_d=-1), dict(m=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(dim=other), dict(dim=64),
                       *nulls("q", "qs", "qo", "d4", "ds", "do", "cand", "out"), dict(q=FAKE + 8), dict(d4=FAKE + 4), dict(qo=FAKE + 2),
                       dict(do=FAKE + 1), dict(out=FAKE + 2), dict(cand=FAKE + 4), dict(ids=FAKE + 4), dict(ld_cand=5), dict(ld=5),
                       dict(maxq=129), dict(n_q=1 << 30, m=16, ld_cand=16, ld=16)],
        "candidates_plan": [dict(plan=None), dict(n_q=-1), dict(m=-1), dict(maxq=-1), dict(maxq=129), dict(n_q=1 << 30, m=16)],
    }[kind]


def abi_answers(w, code):
    """{case: [return code, msim_last_error() of a refusal]} of every ABI case of one width and query code"""
    import colpali_amd

    L = colpali_amd._lib.lib()
    got = {}
    for kind, name in {**ENTRIES[w, code], **PLANS[w]}.items():
        for kw in _bad(kind, w):
            rc = getattr(L, name)(*{**_defaults(kind, w), **kw}.values())
            got[f"{name} {kw}"] = [rc, L.msim_last_error().decode() if rc else ""]
    return got


def _python_cases(w, code):
    """{case: (thunk, lifted)}: `lifted` cases run with the GPU requirement lifted (the refusal under test sits behind it)"""
    import colpali_amd
    from colpali_amd.corpus import PackedQueries

    mod_name, cls_name, scores, from_codes, rerank, quant, sixes = NAMES[w]
    cls, scores, from_codes, rerank, quant = (getattr(colpali_amd, n) for n in (cls_name, scores, from_codes, rerank, quant[code]))
    other_cls = getattr(colpali_amd, NAMES[448 - w][1])
    rb = w // 2

    def shard(width=w, dtype=torch.bfloat16):
        return colpali_amd.pack_passages([torch.ones(3, width).to(dtype) for _ in range(5)], CPU, batch_size=None, id_base=7)

    def index(klass=cls, width=w, device=CPU):
        s = shard(width)
        return klass(torch.zeros(15, width // 2, dtype=torch.uint8, device=device), torch.zeros(15, dtype=torch.uint8, device=device),
                     s.offsets.to(device), None, s.lengths, 7)

    def packed(width=w, dtype=torch.bfloat16, tokens=4):
        off = torch.tensor([0, tokens, 2 * tokens], dtype=torch.int32)
        return PackedQueries(tokens=torch.ones(2 * tokens, width).to(dtype), offsets=off, offsets_host=off)

    s, idx, q = shard(), index(), packed()
    good = (idx.codes, idx.scales, s.offsets, None, s.lengths)
    ctor = lambda **kw: (lambda: cls(*{**dict(zip("csoxl", good)), **kw}.values()))
    off = torch.tensor([0, 4, 8], dtype=torch.int32)
    qcodes, qscales = torch.zeros(8, colpali_amd.__dict__[mod_name].QUERY_CODES[code], dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)
    cands = torch.full((2, 3), 7, dtype=torch.int64)
    cases = {
        "ctor codes dtype": ctor(c=torch.zeros(15, rb, dtype=torch.int8)), "ctor codes width": ctor(c=torch.zeros(15, 224 - rb, dtype=torch.uint8)),
        "ctor codes full width": ctor(c=torch.zeros(15, w, dtype=torch.uint8)), "ctor codes 1-D": ctor(c=torch.zeros(15 * rb, dtype=torch.uint8)),
        "ctor codes strided": ctor(c=torch.zeros(rb, 15, dtype=torch.uint8).t()), "ctor scales dtype": ctor(s=torch.zeros(15, dtype=torch.int8)),
        "ctor scales short": ctor(s=torch.zeros(14, dtype=torch.uint8)), "ctor scales 2-D": ctor(s=torch.zeros(15, 1, dtype=torch.uint8)),
        "ctor offsets short": ctor(o=s.offsets[:-1]), "ctor offsets dtype": ctor(o=s.offsets.long()),
        "ctor clamp0 short": ctor(x=torch.zeros(4, dtype=torch.uint8)), "ctor clamp0 dtype": ctor(x=torch.zeros(5, dtype=torch.int8)),
        "build not a corpus": lambda: cls.build(idx), "build a tensor": lambda: cls.build(torch.zeros(15, w)),
        "build sibling width": lambda: cls.build(shard(448 - w)), "build width 64": lambda: cls.build(shard(64)),
        "build float32": lambda: cls.build(shard(dtype=torch.float32)), "build f16 on the host": lambda: cls.build(shard(dtype=torch.float16)),
        "build on the host": lambda: cls.build(s),
        "scores query_code": lambda: scores(q, idx, query_code="e3m2"), "scores query_code None": lambda: scores(q, idx, query_code=None),
        "scores positional query_code": lambda: scores(q, idx, None, code),
        "scores sibling index": lambda: scores(q, index(other_cls, 448 - w), query_code=code),
        "scores a corpus": lambda: scores(q, s, query_code=code), "scores sibling width": lambda: scores(packed(448 - w), idx, query_code=code),
        "scores width 64": lambda: scores(packed(64), idx, query_code=code),
        "scores float32": lambda: scores(packed(dtype=torch.float32), idx, query_code=code),
        "scores dense host queries": lambda: scores(torch.ones(2, 4, w).to(torch.bfloat16), idx, query_code=code),
        "scores on the host": lambda: scores(q, idx, query_code=code),
        "scores other device": lambda: scores(q, index(device=torch.device("meta")), query_code=code),
        "from_codes query_code": lambda: from_codes(qcodes, qscales, off, 4, idx, query_code="fp6"),
        "from_codes sibling code width": lambda: from_codes(torch.zeros(8, rb if code == "e2m3" else 3 * rb // 2, dtype=torch.uint8), qscales, off, 4, idx, query_code=code),
        "from_codes sibling width": lambda: from_codes(torch.zeros(8, 224 - rb, dtype=torch.uint8), qscales, off, 4, idx, query_code=code),
        "from_codes dtype": lambda: from_codes(qcodes.to(torch.int8), qscales, off, 4, idx, query_code=code),
        "from_codes 1-D": lambda: from_codes(qcodes.flatten(), qscales, off, 4, idx, query_code=code),
        "from_codes strided": lambda: from_codes(qcodes.t().contiguous().t(), qscales, off, 4, idx, query_code=code),
        "from_codes on the host": lambda: from_codes(qcodes, qscales, off, 4, idx, query_code=code),
        "from_codes other device": (lambda: from_codes(qcodes, qscales.to("meta"), off, 4, idx, query_code=code), True),
        "from_codes out shape": (lambda: from_codes(qcodes, qscales, off, 4, idx, torch.zeros(2, 4), query_code=code), True),
        "from_codes out dtype": (lambda: from_codes(qcodes, qscales, off, 4, idx, torch.zeros(2, 5, dtype=torch.float64), query_code=code), True),
        "from_codes out strided": (lambda: from_codes(qcodes, qscales, off, 4, idx, torch.zeros(5, 2).t(), query_code=code), True),
        "quantize sibling width": lambda: quant(packed(448 - w)), "quantize width 64": lambda: quant(packed(64)),
        "quantize float32": (lambda: quant(packed(dtype=torch.float32)), True), "quantize sibling width lifted": (lambda: quant(packed(448 - w)), True),
        "quantize on the host": lambda: quant(q), "quantize dense host queries": lambda: quant(torch.ones(2, 4, w).to(torch.bfloat16)),
        "rerank query_code": lambda: rerank(q, idx, cands, query_code="e3m2"),
        "rerank sibling index": lambda: rerank(q, index(other_cls, 448 - w), cands, query_code=code),
        "rerank a corpus": lambda: rerank(q, s, cands, query_code=code), "rerank on the host": lambda: rerank(q, idx, cands, query_code=code),
        "rerank sibling width": (lambda: rerank(packed(448 - w), idx, cands, query_code=code), True),
        "rerank width 64": (lambda: rerank(packed(64), idx, cands, query_code=code), True),
        "rerank float32": (lambda: rerank(packed(dtype=torch.float32), idx, cands, query_code=code), True),
        "rerank other device": (lambda: rerank(q, index(device=torch.device("meta")), cands, query_code=code), True),
        "rerank 129 tokens": (lambda: rerank(packed(tokens=129), idx, cands, query_code=code), True),
    }
    if code == "e2m3":                                                   # the e2m3 functions themselves: no query_code to pass
        six_scores, six_rerank = (getattr(colpali_amd, n) for n in sixes)
        cases.update({
            "fp6 scores takes no query_code": lambda: six_scores(q, idx, query_code="e2m1"),
            "fp6 scores sibling index": lambda: six_scores(q, index(other_cls, 448 - w)),
            "fp6 scores sibling width": lambda: six_scores(packed(448 - w), idx), "fp6 scores on the host": lambda: six_scores(q, idx),
            "fp6 rerank sibling index": lambda: six_rerank(q, index(other_cls, 448 - w), cands),
            "fp6 rerank a corpus": lambda: six_rerank(q, s, cands),
            "fp6 rerank 129 tokens": (lambda: six_rerank(packed(tokens=129), idx, cands), True),
        })
    return {k: v if isinstance(v, tuple) else (v, False) for k, v in cases.items()}


def python_answers(w, code, holders):
    """{case: [exception type, its text]}; `holders`: the modules whose `_require_gpu` the lifted cases replace"""
    got = {}
    for name, (thunk, lifted) in _python_cases(w, code).items():
        saved = [(m, m._require_gpu) for m in holders] if lifted else []
        for m, _ in saved:
            m._require_gpu = torch.device
        try:
            with pytest.raises(Exception) as exc:
                thunk()
        finally:
            for m, fn in saved:
                m._require_gpu = fn
        got[f"{w} {code}: {name}"] = [type(exc.value).__name__, str(exc.value)]
    return got


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_abi_refusal_keeps_its_code_and_text(golden, w, code):
    got = abi_answers(w, code)
    assert len(got) >= 78 and sum(rc != 0 for rc, _ in got.values()) >= 70
    assert got == golden["abi"][f"{w} {code}"]


@pytest.mark.parametrize("code", CODES)
@pytest.mark.parametrize("w", WIDTHS)
def test_every_python_refusal_keeps_its_type_and_text(golden, w, code):
    got = python_answers(w, code, [importlib.import_module("colpali_amd._fp4_family")])
    assert len(got) >= 55
    assert got == golden["python"][f"{w} {code}"]
