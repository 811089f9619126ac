"""Sign tier: every MaxSim kernel on inputs whose similarities are ALL NEGATIVE, through the C ABI.

Contract (include/maxsim.h):
    scores[q, c] = sum over the tokens i of query q of max over the rows j of document c of <Q_i, D_j>      (fp32 accumulate)
    d_clamp0[c] = 1: a similarity of exactly 0 (the reference's zero padding row) also takes part in every per-token max of c
    a document without rows is a max over nothing: -inf, and 0 when it is flagged
    msim_pairs_argmax / msim_allpairs_argmax / msim_fwd_transposed_route also report the row that attains each max (the first one
    on a tie; -1 when the zero padding row wins)
    msim_i8_scores: the same structure on int8 codes, bit for bit as tests/int8_truth.py restates it

Every forward kernel reads the rows past a document's end as zeros (or leaves stale rows in its LDS ring) and masks them to -inf
after the MFMA; every launch form has its own copy of that mask.  A broken mask lets a ZERO into a max, and that changes a score
only where the true per-token maximum is negative.  Unit-normalised Gaussian rows, which every other GPU test draws, have a positive
maximum over any document of more than about ten rows: max(true, 0) == true and a leaked zero is invisible bit for bit.  Here the
queries sit at +0.7 u and the document rows at -0.7 u (tests/helpers.py: far_side_case), so every similarity is negative.

PRECONDITION, asserted by every test on its own float64 truth before the kernel's output is looked at: every per-token maximum over
every scored document is <= -0.05 (all-negative corpus).  One leaked zero then moves a score by at least 0.05; the score tolerance
is 1e-5 * max(|truth|, 1), at most about 4e-4 at these magnitudes.  The planted-winner corpus replaces one row per document by a row
on the queries' side (similarity about +0.49) at row 0, the last row, the first row of the last slab or next to a slab / chunk
boundary: a mask that removes one valid row moves a score by about 0.7 per token.

For every launch form: (1) truth on both corpora, (2) clamp0 on a random half of the documents -- a flagged all-negative document
scores exactly 0, an unflagged one keeps its bits, on the planted corpus no bit changes --, (3) a permuted corpus gives the permuted
scores bit for bit, (4) the routing, where the kernel reports one, (5) documents without rows.

Tolerances are the project's: scores 1e-5 * max(|truth|, 1) (test_gpu_parity.py), literal tier one bf16 ulp, int8 bit for bit
(test_gpu_int8.py).  The truth is float64 einsum -> max -> sum (tests/helpers.py: maxsim_truth), computed on the GPU by torch.
"""
import numpy as np
import pytest
import torch

from oracle import li_loss_oracle as lo
from oracle import maxsim_oracle as mo
from tests import int8_truth as it
from tests.helpers import SIGN_EDGE_LENS, SIGN_MARGIN, far_side_case, far_side_doc_lens, maxsim_truth, token_sums

pytestmark = pytest.mark.gpu

RTOL = 1e-5
DEV = torch.device("cuda:0")
REF_ROUNDING = 0x1
DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()      # must load: no fallback
    return colpali_amd


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _close(got, want, what=""):
    """finite entries within RTOL * max(|truth|, 1), the others (-inf: documents without rows) equal; prints the figure first"""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin]), f"{what}: documents without rows"
    err = float(((got[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1.0)).max()) if bool(fin.any()) else 0.0
    print(f"    {what}: largest error {err:.3e} (tolerance {RTOL:.0e})")
    assert err <= RTOL, (what, err)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


def _width(amd, dim, dtype):
    return amd._lib.kernel_width(dim, dtype)


def _corpus(amd, ps):
    """the packed blob and device offsets of a list of documents (rows widened to the kernels' width with zero columns)"""
    c = amd.pack_passages(ps, DEV, batch_size=None)
    return c.blob, c.offsets


def _clamp_dev(clamp):
    return None if clamp is None else torch.from_numpy(np.ascontiguousarray(clamp, dtype=np.uint8)).to(DEV)


def _q_offsets(qs):
    off = np.zeros(len(qs) + 1, dtype=np.int32)
    np.cumsum([q.shape[0] for q in qs], out=off[1:])
    return off


def _box(amd, qs, dtype, dim):
    """queries of ONE length as a [n_q, Lq, width] device box"""
    assert len({q.shape[0] for q in qs}) == 1
    box = torch.stack(qs)
    w = _width(amd, dim, dtype)
    if w != dim:
        box = torch.nn.functional.pad(box, (0, w - dim))
    return box.contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------------------ the entries, as a C caller
def run_ragged(amd, qs, ps, clamp, dim, dtype, avg_rows=0, flags=0):
    L = amd._lib.lib()
    blob, d_off = _corpus(amd, ps)
    tokens = torch.cat(qs).contiguous().to(DEV)
    off_h = _q_offsets(qs)
    off_d = torch.from_numpy(off_h).to(DEV)
    cl = _clamp_dev(clamp)
    n_q, n_d = len(qs), len(ps)
    code = amd._lib.dtype_code(dtype)
    nbytes = int(L.msim_fwd_ragged_workspace_bytes(code, off_h.ctypes.data, n_q, n_d, dim))
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV) if nbytes else None
    out = torch.full((n_q, n_d), 7.0, dtype=torch.float32, device=DEV)
    rc = L.msim_fwd_ragged(code, tokens.data_ptr(), off_d.data_ptr(), off_h.ctypes.data, n_q, blob.data_ptr(), d_off.data_ptr(),
                           amd._lib.ptr(cl), n_d, dim, out.data_ptr(), n_d, flags | (min(65535, avg_rows) << 8), amd._lib.ptr(ws), _stream())
    amd._lib.check(rc, "msim_fwd_ragged")
    torch.cuda.synchronize()
    return out.cpu(), None


def run_box(amd, qs, ps, clamp, dim, dtype, avg_rows=0, flags=0, scratch=True):
    L = amd._lib.lib()
    blob, d_off = _corpus(amd, ps)
    box = _box(amd, qs, dtype, dim)
    cl = _clamp_dev(clamp)
    n_q, lq, w = box.shape
    n_d = len(ps)
    code = amd._lib.dtype_code(dtype)
    nbytes = int(L.msim_fwd_workspace_bytes(code, n_q, lq, n_d, w)) if scratch else 0
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=DEV) if nbytes else None
    out = torch.full((n_q, n_d), 7.0, dtype=torch.float32, device=DEV)
    rc = L.msim_fwd(code, box.data_ptr(), n_q, lq, blob.data_ptr(), d_off.data_ptr(), amd._lib.ptr(cl), n_d, w, out.data_ptr(), n_d,
                    flags | (min(65535, avg_rows) << 8), amd._lib.ptr(ws), _stream())
    amd._lib.check(rc, "msim_fwd")
    torch.cuda.synchronize()
    return out.cpu(), None


def run_box_generic(amd, qs, ps, clamp, dim, dtype, **kw):
    return run_box(amd, qs, ps, clamp, dim, dtype, scratch=False, **kw)


def _listed(q, n_q, ident, lists):
    """does query q list the document whose identity is `ident`: every query lists every document ("shared": a document is read once
    per group of queries), or the queries split the documents among themselves ("disjoint": no document is listed twice)"""
    return True if lists == "shared" else ident % n_q == q


def run_candidates(amd, qs, ps, clamp, dim, dtype, lists="shared", ident=None):
    """msim_fwd_candidates (width 128) / msim_fwd_candidates_wide (width 320) as a [n_q, n_d] matrix: entry (q, c) is NaN where query q
    does not list document c.  `ident[c]` names the document at position c, so that a permuted corpus keeps every query's list."""
    L = amd._lib.lib()
    blob, d_off = _corpus(amd, ps)
    tokens = torch.cat(qs).contiguous().to(DEV)
    off_h = _q_offsets(qs)
    off_d = torch.from_numpy(off_h).to(DEV)
    cl = _clamp_dev(clamp)
    n_q, n_d = len(qs), len(ps)
    ident = list(range(n_d)) if ident is None else ident
    id_base = 1000
    g = torch.Generator().manual_seed(5)
    rows = []
    for q in range(n_q):
        mine = [c for c in range(n_d) if _listed(q, n_q, ident[c], lists)]
        mine = [mine[i] for i in torch.randperm(len(mine), generator=g).tolist()]       # every query in an order of its own
        rows.append(mine)
    m = max(len(r) for r in rows)
    cand = torch.full((n_q, m), -1, dtype=torch.int64)
    for q, r in enumerate(rows):
        cand[q, : len(r)] = torch.tensor(r, dtype=torch.int64) + id_base
    cand_d = cand.to(DEV)
    code = amd._lib.dtype_code(dtype)
    wide = dim != 128
    nbytes = int(L.msim_fwd_candidates_wide_workspace_bytes(n_q, m, n_d, dim) if wide else L.msim_fwd_candidates_workspace_bytes(n_q, m, n_d))
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=DEV)
    out = torch.full((n_q, m), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((n_q, m), -7, dtype=torch.int64, device=DEV)
    entry = L.msim_fwd_candidates_wide if wide else L.msim_fwd_candidates
    rc = entry(code, tokens.data_ptr(), off_d.data_ptr(), off_h.ctypes.data, n_q, blob.data_ptr(), d_off.data_ptr(), amd._lib.ptr(cl), n_d,
               dim, cand_d.data_ptr(), m, m, id_base, out.data_ptr(), m, ids.data_ptr(), 0, ws.data_ptr(), _stream())
    amd._lib.check(rc, entry.__name__)
    torch.cuda.synchronize()
    assert int(ws[:4].view(torch.int32)[0]) == 0, "a broken invariant was reported in the workspace"
    assert torch.equal(ids.cpu(), cand)
    full = torch.full((n_q, n_d), float("nan"), dtype=torch.float32)
    got = out.cpu()
    for q, r in enumerate(rows):
        full[q, r] = got[q, : len(r)]
        assert bool(torch.isneginf(got[q, len(r):]).all())                              # the empty entries of a shorter list
    return full, None


def run_pairs(amd, qs, ps, clamp, dim, dtype, max_doc_rows=0):
    """msim_pairs_argmax on the row-major list of all pairs: (scores [n_q, n_d], routing [n_q, n_d, Lq])"""
    L = amd._lib.lib()
    blob, d_off = _corpus(amd, ps)
    box = _box(amd, qs, dtype, dim)
    cl = _clamp_dev(clamp)
    n_q, lq, w = box.shape
    n_d = len(ps)
    pairs = torch.stack(torch.meshgrid(torch.arange(n_q), torch.arange(n_d), indexing="ij"), dim=-1).reshape(-1, 2).to(torch.int32).to(DEV)
    out = torch.full((n_q * n_d,), 7.0, dtype=torch.float32, device=DEV)
    am = torch.full((n_q * n_d, lq), -7, dtype=torch.int32, device=DEV)
    rc = L.msim_pairs_argmax(amd._lib.dtype_code(dtype), box.data_ptr(), n_q, lq, blob.data_ptr(), d_off.data_ptr(), amd._lib.ptr(cl), n_d, w,
                             max_doc_rows, pairs.data_ptr(), n_q * n_d, out.data_ptr(), am.data_ptr(), _stream())
    amd._lib.check(rc, "msim_pairs_argmax")
    torch.cuda.synchronize()
    return out.cpu().view(n_q, n_d), am.cpu().view(n_q, n_d, lq)


def run_pairs_transposed(amd, qs, ps, clamp, dim, dtype):
    return run_pairs(amd, qs, ps, clamp, dim, dtype, max_doc_rows=max(p.shape[0] for p in ps))


def run_allpairs(amd, qs, ps, clamp, dim, dtype):
    L = amd._lib.lib()
    blob, d_off = _corpus(amd, ps)
    box = _box(amd, qs, dtype, dim)
    cl = _clamp_dev(clamp)
    n_q, lq, w = box.shape
    n_d = len(ps)
    out = torch.full((n_q, n_d), 7.0, dtype=torch.float32, device=DEV)
    am = torch.full((n_q * n_d, lq), -7, dtype=torch.int32, device=DEV)
    rc = L.msim_allpairs_argmax(amd._lib.dtype_code(dtype), box.data_ptr(), n_q, lq, blob.data_ptr(), d_off.data_ptr(), amd._lib.ptr(cl), n_d, w,
                                out.data_ptr(), n_d, am.data_ptr(), _stream())
    amd._lib.check(rc, "msim_allpairs_argmax")
    torch.cuda.synchronize()
    return out.cpu(), am.cpu().view(n_q, n_d, lq)


# ------------------------------------------------------------------------------------------------------------ the five assertions
def _flags_for(d_lens, g):
    """clamp0 on a random half of the documents; of the documents without rows at least one is flagged and one is not"""
    flags = (torch.rand(len(d_lens), generator=g) < 0.5).numpy().astype(np.uint8)
    empties = [i for i, n in enumerate(d_lens) if n == 0]
    if len(empties) >= 2:
        flags[empties[0]], flags[empties[1]] = 1, 0
    return flags


def _same_bits(a, b, what):
    """bit equality where both entries were computed (NaN marks an entry a candidate list does not hold)"""
    both = ~(torch.isnan(a) | torch.isnan(b))
    assert bool(both.any())
    assert np.array_equal(_bits(a)[both.numpy()], _bits(b)[both.numpy()]), what


def check_form(amd, run, q_lens, dim, dtype, seed, d_lens=None, max_len=None, n_empty=4, literal=False, hints=False, bit_ref=None, **kw):
    """assertions 1-5 of the module docstring for one launch form.  run(amd, qs, ps, clamp, dim, dtype, **kw) -> (scores [n_q, n_d] on
    the CPU, routing [n_q, n_d, Lq] or None); NaN marks an entry the form does not compute (candidate lists)."""
    g = torch.Generator().manual_seed(seed)
    d_lens = far_side_doc_lens(g, n_empty=n_empty, max_len=max_len) if d_lens is None else d_lens
    n_d = len(d_lens)
    flags = _flags_for(d_lens, g)
    f = torch.from_numpy(flags).bool()
    perm = torch.randperm(n_d, generator=g).tolist()
    empty = torch.tensor([n == 0 for n in d_lens])
    off = np.concatenate([[0], np.cumsum(d_lens)])
    ident = {"ident": perm} if "lists" in kw else {}
    for planted in (False, True):
        tag = "planted" if planted else "all-negative"
        qs, ps, rows = far_side_case(seed * 2 + planted, q_lens, d_lens, dim, dtype, planted=planted)
        M, A, G = maxsim_truth(torch.cat(qs), torch.cat(ps), off, device=DEV)
        live = M[:, ~empty]
        if planted:        # the planted row wins every token's max, well above 0
            assert float(live.min()) >= SIGN_MARGIN, float(live.min())
            assert torch.equal(A[:, ~empty], torch.tensor(rows)[~empty].expand(M.shape[0], -1))
        else:              # PRECONDITION on the inputs alone
            assert float(live.max()) <= -SIGN_MARGIN, float(live.max())
        print(f"  {tag}: per-token maxima in [{float(live.min()):+.3f}, {float(live.max()):+.3f}], std {float(live.std()):.4f}")
        # 1. truth (5. documents without rows score -inf: _close compares them exactly)
        base, route = run(amd, qs, ps, None, dim, dtype, **kw)
        mask = ~torch.isnan(base)
        want = token_sums(M, q_lens)
        _close(base[mask], want[mask], f"{tag}, no flags")
        # 2. clamp0 on a random half
        clamped, route_c = run(amd, qs, ps, flags, dim, dtype, **kw)
        want_c = token_sums(M, q_lens, flags)
        _close(clamped[mask], want_c[mask], f"{tag}, clamp0")
        _same_bits(clamped[:, ~f], base[:, ~f], f"{tag}: an unflagged document keeps its bits")
        if bool((f & empty).any()):
            col = clamped[:, f & empty]
            assert bool((col[~torch.isnan(col)] == 0).all()), f"{tag}: a flagged document without rows scores 0"
        if planted:
            _same_bits(clamped[:, ~empty], base[:, ~empty], "planted: the flags change no bit")
        else:
            col = clamped[:, f]
            assert bool((col[~torch.isnan(col)] == 0).all()), "all-negative: a flagged document scores exactly 0"
        # 3. placement
        moved, _ = run(amd, qs, [ps[i] for i in perm], None, dim, dtype, **kw, **ident)
        _same_bits(moved, base[:, perm], f"{tag}: a permuted corpus gives the permuted scores")
        # 4. routing
        if route is not None:
            lq = q_lens[0]
            At = A.view(len(q_lens), lq, n_d).permute(0, 2, 1)
            Gt = G.view(len(q_lens), lq, n_d).permute(0, 2, 1)
            sure = (Gt > 1e-6) & ~empty.view(1, -1, 1)
            assert torch.equal(route.long()[sure], At[sure]), f"{tag}: routing = float64 arg-max"
            if planted:
                want_r = torch.tensor(rows).view(1, -1, 1).expand_as(At)
                ne = (~empty).view(1, -1, 1).expand_as(At)
                assert torch.equal(route.long()[ne], want_r[ne]) and torch.equal(route_c.long()[ne], want_r[ne]), "the planted row"
            else:
                hit = (f & ~empty).view(1, -1, 1).expand_as(At)
                assert bool((route_c[hit] == -1).all()), "the zero padding row wins every token of a flagged all-negative document"
                keep = sure & (~f).view(1, -1, 1)
                assert torch.equal(route_c.long()[keep], At[keep])
        # a launch-shape hint is never a result (test_gpu_short_docs.py::_both)
        if hints:
            for avg in (32, 4096):
                hinted, _ = run(amd, qs, ps, flags, dim, dtype, avg_rows=avg, **kw)
                _same_bits(hinted, clamped, f"{tag}: MSIM_FLAG_AVG_ROWS({avg})")
        # the scan another entry promises the same bits of (include/maxsim.h: msim_fwd_candidates*)
        if bit_ref is not None:
            ref, _ = bit_ref(amd, qs, ps, flags, dim, dtype)
            _same_bits(clamped, ref, f"{tag}: the bits of {bit_ref.__name__}")
        # literal tier: every similarity rounded to bf16 before the max, the token sum rounded once -- within one bf16 ulp of the oracle
        if literal and not planted:
            lit, _ = run(amd, qs, ps, None, dim, dtype, flags=REF_ROUNDING, **kw)
            ne = (~empty).numpy()
            ref = mo.score_multi_vector([q.float().numpy() for q in qs], [p.float().numpy() for p in ps if p.shape[0]], batch_size=1, mode="bf16ref")
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 1e-30))) - 7)
            d = np.abs(lit.numpy()[:, ne] - ref)
            print(f"    literal tier: largest distance {float((d / ulp).max()):.2f} ulp")
            assert np.all(d <= ulp)
            assert bool(torch.isneginf(lit[:, empty]).all())


def _plan(amd, q_lens=None, n_q=0, lq=0):
    L = amd._lib.lib()
    out = np.zeros(5, dtype=np.int32)
    if q_lens is not None:
        off = np.zeros(len(q_lens) + 1, dtype=np.int32)
        np.cumsum(q_lens, out=off[1:])
        rc = L.msim_fwd_plan(off.ctypes.data, len(q_lens), 0, out.ctypes.data)
    else:
        rc = L.msim_fwd_plan(None, n_q, lq, out.ctypes.data)
    assert rc == 0
    return tuple(int(x) for x in out)


def _ragged_lens(n, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, n).tolist()


# ------------------------------------------------------------------------------------------------------------ K1s and K1b (width 128)
# (id, entry, query lengths, the first three numbers msim_fwd_plan must report: kernel, units per wave | waves, units a wave holds)
TUNED = [
    ("K1s-1q-ragged", run_ragged, [19], (0, 2, 0)),
    ("K1s-4q-ragged", run_ragged, [20, 31, 17, 29], (0, 7, 0)),
    ("K1s-8q-ragged", run_ragged, [9, 16, 12, 15, 7, 16, 11, 13], (0, 7, 0)),
    ("K1s-1q-box", run_box, [32], (0, 2, 0)),
    ("K1s-4q-box", run_box, [32] * 4, (0, 8, 0)),
    ("K1s-8q-box", run_box, [12] * 8, (0, 6, 0)),
    ("K1b-pair", run_ragged, [29, 32, 18, 31, 32, 25, 30, 32], (1, 2, 8)),
    ("K1b-4x5", run_ragged, [30, 32, 28, 32, 31, 32, 29, 32, 32, 25], (1, 4, 5)),
    ("K1b-4x8", run_ragged, _ragged_lens(16, 17, 32, 1), (1, 4, 8)),
    ("K1b-4x10", run_ragged, [32] * 18 + [30, 31], (1, 4, 10)),
    ("K1b-8x8", run_ragged, _ragged_lens(32, 17, 32, 2), (1, 8, 8)),
    ("K1b-8x10", run_ragged, [32] * 36 + [29, 31, 30, 32], (1, 8, 10)),
    ("K1b-pair-box", run_box, [32] * 8, (1, 2, 8)),
    ("K1b-8x10-box", run_box, [32] * 40, (1, 8, 10)),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name,run,q_lens,shape", TUNED, ids=[t[0] for t in TUNED])
def test_stream_and_single_block_batch_kernels(amd, name, run, q_lens, shape, dt):
    plan = _plan(amd, q_lens) if run is run_ragged else _plan(amd, n_q=len(q_lens), lq=q_lens[0])
    assert plan[:3] == shape and plan[3] == 1, (name, plan)          # the case cannot quietly land on another kernel
    check_form(amd, run, q_lens, 128, DT[dt], 100 + len(q_lens) + sum(q_lens), literal=dt == "bf16", hints=shape[0] == 1)


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n_q", [77, 1000])
def test_multi_block_batch_kernel_under_both_length_hints(amd, n_q, dt):
    q_lens = _ragged_lens(n_q, 17, 32, 3) if n_q == 77 else _ragged_lens(n_q, 12, 48, 4)
    plan = _plan(amd, q_lens)
    assert plan[0] == 1 and plan[1] == 8 and plan[3] > 1, plan           # K1b, eight waves, several query blocks (convoy counters in the scratch)
    check_form(amd, run_ragged, q_lens, 128, DT[dt], 200 + n_q, hints=True)


# ------------------------------------------------------------------------------------------------------------ panel kernels (width 320)
# which kernel takes which call: maxsim_abi.hip (msim_fwd_ragged: a uniform call of <= 4 token tiles in all -> K1sP, everything else
# -> K1bPF; msim_fwd: <= 4 tiles in all -> K1sP, whole queries of 32 / 64 rows -> K1bP, every other box -> K1bPF)
WIDE = [
    ("K1sP-flat-4x32", run_ragged, [32] * 4),
    ("K1sP-flat-2x20", run_ragged, [20] * 2),
    ("K1bPF-flat-ragged", run_ragged, [33, 47, 12, 40, 21, 38, 9, 27, 44]),
    ("K1bPF-flat-two-blocks", run_ragged, [31] * 30),
    ("K1sP-box-2x64", run_box, [64] * 2),
    ("K1sP-box-1x128", run_box, [128]),
    ("K1bP-box-13x32", run_box, [32] * 13),
    ("K1bP-box-17x64", run_box, [64] * 17),
    ("K1bPF-box-9x40", run_box, [40] * 9),
]


@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("name,run,q_lens", WIDE, ids=[t[0] for t in WIDE])
def test_panel_kernels_at_width_320(amd, name, run, q_lens, dt):
    check_form(amd, run, q_lens, 320, DT[dt], 300 + len(q_lens) + sum(q_lens), literal=dt == "bf16" and len(q_lens) <= 13)


# ------------------------------------------------------------------------------------------------------------ the generic kernel K1g
GENERIC = [
    ("K1g-fp32-d32", "fp32", 32, [7] * 5),
    ("K1g-fp32-d128", "fp32", 128, [32] * 3),
    ("K1g-fp32-d320", "fp32", 320, [40] * 4),
    ("K1g-fp32-d1024", "fp32", 1024, [33] * 2),
    ("K1g-bf16-d100-padded-to-112", "bf16", 100, [20] * 4),
    ("K1g-fp32-d128-200-tokens-sub-passes", "fp32", 128, [200] * 2),
    ("K1g-bf16-d128-160-tokens-without-scratch", "bf16", 128, [160] * 3),
]


@pytest.mark.parametrize("name,dt,dim,q_lens", GENERIC, ids=[t[0] for t in GENERIC])
def test_generic_kernel(amd, name, dt, dim, q_lens):
    check_form(amd, run_box_generic, q_lens, dim, DT[dt], 400 + dim + q_lens[0])


# ------------------------------------------------------------------------------------------------------------ candidate lists
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("lists", ["shared", "disjoint"])
@pytest.mark.parametrize("dim", [128, 320], ids=["K1c", "K1cP"])
def test_candidate_kernels(amd, dim, lists, dt):
    q_lens = [1, 15, 16, 17, 31, 32, 33, 127, 128, 5, 40, 9]              # mixed lengths: the scan of the same call runs K1b / K1bPF
    check_form(amd, run_candidates, q_lens, dim, DT[dt], 500 + dim, lists=lists, bit_ref=run_ragged)


# ------------------------------------------------------------------------------------------------------------ arg-max kernels
ARGMAX = [
    ("pairs-128-workgroup-per-pair", run_pairs, "bf16", 128, [32] * 8, None),          # <= 1024 pairs
    ("pairs-128-wave-per-pair", run_pairs, "fp16", 128, [20] * 32, None),              # > 1024 pairs
    ("pairs-128-four-tiles", run_pairs, "bf16", 128, [128] * 3, None),
    ("pairs-generic-fp32-d128", run_pairs, "fp32", 128, [32] * 4, None),
    ("pairs-generic-bf16-d320", run_pairs, "bf16", 320, [40] * 4, None),
    ("pairs-generic-bf16-d128-200-tokens", run_pairs, "bf16", 128, [200] * 2, None),
    ("pairs-transposed-200-tokens", run_pairs_transposed, "bf16", 128, [200] * 3, 128),
    ("allpairs-128-one-tile", run_allpairs, "bf16", 128, [32] * 9, None),
    ("allpairs-128-two-tiles", run_allpairs, "fp16", 128, [40] * 5, None),
    ("allpairs-128-four-tiles", run_allpairs, "bf16", 128, [128] * 3, None),
]


@pytest.mark.parametrize("name,run,dt,dim,q_lens,max_len", ARGMAX, ids=[t[0] for t in ARGMAX])
def test_argmax_kernels_scores_and_routing(amd, name, run, dt, dim, q_lens, max_len):
    check_form(amd, run, q_lens, dim, DT[dt], 600 + dim + len(q_lens) + q_lens[0], max_len=max_len)


# ------------------------------------------------------------------------------------------------------------ K1t: the transposed shape
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("ld", [1, 17, 33, 50, 64, 100, 128])
def test_transposed_kernel_scores_and_routing(amd, ld, dt):
    """msim_fwd_transposed / msim_fwd_transposed_route: two dense boxes, the long side (333 rows: not a multiple of the 64-row routing
    pad nor of a 128-row chunk) streams, documents of ld rows are resident; the resident rows past ld are the kernel's to mask.  No
    clamp0 and no ragged documents in this entry: truth, placement and routing."""
    L = amd._lib.lib()
    dtype = DT[dt]
    n_q, lq, n_d = 5, 333, 37
    g = torch.Generator().manual_seed(700 + ld)
    perm = torch.randperm(n_d, generator=g).tolist()
    code = amd._lib.dtype_code(dtype)
    off = np.arange(n_d + 1) * ld
    with_route = bool(L.msim_dense_t_supported(code, n_q, lq, n_d, ld, 128))
    assert with_route == (ld <= 64)

    def run(qs, ps, route):
        Q, D = torch.stack(qs).contiguous().to(DEV), torch.stack(ps).contiguous().to(DEV)
        out = torch.full((n_q, n_d), 7.0, dtype=torch.float32, device=DEV)
        lens = torch.full((n_q,), -1, dtype=torch.int32, device=DEV)
        r = None
        if route:
            r = torch.full((int(L.msim_dense_t_route_bytes(n_q, lq, n_d)),), 255, dtype=torch.uint8, device=DEV)
            rc = L.msim_fwd_transposed_route(code, Q.data_ptr(), n_q, lq, D.data_ptr(), n_d, ld, 128, out.data_ptr(), n_d, lens.data_ptr(),
                                             r.data_ptr(), _stream())
        else:
            rc = L.msim_fwd_transposed(code, Q.data_ptr(), n_q, lq, D.data_ptr(), n_d, ld, 128, out.data_ptr(), n_d, lens.data_ptr(), _stream())
        amd._lib.check(rc, "msim_fwd_transposed")
        torch.cuda.synchronize()
        assert torch.equal(lens.cpu().long(), (Q[:, :, 0] != 0).sum(dim=1).cpu())     # the by-product: rows whose first component is non-zero
        return out.cpu(), (r.cpu().view(n_q, n_d, -1)[:, :, :lq] if route else None)

    for planted in (False, True):
        tag = "planted" if planted else "all-negative"
        qs, ps, rows = far_side_case(1400 + 2 * ld + planted, [lq] * n_q, [ld] * n_d, 128, dtype, planted=planted)
        M, A, G = maxsim_truth(torch.cat(qs), torch.cat(ps), off, device=DEV)
        if planted:
            assert float(M.min()) >= SIGN_MARGIN
        else:
            assert float(M.max()) <= -SIGN_MARGIN, float(M.max())
        want = token_sums(M, [lq] * n_q)
        base, _ = run(qs, ps, False)
        _close(base, want, f"{tag}, msim_fwd_transposed")
        moved, _ = run(qs, [ps[i] for i in perm], False)
        assert np.array_equal(_bits(moved), _bits(base[:, perm]))
        if with_route:
            routed, route = run(qs, ps, True)
            assert np.array_equal(_bits(routed), _bits(base))         # bit-identical scores (include/maxsim.h)
            At = A.view(n_q, lq, n_d).permute(0, 2, 1)
            Gt = G.view(n_q, lq, n_d).permute(0, 2, 1)
            sure = Gt > 1e-6
            assert torch.equal(route.long()[sure], At[sure]), f"{tag}: routing = float64 arg-max"
            if planted:
                assert torch.equal(route.long(), torch.tensor(rows).view(1, -1, 1).expand_as(At))


# ------------------------------------------------------------------------------------------------------------ the int8 scorer
@pytest.mark.parametrize("dt", ["bf16", "fp16"])
@pytest.mark.parametrize("n_q", [3, 70])
def test_int8_scorer_on_far_side_pages(amd, n_q, dt):
    """msim_i8_scores against tests/int8_truth.py, bit for bit as in test_gpu_int8.py: 16-row chunks that straddle page boundaries
    (pages of 1 .. 5 rows between the long ones), every tail class, pages without rows, clamp0.  The integer maxima are all negative
    (asserted on the truth), so a zero row that reaches a max changes the score."""
    L = amd._lib.lib()
    dtype = DT[dt]
    g = torch.Generator().manual_seed(800 + n_q)
    d_lens = far_side_doc_lens(g, lens=SIGN_EDGE_LENS + [2, 3, 5, 2, 1, 3], copies=2, n_empty=4)
    n_d = len(d_lens)
    q_lens = ([1, 16, 17, 32, 33, 64, 5, 40] * 9)[:n_q]
    flags = _flags_for(d_lens, g)
    f = torch.from_numpy(flags).bool()
    perm = torch.randperm(n_d, generator=g).tolist()
    empty = torch.tensor([n == 0 for n in d_lens])
    code = amd._lib.dtype_code(dtype)

    def run(qs, ps, clamp):
        blob, d_off = _corpus(amd, ps)
        rows = int(blob.shape[0])
        d8 = torch.empty((rows, 128), dtype=torch.int8, device=DEV)
        sd = torch.empty((len(ps),), dtype=torch.float32, device=DEV)
        amd._lib.check(L.msim_i8_encode_docs(code, blob.data_ptr(), d_off.data_ptr(), len(ps), rows, 128, d8.data_ptr(), sd.data_ptr(), _stream()),
                       "msim_i8_encode_docs")
        tokens = torch.cat(qs).contiguous().to(DEV)
        t = int(tokens.shape[0])
        q8 = torch.empty((t, 128), dtype=torch.int8, device=DEV)
        sq = torch.empty((t,), dtype=torch.float32, device=DEV)
        amd._lib.check(L.msim_i8_encode_queries(code, tokens.data_ptr(), t, 128, q8.data_ptr(), sq.data_ptr(), _stream()), "msim_i8_encode_queries")
        q_off = torch.from_numpy(_q_offsets(qs)).to(DEV)
        cl = _clamp_dev(clamp)
        out = torch.full((len(qs), len(ps)), 7.0, dtype=torch.float32, device=DEV)
        amd._lib.check(L.msim_i8_scores(q8.data_ptr(), sq.data_ptr(), q_off.data_ptr(), len(qs), t, max(q_lens), d8.data_ptr(), sd.data_ptr(),
                                        d_off.data_ptr(), amd._lib.ptr(cl), len(ps), rows, 128, out.data_ptr(), len(ps), _stream()), "msim_i8_scores")
        torch.cuda.synchronize()
        return out.cpu()

    off = np.concatenate([[0], np.cumsum(d_lens)])
    for planted in (False, True):
        qs, ps, _ = far_side_case(1600 + 2 * n_q + planted, q_lens, d_lens, 128, dtype, planted=planted)
        M, _, _ = maxsim_truth(torch.cat(qs), torch.cat(ps), off, device=DEV)
        q8, sq = it.quantize_tokens(torch.cat(qs).float().numpy())
        d8, sd = it.quantize_pages(torch.cat(ps).float().numpy(), off)
        Mi = it.maxima(q8, d8, off)[:, (~empty).numpy()]
        if planted:
            assert float(M[:, ~empty].min()) >= SIGN_MARGIN and int(Mi.min()) > 0
        else:              # PRECONDITION, in float64 and on the integer maxima the scorer really takes
            assert float(M[:, ~empty].max()) <= -SIGN_MARGIN and int(Mi.max()) < 0
        q_off = np.concatenate([[0], np.cumsum(q_lens)])
        base = run(qs, ps, None)
        assert np.array_equal(_bits(base), it.scores(q8, sq, q_off, d8, sd, off, None).view(np.int32))
        assert bool(torch.isneginf(base[:, empty]).all())
        clamped = run(qs, ps, flags)
        assert np.array_equal(_bits(clamped), it.scores(q8, sq, q_off, d8, sd, off, flags).view(np.int32))
        assert np.array_equal(_bits(clamped[:, ~f]), _bits(base[:, ~f]))
        if planted:
            assert np.array_equal(_bits(clamped[:, ~empty]), _bits(base[:, ~empty]))
        else:
            assert bool((clamped[:, f & ~empty] == 0).all())
        moved = run(qs, [ps[i] for i in perm], None)
        assert np.array_equal(_bits(moved), _bits(base[:, perm]))


# ------------------------------------------------------------------------------------------------------------ the training path, end to end
def _grad_tolerance(want, paths):
    """test_gpu_loss.py::grads_close, restated: per element |want| 2^-7 + 1e-6 for bf16 gradients; with `paths` > 1 that many times,
    plus paths * 2^-9 of the largest element"""
    want = want.float()
    tol = want.abs() * 2.0**-7 + 1e-6
    if paths > 1:
        tol = tol * paths + float(want.abs().max()) * 2.0**-9 * paths
    return tol


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("cls,kind", [("ColbertPairwiseCELoss", "pairwise"), ("ColbertLoss", "infonce")])
@pytest.mark.parametrize("planted", [False, True], ids=["all-negative", "planted"])
def test_losses_on_a_far_side_batch(amd, cls, kind, dt, planted):
    """ColbertPairwiseCELoss / ColbertLoss, forward and backward, in both trainer directions (queries against gathered pages: the
    all-pairs arg-max kernel; pages against gathered queries: K1t and its routing) against oracle/li_loss_oracle.py.  A leaked zero
    here is a wrong gradient: the routing would point at a row that does not exist.

    Tolerances are test_gpu_loss.py's, direction by direction: test_config5_full_shape_loss_and_grads for queries against pages
    (fp32: loss 1e-5, gradients 1e-4 |want| + 1e-6; bf16: loss 2^-8, grads_close with one path), and
    test_symmetric_loss_documents_in_the_query_slot for pages against queries, where ColbertLoss in bf16 runs its backward on
    msim_dense_t_bwd: the upstream gradient enters that kernel rounded to bf16 per term (include/maxsim.h; the reference's own [B, C]
    score gradient is a bf16 tensor too), which that test allows for with paths = 2 in grads_close.  On far-side rows the allowance
    is needed: the rows of a cross-entropy gradient sum to zero and every row carries the same 0.7 u component, so the terms of a
    gradient row cancel and the rounding of G (2^-9 of a term) is large against a small element.  Measured on an MI355X with ONE path
    in that direction: largest error 6.104e-05 (dQ) and 4.883e-04 (dD), one bf16 ulp of the largest element each, but 18.72 and 23.94
    times |want| 2^-7 + 1e-6 on small elements; a float64 evaluation on the CPU with nothing but G rounded to bf16 reproduces 6.104e-05
    and 18.72 exactly, and sits at 0.42 (dQ) and 0.35 (dD) of the two-path tolerance."""
    dtype = DT[dt]
    B, C, lq, ld, offset = 6, 20, 30, 150, 9
    qs, ps, _ = far_side_case(1800 + planted, [lq] * C, [ld] * C, 128, dtype, planted=planted)
    Qall, Dall = torch.stack(qs), torch.stack(ps)
    M, _, _ = maxsim_truth(Qall.view(-1, 128), Dall.view(-1, 128), np.arange(C + 1) * ld, device=DEV)
    if planted:
        assert float(M.min()) >= SIGN_MARGIN
    else:
        assert float(M.max()) <= -SIGN_MARGIN
    kw = dict(normalize_scores=False) if kind == "pairwise" else dict()
    for symmetric, (Qx, Dx) in enumerate(((Qall[offset:offset + B], Dall), (Dall[offset:offset + B], Qall))):
        want_loss, want_dq, want_dd = lo.loss_and_grads(kind, Qx.float(), Dx.float(), offset=offset, **kw)
        q, d = Qx.clone().to(DEV).requires_grad_(True), Dx.clone().to(DEV).requires_grad_(True)
        loss = getattr(amd, cls)(**kw)(query_embeddings=q, doc_embeddings=d, offset=offset)
        assert loss.dtype == dtype and loss.dim() == 0
        loss.backward()
        print(f"    loss {float(loss.detach()):.6f}, oracle {float(want_loss):.6f}")
        if dtype == torch.float32:
            assert abs(float(loss.detach()) - float(want_loss)) <= 1e-5 * abs(float(want_loss)) + 1e-6
            for got, want in ((q.grad, want_dq), (d.grad, want_dd)):
                assert int(((got.cpu().double() - want).abs() > 1e-4 * want.abs() + 1e-6).sum()) == 0
        else:
            assert abs(float(loss.detach()) - float(want_loss)) <= 2.0**-8 * abs(float(want_loss)) + 1e-6
            paths = 2 if symmetric and kind == "infonce" else 1     # msim_dense_t_bwd: see the docstring
            for got, want in ((q.grad, want_dq), (d.grad, want_dd)):
                e = (got.float().cpu() - want.float().to(torch.bfloat16).float()).abs()
                worst = float((e / _grad_tolerance(want, paths)).max())
                print(f"    gradient: largest error {float(e.max()):.3e}, largest |want| {float(want.abs().max()):.3e}, "
                      f"worst error / tolerance ({paths} path(s)) {worst:.2f}")
                assert worst <= 1.0
