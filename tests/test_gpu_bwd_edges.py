"""GPU: the hard-max backward (msim_pairs_bwd) at the capacity edges of its kernels.

The routing is SYNTHETIC: a hand-made int32 argmax [n_pairs, Lq] with values in [-1, len_c), so that entries land exactly on each
limit whatever a forward kernel would have produced; the corpus is packed and ragged (a few long documents among many of 1-8 rows).
Truth is the contract formula in float64 (tests/helpers.py: pairs_bwd_truth).  Every case asserts the launcher branch it claims
(a mirror of abi_train.hip's host-side choices, below) and checks:
  - outputs pre-filled with NaN come back finite everywhere; rows / tokens without entries come back exactly 0;
  - fp32 output within 2e-6 * max|truth|;
  - two runs bit-identical;
  - 16-bit output (out_dtype = dtype) == one rounding of the fp32 output.
"""
from __future__ import annotations

import functools

import pytest
import torch

from tests.helpers import pairs_bwd_truth

pytestmark = pytest.mark.gpu

# ---- the kernels' limits (maxsim_pairs.hip: kBwdRows; maxsim_bwd.hip: kRows*)
BWD_ROWS = 64
ROWS_MAX_ENT, ROWS_MAX_PAIRS, ROWS_MAX_ROWS, ROWS_COUNT_PAIRS = 4096, 1024, 1024, 16384
ESIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def cus():
    """The CU count the library plans with (it reads the same hipDeviceProp field)."""
    return torch.cuda.get_device_properties(torch.device("cuda", torch.cuda.current_device())).multi_processor_count


# ---- mirror of the launcher (colpali_amd/csrc/abi_train.hip: dd_plan, launch_bwd_kernels)
def dd_plan(n_pairs, Lq, n_d, dim, max_doc_rows, n_cus):
    """dd_plan (abi_train.hip: dd_plan) -> (mode, splits, scratch bytes); mode 0: no dense form."""
    if n_d <= 0 or n_pairs <= 0 or max_doc_rows <= 0 or max_doc_rows > BWD_ROWS or dim <= 0:
        return 0, 0, 0
    mode, splits, nbytes = 0, 0, 0
    entries_per_doc = n_pairs * Lq // n_d
    if entries_per_doc >= 1024:
        splits = min(_cdiv(4 * n_cus, n_d), entries_per_doc // 256, 64)
        mode, splits = 1, max(splits, 1)
        nbytes = splits * n_d * max_doc_rows * dim * 4
    elif Lq >= 256:
        mode, splits = 2, min(Lq // 64, 16)
        nbytes = splits * n_pairs * max_doc_rows * dim * 4
    if nbytes > 256 << 20:
        return 0, 0, 0
    return mode, splits, nbytes


def dd_form(n_q, Lq, n_d, n_pairs, dim, max_doc_rows, n_cus, workspace):
    """The dD kernel launch_bwd_kernels picks (abi_train.hip: launch_bwd_kernels, the dD half): ("dense", splits) / ("pairs", splits) for dd_plan modes 1 / 2
    (only with a workspace), ("rows", sy) for the row-list kernel, ("range", gy) for the row-range kernel."""
    if workspace:
        mode, splits, _ = dd_plan(n_pairs, Lq, n_d, dim, max_doc_rows, n_cus)
        if mode:
            return ("dense" if mode == 1 else "pairs"), splits
    pairs_per_doc = min(n_pairs, 2 * n_q)
    dense_enough = n_pairs * Lq >= 64 * n_d
    if dense_enough and pairs_per_doc <= ROWS_MAX_PAIRS and pairs_per_doc * Lq <= ROWS_MAX_ENT:
        sy = min(_cdiv(2 * n_cus, n_d), _cdiv(max_doc_rows, 64))
        need = _cdiv(max_doc_rows, ROWS_MAX_ROWS)
        return "rows", (need if sy < need else max(sy, 1))
    ry = _cdiv(max_doc_rows, BWD_ROWS)
    return "range", max(1, min(_cdiv(8 * n_cus, n_d), ry))


def dq_plan(n_q, Lq, n_pairs):
    """(tpw, psplit) of the dQ launch (abi_train.hip: launch_bwd_kernels, the dQ half)."""
    tokens = n_q * Lq
    tpw = min(max(_cdiv(tokens, 4096), 1), 16)
    psplit = tokens <= 2048 and n_pairs >= 64 * n_q
    return (1 if psplit else tpw), psplit


def dq_groups(dim, dtype):
    """G, the pairs (or tokens) a dQ wave works on per step (maxsim_bwd.hip:115-119)."""
    pieces = dim * ESIZE[dtype] // 16
    pp_log = 1
    while (1 << pp_log) < pieces and pp_log < 6:
        pp_log += 1
    return 64 >> pp_log


def few_pairs(pairs_of_query, G, psplit):
    """The dQ kernel's few-pairs branch (maxsim_bwd.hip:122): lane groups take tokens instead of pairs."""
    return not psplit and pairs_of_query <= 8 and G > 1


# ---- a synthetic problem
class Problem:
    """Ragged packed corpus, queries, a pair list sorted by query and a hand-made routing."""

    def __init__(self, lens, n_q, Lq, pair_list, seed, neg_frac=0.05, max_doc_rows=None, exact=False):
        self.exact = exact
        self.lens = [int(x) for x in lens]
        self.n_q, self.Lq, self.n_d = n_q, Lq, len(self.lens)
        self.max_doc_rows = max(self.lens) if max_doc_rows is None else max_doc_rows
        self.gen = torch.Generator().manual_seed(seed)
        pair_list = sorted(pair_list, key=lambda bc: bc[0])                # stable: sorted by query, as the ABI wants
        self.pairs = torch.tensor(pair_list, dtype=torch.int32).view(-1, 2)
        self.n_pairs = self.pairs.shape[0]
        self.order = torch.sort(self.pairs[:, 1].long(), stable=True).indices.to(torch.int32)
        self.off = torch.zeros(self.n_d + 1, dtype=torch.int32)
        self.off[1:] = torch.cumsum(torch.tensor(self.lens, dtype=torch.int64), 0)
        self.g = torch.randn(self.n_pairs, generator=self.gen)
        if exact:                                                       # multiples of 1/8 in [-2, 2] (see tensors())
            self.g = torch.randint(-16, 17, (self.n_pairs,), generator=self.gen).float() / 8
        # routing: uniform over the document's rows, a fraction -1; length-0 documents: all -1
        doc_len = torch.tensor(self.lens, dtype=torch.int64)[self.pairs[:, 1].long()] if self.n_pairs else torch.zeros(0, dtype=torch.int64)
        u = torch.rand(self.n_pairs, Lq, generator=self.gen, dtype=torch.float64)
        am = (u * doc_len.unsqueeze(1)).long()
        neg = torch.rand(self.n_pairs, Lq, generator=self.gen) < neg_frac
        am[neg | (doc_len.unsqueeze(1) == 0)] = -1
        self.argmax = am.to(torch.int32)

    def entries_of(self, c):
        """(pair, token) index tensors of document c's entries in list order (by-document pair order, then token)."""
        ps = self.order[self.pairs[self.order.long(), 1] == c].long()
        return ps.repeat_interleave(self.Lq), torch.arange(self.Lq).repeat(ps.numel())

    def plant(self, c, rows, fill=False):
        """Route document c's first len(rows) entries to `rows`; fill: route ALL its entries to `rows`, cycled."""
        p, i = self.entries_of(c)
        rows = torch.as_tensor(rows, dtype=torch.int32)
        n = p.numel() if fill else min(rows.numel(), p.numel())
        self.argmax[p[:n], i[:n]] = rows[torch.arange(n) % rows.numel()]

    def n_pd(self, c):
        return int((self.pairs[:, 1] == c).sum())

    def per(self, c, sy):
        """The row range of one row-list workgroup of document c (maxsim_bwd.hip:439)."""
        return _cdiv(self.lens[c], sy)

    def tensors(self, dtype, dim):
        gen = torch.Generator().manual_seed(int(torch.randint(0, 1 << 30, (1,), generator=self.gen)))
        if self.exact:
            # a list-order fp32 sum of 4096 random terms carries ~3e-6 relative rounding by itself; on this grid (k / 1024, |k| < 128,
            # exact in every dtype; g in 1/8 steps) every product and partial sum of up to 8192 terms is exact in fp32, so the bound
            # below measures the routing alone -- one entry lost, added twice or misrouted moves a value by >= 2^-13
            Q = (torch.randint(-127, 128, (self.n_q, self.Lq, dim), generator=gen).float() / 1024).to(dtype)
            D = (torch.randint(-127, 128, (int(self.off[-1]), dim), generator=gen).float() / 1024).to(dtype)
            return Q, D
        Q = torch.nn.functional.normalize(torch.randn(self.n_q, self.Lq, dim, generator=gen), dim=-1).to(dtype)
        D = torch.nn.functional.normalize(torch.randn(int(self.off[-1]), dim, generator=gen), dim=-1).to(dtype)
        return Q, D

    def form(self, dim, workspace=False):
        return dd_form(self.n_q, self.Lq, self.n_d, self.n_pairs, dim, self.max_doc_rows, cus(), workspace)


def _all_pairs(n_q, n_d, times=1):
    return [(b, c) for b in range(n_q) for c in range(n_d) for _ in range(times)]


def run_bwd(pb, Q, D, out_dtype, workspace=False):
    """One msim_pairs_bwd call; outputs pre-filled with NaN.  Returns (dQ, dD) on the host."""
    from colpali_amd import _lib

    lib = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    dim = Q.shape[-1]
    q, d = Q.to(dev), D.to(dev)
    off, pairs, order, g, am = (x.to(dev) for x in (pb.off, pb.pairs, pb.order, pb.g, pb.argmax))
    dq = torch.full((pb.n_q, pb.Lq, dim), float("nan"), dtype=out_dtype, device=dev)
    dd = torch.full((max(D.shape[0], 1), dim), float("nan"), dtype=out_dtype, device=dev)
    nbytes = lib.msim_pairs_bwd_workspace_bytes(pb.n_q, pb.Lq, pb.n_d, dim, pb.max_doc_rows, pb.n_pairs)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev) if workspace and nbytes else None
    code = _lib.dtype_code(Q.dtype)
    rc = lib.msim_pairs_bwd(code, _lib.ptr(q), pb.n_q, pb.Lq, _lib.ptr(d), _lib.ptr(off), pb.n_d, dim, pb.max_doc_rows, _lib.ptr(pairs),
                            _lib.ptr(order), _lib.ptr(g), None, 0, _lib.ptr(am), pb.n_pairs, 2 if out_dtype == torch.float32 else code,
                            _lib.ptr(dq), _lib.ptr(dd), _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_pairs_bwd")
    torch.cuda.synchronize(dev)
    return dq.cpu(), dd[: D.shape[0]].cpu()


def check_bwd(pb, dtype, dim, workspace=False):
    """The module's assertions (see the docstring) for one problem; returns the fp32 (dQ, dD)."""
    from colpali_amd import _lib

    lib = _lib.lib()
    mode, _, nbytes = dd_plan(pb.n_pairs, pb.Lq, pb.n_d, dim, pb.max_doc_rows, cus())
    assert lib.msim_pairs_bwd_workspace_bytes(pb.n_q, pb.Lq, pb.n_d, dim, pb.max_doc_rows, pb.n_pairs) == nbytes   # the mirror plans alike
    Q, D = pb.tensors(dtype, dim)
    want_dq, want_dd = pairs_bwd_truth(Q, D, pb.off, pb.pairs, pb.g, pb.argmax)
    first = run_bwd(pb, Q, D, torch.float32, workspace)
    second = run_bwd(pb, Q, D, torch.float32, workspace)
    # rows / tokens that receive an entry
    am, pr, off = pb.argmax.long(), pb.pairs.long(), pb.off.long()
    p, i = (am >= 0).nonzero(as_tuple=True)
    hit_d = torch.zeros(D.shape[0], dtype=torch.bool)
    hit_d[off[pr[p, 1]] + am[p, i]] = True
    hit_q = torch.zeros(pb.n_q * pb.Lq, dtype=torch.bool)
    hit_q[pr[p, 0] * pb.Lq + i] = True
    for name, got, again, want, hit in (("dQ", first[0], second[0], want_dq, hit_q.view(pb.n_q, pb.Lq)), ("dD", first[1], second[1], want_dd, hit_d)):
        assert torch.isfinite(got).all(), name
        assert torch.equal(got, again), f"{name}: two runs differ"
        assert bool((got[~hit] == 0).all()), f"{name}: a row without entries is not 0"
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        assert err <= 2e-6 * scale, f"{name}: max err {err:.3e} against max|truth| {scale:.3e}"
    if dtype != torch.float32:
        out16 = run_bwd(pb, Q, D, dtype, workspace)
        for name, got, ref in (("dQ", out16[0], first[0]), ("dD", out16[1], first[1])):
            assert got.dtype == dtype
            assert torch.equal(got, ref.to(dtype)), f"{name}: 16-bit output is not one rounding of the fp32 result"
    return first


DTYPE_WIDTH = [pytest.param(dt, w, id=f"{str(dt)[6:]}-{w}") for dt in (torch.bfloat16, torch.float16, torch.float32) for w in (128, 320)]


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _short_lens(gen, n):
    return torch.randint(1, 9, (n,), generator=gen).tolist()


# ---- row-list dD (maxsim_bwd_dd_rows_kernel)
def case_sy1(seed):
    """2 * CUs documents: sy = 1, so a document of 1024 rows is ONE workgroup's range of kRowsMaxRows rows; 1023 beside it."""
    n_d = 2 * cus()
    lens = _short_lens(torch.Generator().manual_seed(seed), n_d)
    lens[0], lens[1], lens[n_d // 2] = 1024, 1023, 1024
    pb = Problem(lens, 4, 32, _all_pairs(4, n_d), seed)
    for c in (0, 1, n_d // 2):
        pb.plant(c, [0, lens[c] - 1, lens[c] - 1, 0, lens[c] - 2])
    form, sy = pb.form(128)
    assert (form, sy) == ("rows", 1)
    assert pb.per(0, sy) == 1024 and pb.per(1, sy) == 1023 and pb.per(n_d // 2, sy) == 1024
    return pb


def case_sy2(seed):
    """CUs documents with 2048 / 2047 / 2046 rows: sy = 2 -- ranges of 1024 + 1024, 1024 + 1023, 1023 + 1023 rows."""
    n_d = cus()
    lens = _short_lens(torch.Generator().manual_seed(seed), n_d)
    lens[0], lens[1], lens[2] = 2048, 2047, 2046
    pb = Problem(lens, 4, 32, _all_pairs(4, n_d), seed)
    form, sy = pb.form(128)
    assert (form, sy) == ("rows", 2)
    assert pb.per(0, sy) == 1024 and pb.per(1, sy) == 1024 and pb.per(2, sy) == 1023
    for c in (0, 1, 2):
        per = pb.per(c, sy)
        pb.plant(c, [0, per - 1, per, lens[c] - 1, per - 1, per, 0, lens[c] - 1])   # row 0, the last of each range, the first of the second
    return pb


def case_ent4096(seed, Lq=64):
    """Every document paired with each of 32 queries twice: n_pd = 64, n_ent = 64 * Lq -- 4096 = kRowsMaxEnt exactly at Lq = 64 (the host
    bound 2 * n_q * Lq = 4096); at Lq = 65 the bound is 4160 and the host routes the list to the row-range kernel.  Document 5 has ALL its
    entries on one row (the in-segment rank loop over 4096 entries, class 4+), document 3 has one row (every entry row 0 or -1)."""
    lens = [300, 150, 64, 1, 400, 77]
    pb = Problem(lens, 32, Lq, _all_pairs(32, len(lens), times=2), seed, exact=True)
    pb.plant(5, [40], fill=True)
    pb.plant(0, [0, 299, 64, 63])
    assert pb.n_pd(0) == 64 and pb.n_pd(0) * Lq == (ROWS_MAX_ENT if Lq == 64 else 4160)
    return pb


def case_pd1024(seed):
    """512 queries of 4 tokens, every document paired with each query twice: n_pd = 1024 = kRowsMaxPairs, n_ent = 4096."""
    lens = [900, 33, 5]
    pb = Problem(lens, 512, 4, _all_pairs(512, 3, times=2), seed, exact=True)
    pb.plant(1, [7], fill=True)                                                  # 4096 entries on one row of a 33-row document
    assert all(pb.n_pd(c) == ROWS_MAX_PAIRS for c in range(3))
    return pb


def case_overflow_entries(seed):
    """Run-time overflow of the entry list: the host bound (2 * 4 * 33 = 264 entries per document) holds for the list's shape, but
    document 0 meets the queries 125 times (4125 > 4096 entries: the direct walk) and document 2 124 times (4092: the LDS lists)."""
    lens = [200, 90, 130, 5]
    lst = [(0, 0)] * 40 + [(1, 0)] * 40 + [(2, 0)] * 20 + [(3, 0)] * 25 + [(b, 1) for b in range(4)]
    lst += [(0, 2)] * 31 + [(1, 2)] * 31 + [(2, 2)] * 31 + [(3, 2)] * 31 + [(1, 3)]
    pb = Problem(lens, 4, 33, lst, seed)
    pb.plant(0, [0, 199, 199, 17])
    pb.plant(2, [129, 0])
    assert pb.n_pd(0) * 33 == 4125 and pb.n_pd(2) * 33 == 4092
    return pb


def case_overflow_pairs(seed):
    """Run-time overflow of the pair list at Lq = 1: document 0 has 1025 pairs (> kRowsMaxPairs, 1025 entries), document 1 exactly 1024."""
    lens = [200, 300, 3]
    lst = [(k % 4, 0) for k in range(1025)] + [(k % 4, 1) for k in range(1024)] + [(b, 2) for b in range(4)]
    pb = Problem(lens, 4, 1, lst, seed)
    pb.plant(1, [299, 0, 0, 150])
    assert pb.n_pd(0) == ROWS_MAX_PAIRS + 1 and pb.n_pd(1) == ROWS_MAX_PAIRS
    return pb


def case_guess_refuted(seed):
    """n_pairs divisible by n_d with UNEQUAL counts per document (3, 5, 1, 3): the per-document guess is refuted by its probes and the
    counting pass finds the ranges; document 2 has length 0 (its pair is routed all -1)."""
    lens = [500, 70, 0, 260]
    lst = [(0, 0), (1, 0), (5, 0), (0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (3, 2), (2, 3), (4, 3), (5, 3)]
    pb = Problem(lens, 6, 24, lst, seed)
    pb.plant(0, [499, 0, 499])
    assert pb.n_pairs % pb.n_d == 0 and [pb.n_pd(c) for c in range(4)] == [3, 5, 1, 3]
    return pb


def case_search(seed, n_pairs):
    """64 queries x 300 documents, n_pairs unique pairs at random: unequal counts, so no guess; 16384 pairs are looked up by the
    workgroup's counting pass (kRowsCountPairs), 16385 by the wave-wide binary searches.  (dQ: 1024 tokens with >= 64 pairs per query on
    average: psplit.)"""
    gen = torch.Generator().manual_seed(seed)
    n_q, n_d = 64, 300
    lens = torch.randint(1, 101, (n_d,), generator=gen).tolist()
    lens[299] = 0
    idx = torch.randperm(n_q * (n_d - 1), generator=gen)[:n_pairs]
    lst = [(int(k) // (n_d - 1), int(k) % (n_d - 1)) for k in idx]
    pb = Problem(lens, n_q, 16, lst, seed)
    counts = torch.bincount(pb.pairs[:, 1].long(), minlength=n_d)
    assert int(counts.max()) != int(counts.min()) and int(counts[299]) == 0
    return pb


def case_left_padded(seed):
    """The left-padded-query pattern: ColbertLoss's dense list (32 queries x 8 pages of 780 rows); per page ~300 of its 1024 entries on
    row 0 (the padding tokens of the queries), the others on distinct rows, about one per row; -1 entries mixed in."""
    lens = [780] * 8
    pb = Problem(lens, 32, 32, _all_pairs(32, 8), seed, neg_frac=0.03)
    gen = torch.Generator().manual_seed(seed + 1)
    for c in range(8):
        p, i = pb.entries_of(c)
        rows = torch.zeros(p.numel(), dtype=torch.int32)
        rest = torch.randperm(p.numel(), generator=gen)[: p.numel() - 300]
        rows[rest] = (torch.randperm(779, generator=gen)[: rest.numel()] + 1).to(torch.int32)
        pb.argmax[p, i] = torch.where(pb.argmax[p, i] < 0, pb.argmax[p, i], rows)
    return pb


ROWS_CASES = {
    "sy1_range_1024": case_sy1,
    "sy2_ranges_1024": case_sy2,
    "entries_4096": case_ent4096,
    "pairs_1024": case_pd1024,
    "overflow_entries": case_overflow_entries,
    "overflow_pairs": case_overflow_pairs,
    "guess_refuted": case_guess_refuted,
    "counting_16384": lambda seed: case_search(seed, ROWS_COUNT_PAIRS),
    "search_16385": lambda seed: case_search(seed, ROWS_COUNT_PAIRS + 1),
    "left_padded": case_left_padded,
}


@pytest.mark.parametrize("dtype,dim", DTYPE_WIDTH)
@pytest.mark.parametrize("case", list(ROWS_CASES))
def test_row_list_dd_at_its_limits(amd, case, dtype, dim):
    """The row-list dD kernel (maxsim_bwd_dd_rows_kernel) on every limit it has: one workgroup's range of exactly kRowsMaxRows rows
    (sy = 1 and sy = 2), kRowsMaxEnt entries and kRowsMaxPairs pairs per document, run-time overflows of both lists (the direct walk),
    the three pair-range lookups (proven guess, counting pass, binary search), crowded rows (4096 entries on one row; 300 on row 0),
    -1 routing and length-0 documents.  Widths 128 and 320 (a partial last 128-column chunk)."""
    pb = ROWS_CASES[case](17)
    assert pb.form(dim)[0] == "rows"
    check_bwd(pb, dtype, dim)


@pytest.mark.parametrize("dtype,dim", [DTYPE_WIDTH[0], DTYPE_WIDTH[5]])
def test_one_entry_over_the_host_bound_takes_the_row_range_kernel(amd, dtype, dim):
    """2 * n_q * Lq = 4160 > kRowsMaxEnt: the host cannot bound the lists and launches the row-range kernel (maxsim_bwd_dd_kernel) --
    the same values, including the document whose 4160 entries all sit on one row."""
    pb = case_ent4096(23, Lq=65)
    assert pb.form(dim)[0] == "range"
    check_bwd(pb, dtype, dim)


# ---- dQ (maxsim_bwd_dq_kernel)
def dq_problem(seed, n_q, Lq, counts, n_d=40, max_len=64):
    """Query b gets counts[b] pairs with documents drawn at random (repeats allowed); short ragged documents, one of length 0."""
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_len + 1, (n_d,), generator=gen).tolist()
    lens[n_d // 2] = 0
    lst = [(b, int(c)) for b, k in enumerate(counts) for c in torch.randint(0, n_d, (int(k),), generator=gen)]
    return Problem(lens, n_q, Lq, lst, seed)


def _psplit_cases():
    return {
        # tokens = 2048 with 64 pairs per query: psplit
        "psplit_2048_tokens": dict(n_q=16, Lq=128, counts=[64] * 16, psplit=True, tpw=1),
        # 2064 tokens: no psplit
        "no_psplit_2064_tokens": dict(n_q=16, Lq=129, counts=[64] * 16, psplit=False, tpw=1),
        # one pair short of 64 per query on average (unequal counts: the per-query guess is refuted), no psplit
        "no_psplit_1023_pairs": dict(n_q=16, Lq=128, counts=[64] * 15 + [63], psplit=False, tpw=1),
        # psplit with unequal counts, queries without pairs
        "psplit_ragged": dict(n_q=8, Lq=100, counts=[200, 0, 1, 130, 0, 100, 48, 33], psplit=True, tpw=1),
        # tokens 13 000: tpw = 4, Lq not a multiple of 4 * tpw
        "tpw_4": dict(n_q=13, Lq=1000, counts=[9] * 13, psplit=False, tpw=4),
        # tokens 62 000: tpw at its cap of 16, Lq % 64 = 40
        "tpw_16": dict(n_q=62, Lq=1000, counts=[9] * 62, psplit=False, tpw=16),
        # few pairs per query: 8 (few-pairs branch where G > 1) against 9 (the pair-group branch), 0 and 1 pair; a refuted guess
        "few_pairs_8_9": dict(n_q=6, Lq=45, counts=[8, 9, 7, 0, 8, 4], psplit=False, tpw=1),
        # every query 8 pairs: the guess holds, every query in the few-pairs branch
        "few_pairs_all_8": dict(n_q=5, Lq=77, counts=[8] * 5, psplit=False, tpw=1),
    }


DQ_CASES = _psplit_cases()


@pytest.mark.parametrize("dtype,dim", DTYPE_WIDTH)
@pytest.mark.parametrize("case", list(DQ_CASES))
def test_dq_kernel_forms(amd, case, dtype, dim):
    """The dQ kernel's launch forms: psplit on either side of 2048 tokens and of 64 pairs per query, tokens per wave 1 / 4 / 16 with Lq
    not a multiple of 4 * tpw, the few-pairs branch at 8 against 9 pairs per query (off where G == 1: width 320 in 16-bit, and fp32
    at 320), refuted per-query guesses, queries without pairs and -1 entries.  dD of the same call is checked too."""
    spec = DQ_CASES[case]
    pb = dq_problem(31, spec["n_q"], spec["Lq"], spec["counts"])
    tpw, psplit = dq_plan(pb.n_q, pb.Lq, pb.n_pairs)
    assert (tpw, psplit) == (spec["tpw"], spec["psplit"])
    G = dq_groups(dim, dtype)
    assert (G > 1) == (dim == 128)
    few = [few_pairs(k, G, psplit) for k in spec["counts"]]
    if case.startswith("few_pairs") and dim == 128:
        assert few == [k <= 8 for k in spec["counts"]]
    if dim == 320:
        assert not any(few)
    check_bwd(pb, dtype, dim)


# ---- dense / workspace dD (dd_plan modes 1 and 2)
def dense_problem(seed, n_q, n_d, Lq, pairs_per_query, max_len, drop=0, dim_hint=None):
    gen = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_len + 1, (n_d,), generator=gen).tolist()
    lens[0] = max_len
    if n_d > 3:
        lens[3] = 0
    if pairs_per_query >= n_d:
        lst = _all_pairs(n_q, n_d)
    else:
        lst = [(b, int(c)) for b in range(n_q) for c in torch.randperm(n_d, generator=gen)[:pairs_per_query]]
    lst = lst[: len(lst) - drop]
    return Problem(lens, n_q, Lq, lst, seed)


DENSE_CASES = {
    # entries_per_doc = 32 * 32 * 8 / 8 = 1024: mode 1; one pair fewer: 1020 and Lq < 256: no dense form
    "epd_1024": (dict(n_q=32, n_d=8, Lq=32, pairs_per_query=8, max_len=64), 1),
    "epd_1020": (dict(n_q=32, n_d=8, Lq=32, pairs_per_query=8, max_len=64, drop=1), 0),
    # Lq = 256 with few entries per document: mode 2; Lq = 255: none
    "lq_256": (dict(n_q=4, n_d=16, Lq=256, pairs_per_query=2, max_len=40), 2),
    "lq_255": (dict(n_q=4, n_d=16, Lq=255, pairs_per_query=2, max_len=40), 0),
    # documents of up to 64 rows: mode 1; 65: none
    "rows_64": (dict(n_q=12, n_d=6, Lq=96, pairs_per_query=6, max_len=64), 1),
    "rows_65": (dict(n_q=12, n_d=6, Lq=96, pairs_per_query=6, max_len=65), 0),
}


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
@pytest.mark.parametrize("case", list(DENSE_CASES))
def test_dense_dd_forms_on_both_sides_of_their_thresholds(amd, case, dtype):
    """dd_plan's thresholds from both sides -- entries per document 1024, Lq 256, documents of 64 rows -- with and without the workspace:
    every call equal to the float64 truth (the two forms are equal only up to fp32 summation order, so not compared bitwise)."""
    spec, mode = DENSE_CASES[case]
    pb = dense_problem(41, **spec)
    assert dd_plan(pb.n_pairs, pb.Lq, pb.n_d, 128, pb.max_doc_rows, cus())[0] == mode
    for ws in (True, False):
        if not ws or mode:
            check_bwd(pb, dtype, 128, workspace=ws)


@pytest.mark.parametrize("n_pairs,mode", [(512, 2), (513, 0)])
def test_dense_dd_scratch_cap(amd, n_pairs, mode):
    """The 256 MB scratch cap: mode 2 at width 512 with Lq = 256 (4 splits) needs n_pairs * 512 KiB -- exactly 256 MiB for 512 pairs
    (kept), one pair more falls back to the row-range kernel (no scratch)."""
    pb = dense_problem(43, n_q=128, n_d=200, Lq=256, pairs_per_query=4, max_len=64)
    if n_pairs > 512:
        pb = Problem(pb.lens, 128, 256, [tuple(x) for x in pb.pairs.tolist()] + [(127, 1)], 43)
    assert pb.n_pairs == n_pairs
    _, _, nbytes = dd_plan(pb.n_pairs, pb.Lq, pb.n_d, 512, pb.max_doc_rows, cus())
    assert dd_plan(pb.n_pairs, pb.Lq, pb.n_d, 512, pb.max_doc_rows, cus())[0] == mode
    assert nbytes == (256 << 20 if mode else 0)
    check_bwd(pb, torch.bfloat16, 512, workspace=True)
    if mode:
        check_bwd(pb, torch.bfloat16, 512, workspace=False)
