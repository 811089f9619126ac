"""GPU: the smooth-max kernels (maxsim_smooth.hip) at every launch form, through the C ABI.

msim_smooth_fwd, msim_smooth_pairs and msim_smooth_pairs_bwd are called with hand-made RAGGED d_off (documents of 0, 1..31 rows,
lengths on both sides of a 32-row slab, max_doc_rows not a multiple of 32), pair lists sorted by query with queries and documents
that no pair names and documents shared by several queries, and the stable by-document permutation.  Truth is the contract formula of
include/maxsim.h in float64 (tests/helpers.py: smooth_truth, smooth_bwd_truth; themselves tested on the CPU in
tests/test_smooth_truth.py) on the exact values the kernels read.  Every case ASSERTS the launcher branch it is named after through a
mirror of abi_train.hip's host-side choices (`plan`, computed from the device's CU count), so that a case cannot drift onto another
branch unnoticed.

Forward: scores and per-token lse within 1e-5 of the truth relative to max(|truth|, 1); dense entry point against the pair-list one over
all pairs under the same bound; an empty document gives -inf (score and lse).

Backward, per element:  |got - truth| <= c * A + floor,   A = sum |g| w |x| at that element (the helper's absolute-value sum).
The kernels get the float64 lse rounded to fp32, so that the bound describes the backward alone.  c is the sum of
  u_w            the weight as the second MFMA sees it: bf16 head + bf16 remainder, 2^-9 * 2^-9 = 2^-18; fp16 head + remainder
                 2^-12 * 2^-12 = 2^-24 (in the normal range); fp32: 0;
  2^-23          the hardware exp2 (about 1 ulp);
  2^-24          the product with g[p];
  2^-24 * X * (n_steps / 2 + 4)
                 the exponent's argument x = S / tau - lse with |x|, |lse| <= X = 2 M / tau + log(longest document), M = the largest
                 |q| |d|: one fp32 rounding of the first product per k-step (n_steps * M / tau <= n_steps * X / 2), 1 / tau and the
                 product with it (X), lse stored as fp32 (X), the difference (X), the product with log2(e) (X);
  2^-24 * depth  the fp32 accumulation: `depth` = the longest chain of additions one output element goes through = the (pair, tile)
                 items of one wave (the mirror counts them: list order, item % waves, pairs strided by n_split) times 32 rows (64 for
                 16-bit: head and remainder), plus the waves of the workgroup, plus n_split.
floor = q * max|g| of the owner's pair list * sum over its pairs of the other side's column sums sum_t |x_t|: what a weight below the
number format's smallest step loses at worst, q = 2^-24 for fp16 (the spacing of fp16 subnormals: weights are normalised by a power of
two near the owner's largest |g| before the split) and 2^-120 for bf16 / fp32 (fp32 exponent range).
An fp32 torch evaluation of the same formula with the weights split the same way (`model_bwd`, CPU) must stay under HALF of this bound:
test_cpu_model_stays_under_half_the_bound measures it without a GPU on every case but the four large ones (config 5 twice, the
grid-stride and the n_split == 1 shapes); worst error / bound there: bf16 0.28, fp16 0.10, fp32 0.16.  The kernels themselves, all
cases, on an MI355X: at most 0.31.
"""
from __future__ import annotations

import functools
import hashlib
import math

import pytest
import torch

from tests.helpers import smooth_bwd_truth, smooth_truth

gpu = pytest.mark.gpu

ESIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}
TOK, WAVES_GENERIC, LDS_PER_CU, PAIRS_RING, SLAB_BYTES = 32, 8, 160 * 1024, 2, 8192     # maxsim_common.hpp, maxsim_generic.hip, abi_common.hpp / abi_core.cpp (device_info)
WAVES_DQ, WAVES_DD = 8, 4                                                                # maxsim_smooth.hip: kSmoothWavesDQ / DD


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def cus():
    """The CU count the library plans with (it reads the same hipDeviceProp field)."""
    return torch.cuda.get_device_properties(torch.device("cuda", torch.cuda.current_device())).multi_processor_count


# ---- mirror of the launcher (colpali_amd/csrc/abi_train.hip: smooth_dispatch, launch_smooth, msim_smooth_pairs, smooth_bwd, smooth_dq_split)
def plan(dtype, dim, n_q, Lq, n_d, n_pairs, n_cus):
    rb = dim * ESIZE[dtype]
    n_steps, tpq = rb // 32, _cdiv(Lq, TOK)
    p = {"n_steps": n_steps, "tpq": tpq}
    # dense forward
    tiles, tile_lds, T = n_q * tpq, TOK * (rb + 16), 2
    while T > 1 and (T * tile_lds > 80 * 1024 or T // 2 >= tiles):
        T >>= 1
    whole = tpq <= T
    per_cu = min(max(LDS_PER_CU // (T * tile_lds), 1), 4)
    wgs = min(_cdiv(n_d, WAVES_GENERIC), n_cus * per_cu)
    p.update(T=T, whole=whole, qpg=(T // tpq if whole else 1), n_pass=(1 if whole else _cdiv(tpq, T)),
             T1_by_lds=2 * tile_lds > 80 * 1024, fwd_tail=n_steps % 4, fwd_trips=_cdiv(n_d, wgs * WAVES_GENERIC) if n_d else 0)
    # pair-list forward
    stream = dim == 128 and dtype != torch.float32 and tpq <= 4
    if stream:
        cap = n_cus * (LDS_PER_CU // (4 * PAIRS_RING * SLAB_BYTES))
        p.update(pairs="stream", TPQ=tpq)
    else:
        cap = n_cus * 8
        p.update(pairs="generic", TPQ=None, pairs_clamped=n_steps % 8 != 0)
    p["pairs_trips"] = _cdiv(n_pairs, 4 * min(_cdiv(n_pairs, 4), cap)) if n_pairs else 0
    # backward
    staged = dtype != torch.float32 and dim == 128
    p.update(bwd="staged" if staged else "generic", hoist=None if staged else rb <= 256, cg=1 if staged else _cdiv(dim, 128),
             n_split=min(max(_cdiv(2 * n_cus, tiles), 1), 32))
    return p


class Case:
    """One problem: packed ragged corpus, queries, a pair list sorted by query, upstream gradients g."""

    def __init__(self, dtype, dim, n_q, Lq, lens, pair_list, tau=0.05, seed=0, norm=1.0, max_doc_rows=None, zero_rows=False):
        self.dtype, self.dim, self.n_q, self.Lq, self.tau = dtype, dim, n_q, Lq, tau
        self.lens = [int(x) for x in lens]
        self.n_d = len(self.lens)
        self.max_doc_rows = max(self.lens) if max_doc_rows is None else max_doc_rows
        gen = torch.Generator().manual_seed(seed)
        pair_list = sorted(pair_list, key=lambda bc: bc[0])                    # stable: sorted by query, as the ABI wants
        self.pairs = torch.tensor(pair_list, dtype=torch.int32).view(-1, 2)
        self.n_pairs = self.pairs.shape[0]
        self.order = torch.sort(self.pairs[:, 1].long(), stable=True).indices.to(torch.int32)
        self.off = torch.zeros(self.n_d + 1, dtype=torch.int32)
        self.off[1:] = torch.cumsum(torch.tensor(self.lens, dtype=torch.int64), 0)
        rows = int(self.off[-1])
        # mixed sign, magnitudes within 1 .. 1e-3
        self.g = (torch.randint(0, 2, (self.n_pairs,), generator=gen).float() * 2 - 1) * 10.0 ** (-3 * torch.rand(self.n_pairs, generator=gen))
        unit = torch.nn.functional.normalize
        self.Q = (unit(torch.randn(n_q, Lq, dim, generator=gen), dim=-1) * norm).to(dtype)
        self.D = (unit(torch.randn(rows, dim, generator=gen), dim=-1) * norm).to(dtype)
        if zero_rows:                                                          # padding rows inside the tensors (they contribute exp(0))
            self.Q[0, : min(3, Lq)] = 0
            self.D[: min(5, rows)] = 0

    def plan(self, n_cus=None):
        return plan(self.dtype, self.dim, self.n_q, self.Lq, self.n_d, self.n_pairs, n_cus or cus())

    def all_pairs(self):
        return torch.tensor([(b, c) for b in range(self.n_q) for c in range(self.n_d)], dtype=torch.int32)

    # ---- the bound of the module docstring
    def depth(self, n_cus=None):
        """(dQ, dD): the longest chain of fp32 additions behind one output element."""
        n_split = self.plan(n_cus)["n_split"]
        per_item = 32 * (1 if self.dtype == torch.float32 else 2)
        tiles_of_doc = [_cdiv(n, 32) for n in self.lens]
        dq_items, by_q = 0, {}
        for b, c in self.pairs.tolist():
            by_q.setdefault(b, []).append(tiles_of_doc[c])
        for lst in by_q.values():
            for s in range(n_split):
                dq_items = max(dq_items, _cdiv(sum(lst[s::n_split]), WAVES_DQ))
        n_pd = torch.bincount(self.pairs[:, 1].long(), minlength=self.n_d).max().item() if self.n_pairs else 0
        dd_items = _cdiv(n_pd * _cdiv(self.Lq, 32), WAVES_DD)
        return dq_items * per_item + WAVES_DQ + n_split, dd_items * per_item + WAVES_DD

    def c(self, n_cus=None):
        u_w = {torch.bfloat16: 2.0**-18, torch.float16: 2.0**-24, torch.float32: 0.0}[self.dtype]
        M = float(self.Q.float().norm(dim=-1).max()) * float(self.D.float().norm(dim=-1).max()) if self.D.shape[0] else 0.0
        X = 2 * M / self.tau + math.log(max(self.max_doc_rows, 1))
        common = u_w + 2.0**-23 + 2.0**-24 + 2.0**-24 * X * (self.plan(n_cus)["n_steps"] / 2 + 4)
        return tuple(common + 2.0**-24 * d for d in self.depth(n_cus))

    def floors(self, g):
        """(dQ [n_q, 1, dim], dD [rows, dim]) floor of the docstring for upstream gradients g."""
        q = 2.0**-24 if self.dtype == torch.float16 else 2.0**-120
        pr, off = self.pairs.long(), self.off.long()
        col_d = torch.zeros(self.n_d + 1, self.dim, dtype=torch.float64)
        col_d.index_add_(0, torch.repeat_interleave(torch.arange(self.n_d), torch.tensor(self.lens)), self.D.double().abs())
        col_q = self.Q.double().abs().sum(1)
        gq, gd = torch.zeros(self.n_q, dtype=torch.float64), torch.zeros(self.n_d, dtype=torch.float64)
        gq.scatter_reduce_(0, pr[:, 0], g.double().abs(), "amax")
        gd.scatter_reduce_(0, pr[:, 1], g.double().abs(), "amax")
        fq = torch.zeros(self.n_q, self.dim, dtype=torch.float64).index_add_(0, pr[:, 0], col_d[pr[:, 1]])
        fd = torch.zeros(self.n_d, self.dim, dtype=torch.float64).index_add_(0, pr[:, 1], col_q[pr[:, 0]])
        doc_of_row = torch.repeat_interleave(torch.arange(self.n_d), torch.tensor(self.lens))
        return (q * gq.view(-1, 1) * fq).unsqueeze(1), (q * gd.view(-1, 1) * fd)[doc_of_row]


def model_bwd(cs, g, lse32):
    """The backward formula in fp32 torch with the weights split as the kernels split them (CPU): what fp32 arithmetic plus the head /
    remainder split costs, without the kernels."""
    Q, D, off = cs.Q.float(), cs.D.float(), cs.off.long().tolist()
    dq, dd = torch.zeros(cs.n_q, cs.Lq, cs.dim), torch.zeros(D.shape[0], cs.dim)
    inv_tau = torch.tensor(1.0) / torch.tensor(cs.tau)
    # fp16: the kernels normalise g by the power of two at the owner's largest |g| before the split and undo it at the store
    pr = cs.pairs.long()
    gmax_q = torch.zeros(cs.n_q).scatter_reduce_(0, pr[:, 0], g.float().abs(), "amax")
    gmax_d = torch.zeros(cs.n_d).scatter_reduce_(0, pr[:, 1], g.float().abs(), "amax")
    pow2 = lambda x: torch.exp2(torch.floor(torch.log2(x))) if cs.dtype == torch.float16 and x > 0 else torch.tensor(1.0)   # noqa: E731

    def split_mm(w, x, scale):
        if cs.dtype == torch.float32:
            return w @ x
        w = w / scale
        hi = w.to(cs.dtype).float()
        lo = (w - hi).to(cs.dtype).float()
        return (hi @ x + lo @ x) * scale

    for p, (b, c) in enumerate(cs.pairs.tolist()):
        if off[c + 1] == off[c]:
            continue
        d = D[off[c]:off[c + 1]]
        w = g[p].float() * torch.exp2(((Q[b] @ d.T) * inv_tau - lse32[p].unsqueeze(1)) * 1.4426950408889634)
        dq[b] += split_mm(w, d, pow2(gmax_q[b]))
        dd[off[c]:off[c + 1]] += split_mm(w.T, Q[b], pow2(gmax_d[c]))
    return dq, dd


# ---- calls through the C ABI
def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def run_dense(cs, Q=None, D=None):
    from colpali_amd import _lib

    lib, dev = _lib.lib(), _dev()
    q, d, off = (cs.Q if Q is None else Q).to(dev), (cs.D if D is None else D).to(dev), cs.off.to(dev)
    if d.shape[0] == 0:
        d = torch.zeros(1, q.shape[-1], dtype=q.dtype, device=dev)
    out = torch.full((cs.n_q, cs.n_d), float("nan"), dtype=torch.float32, device=dev)
    rc = lib.msim_smooth_fwd(_lib.dtype_code(q.dtype), _lib.ptr(q), cs.n_q, cs.Lq, _lib.ptr(d), _lib.ptr(off), cs.n_d, q.shape[-1], cs.tau,
                             _lib.ptr(out), cs.n_d, _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_smooth_fwd")
    torch.cuda.synchronize(dev)
    return out.cpu()


def run_pairs(cs, pairs, Q=None, D=None, fill=float("nan")):
    from colpali_amd import _lib

    lib, dev = _lib.lib(), _dev()
    q, d, off, pr = (cs.Q if Q is None else Q).to(dev), (cs.D if D is None else D).to(dev), cs.off.to(dev), pairs.to(dev)
    n = pairs.shape[0]
    scores = torch.full((n,), fill, dtype=torch.float32, device=dev)
    lse = torch.full((n, cs.Lq), fill, dtype=torch.float32, device=dev)
    rc = lib.msim_smooth_pairs(_lib.dtype_code(q.dtype), _lib.ptr(q), cs.n_q, cs.Lq, _lib.ptr(d), _lib.ptr(off), cs.n_d, q.shape[-1],
                               _lib.ptr(pr), n, cs.tau, _lib.ptr(scores), _lib.ptr(lse), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_smooth_pairs")
    torch.cuda.synchronize(dev)
    return scores.cpu(), lse.cpu()


def run_bwd(cs, g, lse32, Q=None, D=None):
    """One msim_smooth_pairs_bwd call; outputs (and the workspace) pre-filled with NaN.  Returns (dQ, dD) on the host."""
    from colpali_amd import _lib

    lib, dev = _lib.lib(), _dev()
    q, d = (cs.Q if Q is None else Q).to(dev), (cs.D if D is None else D).to(dev)
    dim = q.shape[-1]
    off, pairs, order, gg, ls = (x.to(dev) for x in (cs.off, cs.pairs, cs.order, g.float(), lse32))
    dq = torch.full((cs.n_q, cs.Lq, dim), float("nan"), dtype=torch.float32, device=dev)
    dd = torch.full((max(d.shape[0], 1), dim), float("nan"), dtype=torch.float32, device=dev)
    nbytes = lib.msim_smooth_bwd_workspace_bytes(cs.n_q, cs.Lq, dim)
    n_split = plan(q.dtype, dim, cs.n_q, cs.Lq, cs.n_d, cs.n_pairs, cus())["n_split"]
    assert nbytes == (n_split * cs.n_q * cs.Lq * dim * 4 if n_split > 1 else 0)              # the mirror splits alike
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev) if nbytes else None
    rc = lib.msim_smooth_pairs_bwd(_lib.dtype_code(q.dtype), _lib.ptr(q), cs.n_q, cs.Lq, _lib.ptr(d), _lib.ptr(off), cs.n_d, dim,
                                   cs.max_doc_rows, _lib.ptr(pairs), _lib.ptr(order), _lib.ptr(gg), _lib.ptr(ls), cs.n_pairs, cs.tau,
                                   _lib.ptr(dq), _lib.ptr(dd), _lib.ptr(ws), _lib.current_stream_handle(dev))
    _lib.check(rc, "msim_smooth_pairs_bwd")
    torch.cuda.synchronize(dev)
    return dq.cpu(), dd[: d.shape[0]].cpu()


def _truth_device(cs):
    """float64 torch on the GPU for the large shapes (the truth is plain torch either way), the CPU otherwise."""
    work = sum(cs.lens[c] for c in cs.pairs[:, 1].tolist()) * cs.Lq * cs.dim
    return _dev() if work > 2e9 else torch.device("cpu")


def fwd_close(got, want, what):
    """1e-5 relative to max(|truth|, 1); -inf must be -inf.  Returns the measured maximum."""
    got, want = got.double(), want.double().cpu()
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), f"{what}: an empty document must give -inf"
    assert torch.isfinite(got[~inf]).all(), f"{what}: not finite"
    err = ((got[~inf] - want[~inf]).abs() / want[~inf].abs().clamp_min(1.0)).max().item() if (~inf).any() else 0.0
    print(f"{what}: max err {err:.3e}")
    assert err <= 1e-5, f"{what}: {err:.3e}"
    return err


def bwd_ratio(cs, got, truth, g, what="", check=True):
    """Asserts |got - truth| <= c * A + floor per element; returns the worst error / bound of (dQ, dD) (check=False: inf where a value
    is not finite, nothing asserted: the caller does)."""
    want_dq, want_dd, AQ, AD = (t.cpu() for t in truth)
    fq, fd = cs.floors(g)
    out = []
    for name, x, want, A, c, floor in (("dQ", got[0], want_dq, AQ, cs.c()[0], fq), ("dD", got[1], want_dd, AD, cs.c()[1], fd)):
        assert not check or torch.isfinite(x).all(), f"{what}{name}: not finite"
        bound = c * A + floor
        ratio = ((x.double() - want).abs() / bound.clamp_min(1e-300))[bound > 0]
        worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
        if not bool((x[(bound == 0).expand_as(x)] == 0).all()):                # an element without a contribution must be exactly 0
            worst = float("inf")
        out.append(worst)
        print(f"{what}{name}: worst error / bound {worst:.3f} (c = {c:.3e})")
    assert not check or max(out) <= 1.0, f"{what}error / bound: dQ {out[0]:.3f}, dD {out[1]:.3f}"
    return out


def check_case(cs, dense=True):
    """The module's assertions (see the docstring) for one case."""
    dev = _truth_device(cs)
    Qd, Dd = cs.Q.to(dev), cs.D.to(dev)
    want_s, want_lse = smooth_truth(Qd, Dd, cs.off, cs.pairs, cs.tau)
    got_s, got_lse = run_pairs(cs, cs.pairs)
    fwd_close(got_s, want_s, "scores")
    fwd_close(got_lse, want_lse, "lse")
    again_s, again_lse = run_pairs(cs, cs.pairs)
    assert torch.equal(got_s, again_s) and torch.equal(got_lse, again_lse), "pair forward: two runs differ"
    if dense:
        allp = cs.all_pairs()
        want_all, _ = smooth_truth(Qd, Dd, cs.off, allp, cs.tau)
        d_s = run_dense(cs).view(-1)
        p_s, _ = run_pairs(cs, allp)
        fwd_close(d_s, want_all, "dense scores")
        fwd_close(p_s, want_all, "all-pairs scores")
        fwd_close(d_s, p_s, "dense against pair-list")
        assert torch.equal(d_s, run_dense(cs).view(-1)), "dense forward: two runs differ"
    # backward, fed with the float64 lse rounded to fp32
    truth = smooth_bwd_truth(Qd, Dd, cs.off, cs.pairs, cs.g, cs.tau)
    lse32 = want_lse.float().cpu()
    first = run_bwd(cs, cs.g, lse32)
    second = run_bwd(cs, cs.g, lse32)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1]), "backward: two runs differ"
    named_q = torch.zeros(cs.n_q, dtype=torch.bool)
    named_q[cs.pairs[:, 0].long()] = True
    named_d = torch.zeros(cs.n_d, dtype=torch.bool)
    named_d[cs.pairs[:, 1].long()] = True
    row_named = named_d[torch.repeat_interleave(torch.arange(cs.n_d), torch.tensor(cs.lens))]
    assert bool((first[0][~named_q] == 0).all()), "dQ of a query that no pair names is not exactly 0"
    assert bool((first[1][~row_named] == 0).all()), "dD of a document that no pair names is not exactly 0"
    bwd_ratio(cs, first, truth, cs.g)
    return first


# ---- the cases, named after the branch they pin.  `n_cus` only sizes the shapes that must reach a CU-dependent branch.
RAGGED = [40, 1, 0, 31, 32, 33, 7, 64, 65, 100, 3, 17, 16, 2, 90]          # max 100: not a multiple of 32; document 2 is empty


def _ragged_pairs(n_q, n_d, gen, skip_q=(1,), skip_d=(4,)):
    """A few documents per query; every query but skip_q, every document but skip_d; documents shared by several queries."""
    lst = []
    for b in range(n_q):
        if b in skip_q:
            continue
        k = 1 + int(torch.randint(0, 6, (1,), generator=gen))
        docs = torch.randperm(n_d, generator=gen)[:k].tolist() + [2, 9]     # the empty and the longest document, shared
        lst += [(b, c) for c in sorted(set(docs)) if c not in skip_d]
    return lst


def _small(dtype, dim, Lq, n_q=5, seed=1, every_query=False, **kw):
    gen = torch.Generator().manual_seed(seed)
    skips = dict(skip_q=()) if every_query else {}
    return Case(dtype, dim, n_q, Lq, RAGGED, _ragged_pairs(n_q, len(RAGGED), gen, **skips), seed=seed, zero_rows=True, **kw)


def _config5(dtype):
    """The trainer's forward direction: 32 queries of 32 tokens against 256 pages of 780 rows, all pairs."""
    return Case(dtype, 128, 32, 32, [780] * 256, [(b, c) for b in range(32) for c in range(256)], tau=0.1, seed=5, zero_rows=True)


def _symmetric(n_cus):
    """The trainer's symmetric direction: pages as 780-token "queries" against 32-row "documents", all pairs (tpq = 25)."""
    return Case(torch.bfloat16, 128, 12, 780, [32] * 12, [(b, c) for b in range(12) for c in range(12)], tau=0.1, seed=6)


def _nsplit1(n_cus):
    """2 * CUs token tiles: n_split == 1; two short documents per query, a few queries without pairs."""
    n_q = 2 * n_cus
    gen = torch.Generator().manual_seed(7)
    lens = torch.randint(1, 41, (48,), generator=gen).tolist()
    lst = [(b, int(c)) for b in range(n_q) if b % 7 != 3 for c in torch.randperm(48, generator=gen)[:2]]
    return Case(torch.bfloat16, 64, n_q, 32, lens, lst, seed=7)


def _nsplit_uncapped(n_cus):
    """About n_cus / 2.5 token tiles: n_split = 5 or 6, with queries that have fewer pairs than splits (splits without a pair)."""
    n_q = max(n_cus // 10, 1)
    gen = torch.Generator().manual_seed(8)
    lst = _ragged_pairs(n_q, len(RAGGED), gen, skip_q=(2,)) + [(0, c) for c in (0, 5, 7, 8, 11, 12, 14)]
    return Case(torch.float32, 64, n_q, 100, RAGGED, lst, seed=8)


def _gridstride(n_cus):
    """fp32 x 320 (T == 1 forced by LDS: 3 workgroups per CU): more documents than the dense forward's waves, and more pairs than the
    generic pair forward's, so both grid-stride loops take a second trip.  Documents of 1..3 rows."""
    n_d = n_cus * 3 * WAVES_GENERIC + 37
    gen = torch.Generator().manual_seed(9)
    lens = [1 + (i // 64) % 3 for i in range(n_d)]
    n_q = 1 + _cdiv(4 * n_cus * 8 + 1, n_d)
    return Case(torch.float32, 320, n_q, 20, lens, [(b, c) for b in range(n_q) for c in range(n_d)], seed=9)


CASES = {
    # name: (builder(n_cus), the branches the mirror must report, dense forward too)
    "stream_tpq4_f16_staged_f16": (lambda n: _small(torch.float16, 128, 100), dict(pairs="stream", TPQ=4, bwd="staged", T=2, whole=False, n_pass=2)),
    "stream_tpq1_bf16_staged_bf16": (lambda n: _small(torch.bfloat16, 128, 20), dict(pairs="stream", TPQ=1, bwd="staged", whole=True, qpg=2)),
    "stream_tpq3_f16": (lambda n: _small(torch.float16, 128, 70, seed=2), dict(pairs="stream", TPQ=3, bwd="staged")),
    "generic_pairs_tpq25_symmetric_bf16": (_symmetric, dict(pairs="generic", tpq=25, bwd="staged", whole=False, n_pass=13)),
    "generic_pairs_tpq5_f16x128": (lambda n: _small(torch.float16, 128, 130, n_q=3), dict(pairs="generic", tpq=5, pairs_clamped=False, bwd="staged")),
    "nsplit1_bf16x64_hoist": (_nsplit1, dict(n_split=1, bwd="generic", hoist=True, n_steps=4, fwd_tail=0)),
    "nsplit_uncapped_f32x64_hoist": (_nsplit_uncapped, dict(bwd="generic", hoist=True, n_steps=8, pairs="generic")),
    "gridstride_T1_by_lds_f32x320": (_gridstride, dict(T=1, T1_by_lds=True, n_steps=40, hoist=False, cg=3, pairs_clamped=False)),
    "T1_single_tile_bf16": (lambda n: _small(torch.bfloat16, 128, 32, n_q=1, every_query=True), dict(T=1, T1_by_lds=False, whole=True, qpg=1)),
    "whole_qpg2_odd_nq_bf16x48_ksteps3": (lambda n: _small(torch.bfloat16, 48, 32, n_q=5), dict(T=2, whole=True, qpg=2, n_steps=3, fwd_tail=3, pairs_clamped=True, hoist=True)),
    "ksteps10_bf16x160_nohoist": (lambda n: _small(torch.bfloat16, 160, 45), dict(n_steps=10, fwd_tail=2, pairs_clamped=True, hoist=False, cg=2)),
    "ksteps20_bf16x320": (lambda n: _small(torch.bfloat16, 320, 33, seed=3), dict(n_steps=20, fwd_tail=0, pairs_clamped=True, hoist=False, cg=3)),
    "ksteps3_f32x24_hoist": (lambda n: _small(torch.float32, 24, 40), dict(n_steps=3, fwd_tail=3, pairs_clamped=True, hoist=True, cg=1)),
    "f16x160_nohoist": (lambda n: _small(torch.float16, 160, 50, seed=4), dict(bwd="generic", hoist=False, n_steps=10)),
    "f16x64_hoist": (lambda n: _small(torch.float16, 64, 64), dict(bwd="generic", hoist=True, whole=True, qpg=1)),
    "bf16x96_hoist": (lambda n: _small(torch.bfloat16, 96, 36), dict(bwd="generic", hoist=True, n_steps=6, fwd_tail=2)),
    "large_x_tau001_bf16": (lambda n: _small(torch.bfloat16, 128, 40, tau=0.01, norm=2.0), dict(pairs="stream", TPQ=2, bwd="staged")),
    "large_x_tau001_f32x64": (lambda n: _small(torch.float32, 64, 40, tau=0.01, norm=2.0), dict(pairs="generic", bwd="generic", hoist=True)),
    "config5_bf16": (lambda n: _config5(torch.bfloat16), dict(pairs="stream", TPQ=1, bwd="staged", whole=True, qpg=2)),
    "config5_f32": (lambda n: _config5(torch.float32), dict(pairs="generic", bwd="generic", hoist=False, n_steps=16)),
}
SMALL = [k for k in CASES if not k.startswith(("config5", "gridstride", "nsplit1", "generic_pairs_tpq25"))]


def build_case(name, n_cus):
    make, want = CASES[name]
    cs = make(n_cus)
    got = cs.plan(n_cus)
    assert {k: got[k] for k in want} == want, (name, got)
    return cs


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_smooth_launch_form(name):
    n = cus()
    cs = build_case(name, n)
    p = cs.plan()
    # what only the device's CU count decides
    if name == "nsplit1_bf16x64_hoist":
        assert p["n_split"] == 1
    if name == "nsplit_uncapped_f32x64_hoist":
        if not 1 < p["n_split"] < 32:
            pytest.skip(f"{n} CUs: no un-capped split at this shape")
        by_q = torch.bincount(cs.pairs[:, 0].long(), minlength=cs.n_q)
        assert int(by_q[by_q > 0].min()) < p["n_split"] < int(by_q.max())               # splits without a pair, splits with several
    if name == "gridstride_T1_by_lds_f32x320":
        assert p["fwd_trips"] == 2 and p["pairs_trips"] >= 2
    if name.startswith("config5"):
        assert p["n_split"] == min(max(_cdiv(2 * n, 32), 1), 32)                         # 16 on a 256-CU part
        assert p["pairs_trips"] == _cdiv(8192, 4 * min(2048, n * (2 if cs.dtype != torch.float32 else 8)))
    if name == "generic_pairs_tpq25_symmetric_bf16":
        assert p["n_split"] == min(max(_cdiv(2 * n, 300), 1), 32)
    check_case(cs, dense=True)


def test_cpu_model_stays_under_half_the_bound():
    """The derived bound against an fp32 torch evaluation of the same formula (no kernels, no GPU): under half on the small cases."""
    worst = {}
    for name in SMALL:
        cs = build_case(name, 256)
        _, lse = smooth_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.tau)
        want_dq, want_dd, AQ, AD = smooth_bwd_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.g, cs.tau)
        got = model_bwd(cs, cs.g, lse.float())
        fq, fd = cs.floors(cs.g)
        c = cs.c(256)
        for x, want, A, cc, fl in ((got[0], want_dq, AQ, c[0], fq), (got[1], want_dd, AD, c[1], fd)):
            bound = cc * A + fl
            r = float(((x.double() - want).abs() / bound.clamp_min(1e-300))[bound > 0].max())
            worst[cs.dtype] = max(worst.get(cs.dtype, 0.0), r)
    print({str(k): round(v, 3) for k, v in worst.items()})
    assert all(v <= 0.5 for v in worst.values()), worst


# ---- zero-column widening: staged against generic backward, stream against generic pair forward
@gpu
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_zero_column_widening_changes_no_bit_of_the_backward(dtype):
    cs = _small(dtype, 128, 70, seed=21)
    narrow, wide = cs.plan(), plan(dtype, 160, cs.n_q, cs.Lq, cs.n_d, cs.n_pairs, cus())
    assert (narrow["bwd"], narrow["pairs"]) == ("staged", "stream") and (wide["bwd"], wide["hoist"], wide["pairs"]) == ("generic", False, "generic")
    Qw, Dw = (torch.nn.functional.pad(t, (0, 32)).contiguous() for t in (cs.Q, cs.D))
    _, want_lse = smooth_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.tau)
    lse32 = want_lse.float()
    dq, dd = run_bwd(cs, cs.g, lse32)
    dqw, ddw = run_bwd(cs, cs.g, lse32, Q=Qw, D=Dw)
    assert torch.equal(dqw[..., :128], dq) and torch.equal(ddw[..., :128], dd), "staged and generic backward differ in some bit"
    assert bool((dqw[..., 128:] == 0).all()) and bool((ddw[..., 128:] == 0).all()), "a padded column is not exactly 0"
    s, lse = run_pairs(cs, cs.pairs)
    sw, lsew = run_pairs(cs, cs.pairs, Q=Qw, D=Dw)
    fwd_close(sw, s, "stream against generic pair forward: scores")
    fwd_close(lsew, lse, "stream against generic pair forward: lse")


# ---- the scale of g
SCALES = [2.0**-30, 2.0**-20, 2.0**-10, 1.0, 2.0**10, 2.0**14]
SCALE_CASES = {"bf16_staged": (torch.bfloat16, 128), "bf16_generic": (torch.bfloat16, 160), "f16_staged": (torch.float16, 128),
               "f16_generic": (torch.float16, 160), "f16_hoist": (torch.float16, 64), "f32": (torch.float32, 64)}


@gpu
@pytest.mark.parametrize("name", list(SCALE_CASES))
def test_backward_is_linear_in_the_scale_of_g(name):
    """g = s * g0 for powers of two s: the truth scales exactly, the bound with it (A and the floor are linear in |g|).  Every s must
    hold the bound and come back finite (max |g| <= 2^14 here; the weights are at most |g|); for bf16 / fp32, got(s) / s is got(1) to
    the bit."""
    dtype, dim = SCALE_CASES[name]
    cs = _small(dtype, dim, 60, seed=31)
    assert cs.plan()["bwd"] == ("staged" if dim == 128 else "generic")
    assert 1e-3 <= float(cs.g.abs().min()) and float(cs.g.abs().max()) <= 1.0 and bool((cs.g < 0).any()) and bool((cs.g > 0).any())
    _, want_lse = smooth_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.tau)
    lse32 = want_lse.float()
    truth1 = smooth_bwd_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.g, cs.tau)
    unit, failed = None, []
    for s in SCALES:
        g = cs.g * s
        got = run_bwd(cs, g, lse32)
        finite = bool(torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all())
        r = bwd_ratio(cs, got, tuple(t * s for t in truth1), g, what=f"s=2^{int(math.log2(s))} ", check=False)
        print(f"{name} s=2^{int(math.log2(s))}: finite={finite} error/bound dQ {r[0]:.3g} dD {r[1]:.3g} sha256(dQ,dD)="
              f"{hashlib.sha256(got[0].numpy().tobytes() + got[1].numpy().tobytes()).hexdigest()[:16]}")
        if not finite or max(r) > 1.0:
            failed.append(f"s=2^{int(math.log2(s))}: finite={finite}, error / bound dQ {r[0]:.3g}, dD {r[1]:.3g}")
        if s == 1.0:
            unit = got
    assert not failed, failed
    if dtype != torch.float16:
        for s in SCALES:
            got = run_bwd(cs, cs.g * s, lse32)
            assert torch.equal(got[0] / s, unit[0]) and torch.equal(got[1] / s, unit[1]), f"s={s}: got(s) / s differs from got(1)"


# ---- pairs with an index out of range: skipped by the forward, outputs untouched (include/maxsim.h)
@gpu
@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 128), (torch.float32, 64)], ids=["stream", "generic"])
def test_forward_skips_out_of_range_pairs_and_leaves_their_outputs(dtype, dim):
    cs = _small(dtype, dim, 40, seed=41)
    assert cs.plan()["pairs"] == ("stream" if dim == 128 else "generic")
    pairs = cs.pairs.clone()
    bad = {1: (-1, 0), 4: (0, cs.n_d), 7: (cs.n_q, 3), 9: (2, -5)}
    for p, bc in bad.items():
        pairs[p] = torch.tensor(bc, dtype=torch.int32)
    got_s, got_lse = run_pairs(cs, pairs, fill=-12345.0)
    want_s, want_lse = smooth_truth(cs.Q, cs.D, cs.off, cs.pairs, cs.tau)
    ok = torch.ones(cs.n_pairs, dtype=torch.bool)
    ok[list(bad)] = False
    assert bool((got_s[~ok] == -12345.0).all()) and bool((got_lse[~ok] == -12345.0).all()), "an out-of-range pair's outputs were written"
    fwd_close(got_s[ok], want_s[ok], "scores of the valid pairs")
    fwd_close(got_lse[ok], want_lse[ok], "lse of the valid pairs")


# ---- the contract of a document without rows (include/maxsim.h)
@gpu
@pytest.mark.parametrize("dtype,dim", [(torch.bfloat16, 128), (torch.float16, 160), (torch.float32, 64)], ids=["bf16", "f16x160", "f32"])
def test_empty_document_gives_minus_inf_and_no_gradient(dtype, dim):
    """Forward: score and lse of a pair whose document has no rows are -inf.  Backward, fed with that -inf lse: the pair contributes
    nothing, every other pair's gradient is what it is without the pair (bit for bit), and everything is finite."""
    cs = _small(dtype, dim, 40, seed=51)
    empty = (cs.pairs[:, 1] == 2)
    assert cs.lens[2] == 0 and int(empty.sum()) >= 2
    s, lse = run_pairs(cs, cs.pairs)
    assert bool((s[empty] == float("-inf")).all()) and bool((lse[empty] == float("-inf")).all())
    assert torch.isfinite(s[~empty]).all() and torch.isfinite(lse[~empty]).all()
    assert bool((run_dense(cs)[:, 2] == float("-inf")).all())
    dq, dd = run_bwd(cs, cs.g, lse)                                   # the kernel's own lse, -inf rows included
    assert torch.isfinite(dq).all() and torch.isfinite(dd).all()
    g0 = cs.g.clone()
    g0[empty] = -g0[empty]                                            # whatever its g: the pair has nothing to give
    dq0, dd0 = run_bwd(cs, g0, lse)
    assert torch.equal(dq, dq0) and torch.equal(dd, dd0)
