"""GPU: ties among REAL document rows.  include/maxsim.h promises "first maximum wins on ties"; every arg-max producer combines partial
maxima across the rows of a lane, the two half-waves, 32-row slabs and waves -- any of those combines could keep the wrong row of a
tie.  Documents here carry exact duplicates of a non-zero row equal to a query token (so that the duplicates ARE the maximum), placed
  - within one lane's accumulator rows (rows 0-3 / 8-11 / ... of a slab sit in lanes 0-31, rows 4-7 / 12-15 / ... in lanes 32-63),
  - across the two half-waves, in both orders,
  - across 32-row slabs (and the waves that own them): r, r + 32, r + 64, r + 96,
  - in the last, partial slab,
and the routing must name the first row of every class.  Then the losses: autograd splits the gradient of a tied maximum evenly
among the tied rows (late_interaction_losses.py:91); the kernels give it all to the first row (tie semantics).  Pinned
here: loss and dQ as the float64 oracle, dD summed over each tie class as the oracle, held by the class' first row, the others 0.
"""
from __future__ import annotations

import pytest
import torch

from oracle import li_loss_oracle as lo
from tests.test_gpu_loss import grads_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def tie_classes(Ld):
    """Row classes of exact duplicates (first row first) for a document of Ld rows."""
    last = (Ld - 1) // 32 * 32                                          # first row of the last slab
    classes = [
        [1, 2, 9],                      # one lane's accumulator rows (lanes 0-31)
        [13, 14, 15],                   # one lane's accumulator rows (lanes 32-63)
        [3, 4],                         # lanes 0-31 first, then lanes 32-63
        [12, 16],                       # lanes 32-63 first, then lanes 0-31
        [last + (Ld - last) // 2, Ld - 1],   # the last slab (partial unless Ld is a multiple of 32)
    ]
    if Ld > 96:
        classes.append([20, 52, 84, 116] if Ld > 116 else [20, 52, 84])  # one row per slab (per wave)
    elif Ld > 32:
        classes.append([20, 52] if Ld > 52 else [20, Ld - 2])
    return classes


def planted(n_q, Lq, n_d, Ld, dtype, seed):
    """Random unit rows; in document c, class k's rows are copies of token k of query c % n_q.  Returns (Q, D, {(b, c): [(token,
    class rows)]})."""
    g = torch.Generator().manual_seed(seed)
    Q = torch.nn.functional.normalize(torch.randn(n_q, Lq, 128, generator=g), dim=-1).to(dtype)
    D = torch.nn.functional.normalize(torch.randn(n_d, Ld, 128, generator=g), dim=-1).to(dtype)
    classes = tie_classes(Ld)
    assert len(classes) <= Lq
    want = {}
    for c in range(n_d):
        b = c % n_q
        for k, rows in enumerate(classes):
            tok = (k * 7 + c) % Lq
            D[c, rows] = Q[b, tok]
            want.setdefault((b, c), []).append((tok, rows))
    return Q, D, want


def check_first(argmax_of, want):
    """argmax_of(b, c) -> int tensor [Lq] of pair (b, c)'s routing; every planted token must route to its class' first row."""
    for (b, c), items in want.items():
        got = argmax_of(b, c)
        for tok, rows in items:
            assert int(got[tok]) == rows[0], f"pair ({b}, {c}) token {tok}: row {int(got[tok])}, the tie class is {rows}"


def pairs_argmax(Q, D, pairs, max_doc_rows):
    from colpali_amd import _lib

    n_q, Lq, dim = Q.shape
    n_d, Ld, _ = D.shape
    q, d = Q.cuda(), D.cuda()
    off = torch.arange(0, (n_d + 1) * Ld, Ld, dtype=torch.int32, device=q.device)
    pr = pairs.cuda()
    am = torch.full((pairs.shape[0], Lq), -7, dtype=torch.int32, device=q.device)
    rc = _lib.lib().msim_pairs_argmax(_lib.dtype_code(Q.dtype), _lib.ptr(q), n_q, Lq, _lib.ptr(d), _lib.ptr(off), None, n_d, dim,
                                      max_doc_rows, _lib.ptr(pr), pairs.shape[0], None, _lib.ptr(am), _lib.current_stream_handle(q.device))
    _lib.check(rc, "msim_pairs_argmax")
    return am.cpu()


def pair_list(n_q, n_d, n_pairs):
    """The all-pairs list repeated up to n_pairs entries, sorted by query."""
    base = [(b, c) for b in range(n_q) for c in range(n_d)]
    lst = sorted((base * (n_pairs // len(base) + 1))[:n_pairs], key=lambda bc: bc[0])
    return torch.tensor(lst, dtype=torch.int32)


def _check_list(Q, D, want, pairs, max_doc_rows):
    am = pairs_argmax(Q, D, pairs, max_doc_rows)
    index = {}
    for p, (b, c) in enumerate(pairs.tolist()):
        index.setdefault((b, c), []).append(p)
    for (b, c), ps in index.items():
        for p in ps[1:]:
            assert torch.equal(am[p], am[ps[0]])                        # the same pair listed twice: the same routing
    check_first(lambda b, c: am[index[(b, c)][0]], {k: v for k, v in want.items() if k in index})


@pytest.mark.parametrize("n_pairs", [16, 600, 1500])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_pair_kernels_keep_the_first_of_tied_rows(amd, dtype, n_pairs):
    """msim_pairs_argmax: one workgroup per pair (<= CUs: deep ring; <= 1024 pairs) and one wave per pair (more); documents of 150 rows
    (a partial fifth slab)."""
    Q, D, want = planted(4, 32, 8, 150, dtype, seed=n_pairs)
    _check_list(Q, D, want, pair_list(4, 8, n_pairs), 150)


@pytest.mark.parametrize("n_pairs", [16, 600])
@pytest.mark.parametrize("Ld", [100, 128])
def test_transposed_pair_kernel_keeps_the_first_of_tied_rows(amd, Ld, n_pairs):
    """msim_pairs_argmax's transposed kernel (queries of more than 128 tokens against documents of at most 128 rows)."""
    Q, D, want = planted(3, 200, 6, Ld, torch.bfloat16, seed=Ld + n_pairs)
    _check_list(Q, D, want, pair_list(3, 6, n_pairs), Ld)


@pytest.mark.parametrize("form", ["fp32", "bf16_no_bound", "bf16_width_256"])
def test_generic_kernel_keeps_the_first_of_tied_rows(amd, form):
    """The generic pair kernel: fp32 embeddings, long queries without a row bound (max_doc_rows = 0), and a width other than 128."""
    if form == "bf16_width_256":
        g = torch.Generator().manual_seed(9)
        Q = torch.nn.functional.normalize(torch.randn(3, 40, 256, generator=g), dim=-1).to(torch.bfloat16)
        D = torch.nn.functional.normalize(torch.randn(5, 150, 256, generator=g), dim=-1).to(torch.bfloat16)
        want = {}
        for c in range(5):
            for k, rows in enumerate(tie_classes(150)):
                tok = (k * 7 + c) % 40
                D[c, rows] = Q[c % 3, tok]
                want.setdefault((c % 3, c), []).append((tok, rows))
        _check_list(Q, D, want, pair_list(3, 5, 15), 150)
        return
    dtype, Lq = (torch.float32, 32) if form == "fp32" else (torch.bfloat16, 200)
    Q, D, want = planted(3, Lq, 5, 150, dtype, seed=7)
    _check_list(Q, D, want, pair_list(3, 5, 15), 0 if form == "bf16_no_bound" else 150)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_all_pairs_kernel_keeps_the_first_of_tied_rows(amd, dtype):
    """msim_allpairs_argmax (a wave scores up to four queries against one document)."""
    from colpali_amd import loss as L_

    for n_q, Lq in ((4, 32), (2, 100)):
        Q, D, want = planted(n_q, Lq, 8, 150, dtype, seed=Lq)
        q, d = Q.cuda(), D.cuda()
        _, am = L_.maxsim_all_pairs(q, d, L_._dense_corpus(d).offsets, want_scores=False)
        am = am.cpu()
        check_first(lambda b, c: am[b * 8 + c], want)


@pytest.mark.parametrize("Ld", [50, 64])
def test_transposed_route_keeps_the_first_of_tied_rows(amd, Ld):
    """The routing bytes of msim_fwd_transposed_route (documents of at most 64 rows, queries streamed)."""
    from colpali_amd import _lib, loss as L_

    Q, D, want = planted(3, 300, 5, Ld, torch.bfloat16, seed=Ld)
    q, d = Q.cuda(), D.cuda()
    assert L_._dense_t_ok(q, d)
    _, _, route = L_._dense_t_forward(q, d)
    lq_pad = _lib.lib().msim_dense_t_route_bytes(3, 300, 5) // 15
    route = route.cpu().view(3, 5, lq_pad)
    check_first(lambda b, c: route[b, c].long(), want)


# ---- the losses
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("cls,kind", [("ColbertPairwiseCELoss", "pairwise"), ("ColbertLoss", "infonce")])
def test_losses_route_a_tied_maximum_to_its_first_row(amd, cls, kind, dtype):
    """Loss and dQ equal the float64 oracle (the tied rows are identical, so the maximum is too); dD summed over each tie class equals
    the oracle's sum (which autograd spreads evenly over the class), held entirely by the class' first row; the other rows hold 0."""
    B, C, Lq, Ld = 6, 6, 32, 150
    Q, D, want = planted(B, Lq, C, Ld, dtype, seed=3)
    want_loss, want_dq, want_dd = lo.loss_and_grads(kind, Q.float(), D.float())
    q = Q.cuda().requires_grad_(True)
    d = D.cuda().requires_grad_(True)
    loss = getattr(amd, cls)()(q, d)
    loss.backward()
    assert abs(float(loss.detach()) - float(want_loss)) <= 2.0**-8 * abs(float(want_loss)) + 1e-6
    assert grads_close(q.grad, want_dq)
    got_dd = d.grad.float().cpu()
    in_class = torch.zeros(C, Ld, dtype=torch.bool)
    for (_, c), items in want.items():
        for _, rows in items:
            in_class[c, rows] = True
            first, rest = rows[0], rows[1:]
            assert grads_close(got_dd[c, first], want_dd[c, rows].sum(0)), (c, rows)
            assert bool((got_dd[c, rest] == 0).all()), (c, rows)
            # the oracle really does split: each tied row holds an equal share
            assert torch.allclose(want_dd[c, rows], want_dd[c, first].expand(len(rows), -1))
    assert grads_close(got_dd, want_dd, ~in_class.unsqueeze(-1).expand_as(want_dd))
