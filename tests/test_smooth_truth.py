"""CPU: the float64 truth of the smooth-max entry points (tests/helpers.py: smooth_truth, smooth_bwd_truth) against torch autograd of
the expression they claim to describe -- loss = sum_p g[p] * sum_i tau * logsumexp_j(<Q[q_p, i], D[d_off[c_p] + j]> / tau) -- on a
small ragged corpus with an empty document, a one-row document, a repeated pair and a query / a document that no pair names; and
against oracle/li_loss_oracle.py on a dense box."""
import torch

from oracle import li_loss_oracle as lo
from tests.helpers import smooth_bwd_truth, smooth_truth


def _ragged():
    gen = torch.Generator().manual_seed(11)
    n_q, Lq, dim = 4, 5, 8
    lens = [4, 0, 3, 1, 6, 2]
    off = torch.zeros(len(lens) + 1, dtype=torch.int32)
    off[1:] = torch.cumsum(torch.tensor(lens), 0)
    # query 2 and document 5 appear in no pair; query 0 meets document 2 twice; document 1 is empty
    pairs = torch.tensor([(0, 0), (0, 2), (0, 2), (1, 4), (1, 1), (1, 3), (3, 0), (3, 4)], dtype=torch.int32)
    Q = torch.randn(n_q, Lq, dim, generator=gen, dtype=torch.float64)
    D = torch.randn(int(off[-1]), dim, generator=gen, dtype=torch.float64)
    g = torch.randn(pairs.shape[0], generator=gen, dtype=torch.float64)
    return Q, D, off, lens, pairs, g


def test_smooth_truth_is_logsumexp_and_its_autograd():
    Q, D, off, lens, pairs, g = _ragged()
    tau = 0.3
    scores, lse = smooth_truth(Q, D, off, pairs, tau)
    dQ, dD, AQ, AD = smooth_bwd_truth(Q, D, off, pairs, g, tau)

    q, d = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
    qa, da = Q.abs().requires_grad_(True), D.abs().requires_grad_(True)
    total, total_abs = 0.0, 0.0
    for p, (b, c) in enumerate(pairs.tolist()):
        rows = slice(int(off[c]), int(off[c + 1]))
        want_lse = torch.logsumexp(q[b] @ d[rows].T / tau, dim=1)
        assert torch.allclose(lse[p], want_lse.detach(), rtol=0, atol=1e-12) or lens[c] == 0
        if lens[c] == 0:
            assert bool((lse[p] == float("-inf")).all()) and float(scores[p]) == float("-inf")
            continue                                            # the contract: no gradient from a document without rows
        assert abs(float(scores[p]) - float(tau * want_lse.detach().sum())) <= 1e-12
        total = total + g[p] * tau * want_lse.sum()
        # the absolute-value sums are linear in (|Q|, |D|) with the weights held fixed: sum |g| w <|q|, |d|>
        w = torch.softmax(Q[b] @ D[rows].T / tau, dim=1)
        total_abs = total_abs + g[p].abs() * (w * (qa[b] @ da[rows].T)).sum()
    total.backward()
    total_abs.backward()
    for got, want in ((dQ, q.grad), (dD, d.grad), (AQ, qa.grad), (AD, da.grad)):
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
    assert float(dQ[2].abs().sum()) == 0 and float(dD[int(off[5]):].abs().sum()) == 0      # named by no pair: exactly zero
    assert float(dQ[1].abs().sum()) > 0 and float(dD[int(off[3])].abs().sum()) > 0
    assert bool((AQ >= dQ.abs() - 1e-15).all()) and bool((AD >= dD.abs() - 1e-15).all())


def test_smooth_truth_equals_the_loss_oracle_on_a_dense_box():
    gen = torch.Generator().manual_seed(12)
    B, C, Lq, Ld, dim, tau = 3, 5, 6, 9, 16, 0.1
    Q = torch.nn.functional.normalize(torch.randn(B, Lq, dim, generator=gen, dtype=torch.float64), dim=-1)
    D = torch.nn.functional.normalize(torch.randn(C, Ld, dim, generator=gen, dtype=torch.float64), dim=-1)
    off = torch.arange(C + 1, dtype=torch.int32) * Ld
    pairs = torch.tensor([(b, c) for b in range(B) for c in range(C)], dtype=torch.int32)
    scores, _ = smooth_truth(Q, D.view(-1, dim), off, pairs, tau)
    q, d = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
    want, pos_idx = lo._scores(q, d, 1, False, False, 0.95, 0.5, use_smooth_max=True, tau=tau)
    assert torch.allclose(scores.view(B, C), want.detach(), rtol=0, atol=1e-12)
    # the gradient of the oracle's InfoNCE loss through these scores = the pair-list backward with g = dLoss/dscores
    loss = torch.nn.functional.cross_entropy(want / 0.5, pos_idx)
    G, = torch.autograd.grad(loss, want, retain_graph=True)
    loss.backward()
    want_loss, want_dq, want_dd = lo.loss_and_grads("infonce", Q, D, offset=1, temperature=0.5, normalize_scores=False,
                                                    use_smooth_max=True, tau=tau)
    assert abs(float(loss.detach()) - float(want_loss)) <= 1e-12
    dQ, dD, _, _ = smooth_bwd_truth(Q, D.view(-1, dim), off, pairs, G.reshape(-1), tau)
    assert torch.allclose(dQ, want_dq, rtol=0, atol=1e-12) and torch.allclose(dD.view(C, Ld, dim), want_dd, rtol=0, atol=1e-12)
