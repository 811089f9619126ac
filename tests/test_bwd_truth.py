"""CPU: the float64 truth of the hard-max backward (tests/helpers.py: pairs_bwd_truth) against torch autograd of the expression it
claims to be the gradient of -- scores[p] = sum_i <Q[b_p, i], D[d_off[c_p] + argmax[p, i]]> over the tokens whose routing is not -1,
loss = sum_p g[p] * scores[p] -- on a tiny ragged corpus with a length-0 document, a repeated pair and -1 routing."""
import torch

from tests.helpers import pairs_bwd_truth


def test_pairs_bwd_truth_is_the_autograd_of_the_routed_gather():
    gen = torch.Generator().manual_seed(5)
    n_q, Lq, dim = 3, 5, 8
    lens = [4, 0, 3, 6]
    off = torch.tensor([0] + list(torch.cumsum(torch.tensor(lens), 0)), dtype=torch.int32)
    pairs = torch.tensor([(0, 0), (0, 2), (0, 2), (1, 3), (1, 1), (2, 0), (2, 3)], dtype=torch.int32)   # query 0 meets document 2 twice
    Q = torch.randn(n_q, Lq, dim, generator=gen, dtype=torch.float64)
    D = torch.randn(int(off[-1]), dim, generator=gen, dtype=torch.float64)
    g = torch.randn(pairs.shape[0], generator=gen, dtype=torch.float64)
    argmax = torch.full((pairs.shape[0], Lq), -1, dtype=torch.int32)
    for p, (_, c) in enumerate(pairs.tolist()):
        if lens[c]:
            argmax[p] = torch.randint(-1, lens[c], (Lq,), generator=gen, dtype=torch.int32)
    argmax[0, :3] = 0                                                    # several tokens of one pair on one row
    want_dq, want_dd = pairs_bwd_truth(Q, D, off, pairs, g, argmax)

    q, d = Q.clone().requires_grad_(True), D.clone().requires_grad_(True)
    am, pr = argmax.long(), pairs.long()
    ok = am >= 0
    rows = off.long()[pr[:, 1]].unsqueeze(1) + am.clamp_min(0)
    scores = (q[pr[:, 0]] * d[rows]).sum(-1).where(ok, torch.zeros((), dtype=torch.float64)).sum(1)
    (g * scores).sum().backward()
    assert torch.allclose(want_dq, q.grad, rtol=0, atol=1e-12)
    assert torch.allclose(want_dd, d.grad, rtol=0, atol=1e-12)
    assert float(want_dd[off[2]:off[3]].abs().sum()) > 0 and float(want_dq[1].abs().sum()) > 0
