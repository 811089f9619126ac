"""The scorer and loss contracts of `colpali_engine` as its callers see them, checked through the stub package under stub/.

Run as a script in a subprocess (tests/test_gpu_reference_suite.py, tests/test_host_path.py) with stub/ and the repository on
PYTHONPATH: `python contract_checks.py {scorer|losses|helpers}`.  REFSUITE_DEVICE names the device new tensors default to ("cpu": the
torch default).  Prints "<n> passed" and exits 0 when every check of the group holds; prints the failures and exits 1 otherwise.
"""
import math
import os
import sys
import traceback

import torch
import torch.nn.functional as F

from colpali_engine.loss import (ColbertLoss, ColbertModule, ColbertNegativeCELoss, ColbertPairwiseCELoss,
                                 ColbertPairwiseNegativeCELoss)
from colpali_engine.utils.processing_utils import BaseVisualRetrieverProcessor as P


def _maxsim_f64(qs, ps):
    """Late-interaction scores in float64 with every page zero-padded to the longest one (what a single scoring block sees)."""
    n = max(p.shape[0] for p in ps)
    pad = torch.zeros(len(ps), n, ps[0].shape[1], dtype=torch.float64, device="cpu")
    for j, p in enumerate(ps):
        pad[j, : p.shape[0]] = p.double().cpu()
    return torch.stack([torch.einsum("qd,jnd->jqn", q.double().cpu(), pad).amax(dim=2).sum(dim=1) for q in qs])


def scorer_single_vector():
    g = torch.Generator().manual_seed(5)
    qs = [torch.randn(24, generator=g, device="cpu").to(torch.get_default_device()) for _ in range(3)]
    ps = [torch.randn(24, generator=g, device="cpu").to(torch.get_default_device()) for _ in range(7)]
    got = P.score_single_vector(qs, ps)
    assert got.shape == (3, 7)
    want = torch.stack(qs).double().cpu() @ torch.stack(ps).double().cpu().T
    assert torch.allclose(got.double().cpu(), want, rtol=1e-5, atol=1e-5)


def scorer_multi_vector_list_and_padded_tensor():
    g = torch.Generator().manual_seed(6)
    qs = [torch.randn(n, 32, generator=g, device="cpu").to(torch.get_default_device()) for n in (3, 5)]
    ps = [torch.randn(n, 32, generator=g, device="cpu").to(torch.get_default_device()) for n in (6, 2, 11)]
    from_list = P.score_multi_vector(qs, ps)
    assert from_list.shape == (2, 3)
    from_tensor = P.score_multi_vector(torch.nn.utils.rnn.pad_sequence(qs, batch_first=True),
                                       torch.nn.utils.rnn.pad_sequence(ps, batch_first=True))
    assert from_tensor.shape == (2, 3)
    assert torch.allclose(from_list, from_tensor)
    assert torch.allclose(from_list.double().cpu(), _maxsim_f64(qs, ps), rtol=1e-5, atol=1e-4)


def _zeros(*shape):
    return torch.zeros(*shape)


_PLAIN = dict(temperature=1.0, normalize_scores=False, use_smooth_max=False, pos_aware_negative_filtering=False)


def loss_colbert_zero_embeddings_is_log_batch():
    B = 4
    loss = ColbertLoss(**_PLAIN)(_zeros(B, 1, 5), _zeros(B, 1, 5))
    assert torch.allclose(loss.float().cpu(), torch.tensor(math.log(B), device="cpu"))


def loss_colbert_filtering_leaves_ties_alone():
    q, d = _zeros(3, 1, 5), _zeros(3, 1, 5)
    base = ColbertLoss(**_PLAIN)(q, d)
    filt = ColbertLoss(**dict(_PLAIN, pos_aware_negative_filtering=True))(q, d)
    assert torch.allclose(base.float().cpu(), filt.float().cpu())


def _softplus0():
    return F.softplus(torch.tensor(0.0, device="cpu"))


def loss_pairwise_zero_embeddings_is_softplus0():
    loss = ColbertPairwiseCELoss(**_PLAIN)(_zeros(3, 1, 5), _zeros(3, 1, 5))
    assert torch.allclose(loss.float().cpu(), _softplus0())


def _negatives_case(cls, weight):
    # two pages, one negative each: every term of either loss is a two-way tie, so the weighted mix is softplus(0) = log 2 too
    loss = cls(**_PLAIN, in_batch_term_weight=weight)(_zeros(2, 1, 5), _zeros(2, 1, 5), _zeros(2, 1, 1, 5))
    assert torch.allclose(loss.float().cpu(), _softplus0())


def loss_negative_ce_without_in_batch_term():
    _negatives_case(ColbertNegativeCELoss, 0)


def loss_negative_ce_with_in_batch_term():
    _negatives_case(ColbertNegativeCELoss, 0.5)


def loss_pairwise_negative_ce_without_in_batch_term():
    _negatives_case(ColbertPairwiseNegativeCELoss, 0)


def loss_pairwise_negative_ce_with_in_batch_term():
    _negatives_case(ColbertPairwiseNegativeCELoss, 0.5)


def helper_get_idx():
    idx, pos = ColbertModule(max_batch_size=8)._get_idx(batch_size=4, offset=3, device=torch.device("cpu"))
    assert idx.tolist() == [0, 1, 2, 3] and pos.tolist() == [3, 4, 5, 6]


def helper_smooth_max():
    tau = 0.5
    out = ColbertModule(tau=tau)._smooth_max(torch.tensor([[1.0, 1.0, 1.0]]), dim=1)
    assert torch.allclose(out, torch.tensor([1.0 + tau * math.log(3.0)]))


def helper_normalization_within_bounds():
    scores = torch.tensor([[0.9, 0.3], [1.2, 0.6]])
    lengths = torch.tensor([3.0, 2.0])
    out = ColbertModule(norm_tol=1e-3)._apply_normalization(scores, lengths)
    assert torch.allclose(out, scores / lengths[:, None])


def helper_aggregate_max():
    raw = torch.tensor([[[0.5, -1.0, 2.0], [3.0, 1.0, 0.0]], [[-2.0, -1.0, -3.0], [4.0, 4.5, 1.0]]])
    out = ColbertModule()._aggregate(raw, use_smooth_max=False, dim_max=2, dim_sum=1)
    assert torch.allclose(out, torch.tensor([5.0, 3.5]))


def helper_aggregate_smooth_max():
    out = ColbertModule(tau=1.0)._aggregate(torch.zeros(2, 3, 4), use_smooth_max=True, dim_max=2, dim_sum=1)
    assert torch.allclose(out, torch.full((2,), 3 * math.log(4.0)))


def helper_filter_high_negatives():
    scores = torch.tensor([[0.8, 0.9, 0.1], [0.2, 0.5, 0.3], [0.95, 0.1, 1.0]])
    before = scores.clone()
    ColbertModule(filter_threshold=0.95, filter_factor=0.25)._filter_high_negatives(scores, torch.tensor([0, 1, 2]))
    # 0.9 > 0.95 * 0.8 and 0.95 > 0.95 * 1.0 is false: only the first row's negative above the threshold is scaled
    want = before.clone()
    want[0, 1] = 0.9 * 0.25
    assert torch.allclose(scores, want)


GROUPS = {
    "scorer": (scorer_single_vector, scorer_multi_vector_list_and_padded_tensor),
    "losses": (loss_colbert_zero_embeddings_is_log_batch, loss_colbert_filtering_leaves_ties_alone, loss_pairwise_zero_embeddings_is_softplus0,
               loss_negative_ce_without_in_batch_term, loss_negative_ce_with_in_batch_term,
               loss_pairwise_negative_ce_without_in_batch_term, loss_pairwise_negative_ce_with_in_batch_term),
    "helpers": (helper_get_idx, helper_smooth_max, helper_normalization_within_bounds, helper_aggregate_max,
                helper_aggregate_smooth_max, helper_filter_high_negatives),
}


def main(group):
    dev = os.environ.get("REFSUITE_DEVICE", "cpu")
    if dev != "cpu":
        torch.set_default_device(dev)
    failed = []
    for check in GROUPS[group]:
        try:
            check()
        except Exception:
            failed.append(check.__name__)
            print(f"FAILED {check.__name__}\n{traceback.format_exc()}")
    print(f"{len(GROUPS[group]) - len(failed)} passed" + (f", {len(failed)} failed" if failed else ""))
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
