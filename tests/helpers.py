"""Shared helpers for the parity tests (CPU side only; no product imports)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

from oracle import maxsim_oracle as mo


def split_rows(flat: np.ndarray, lens) -> list:
    out, o = [], 0
    for n in lens:
        out.append(flat[o : o + int(n)])
        o += int(n)
    return out


def ragged_from_golden(z):
    """score_ragged_d128.npz -> (list of uint16 [L,dim] queries, list of docs)."""
    dim = int(z["dim"])
    q = z["q_bits"].reshape(-1, dim)
    p = z["p_bits"].reshape(-1, dim)
    return split_rows(q, z["q_lens"]), split_rows(p, z["p_lens"])


def config1_inputs(z):
    """Regenerate BASELINE config-1 inputs from the seed and check their sha256."""
    import hashlib

    import torch
    import torch.nn.functional as F

    g = torch.Generator().manual_seed(int(z["seed"]))

    def unit(n):
        return F.normalize(torch.randn(n, int(z["dim"]), generator=g), dim=-1).to(torch.bfloat16)

    qs = [unit(int(z["Lq"])) for _ in range(int(z["n_q"]))]
    ps = [unit(int(z["Ld"])) for _ in range(int(z["n_d"]))]
    h = hashlib.sha256()
    for t in qs + ps:
        h.update(t.contiguous().view(torch.int16).numpy().tobytes())
    assert h.digest() == z["sha256"].tobytes(), "torch RNG stream changed: regenerate tests/golden"
    return qs, ps


def bits_list_to_f32(lst):
    return [mo.bf16_bits_to_f32(x) for x in lst]


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-6)))


def topk_tie_aware_equal(got_idx, truth_scores, k, rtol=1e-6):
    """Top-k index parity that tolerates permutations only inside exact/near ties.

    `truth_scores` is the oracle's score row; `got_idx` the candidate top-k.
    Accept iff for every rank r the truth score of got_idx[r] equals the r-th
    best truth score within rtol (so a differing index is only allowed when the
    two documents are indistinguishable at the oracle's own precision).
    """
    order = np.argsort(-truth_scores, kind="stable")[:k]
    want = truth_scores[order]
    got = truth_scores[np.asarray(got_idx[:k], dtype=np.int64)]
    return bool(np.all(np.abs(got - want) <= rtol * np.maximum(np.abs(want), 1.0)))


def planted_inputs(z, tag):
    """Regenerate the planted-retrieval inputs of topk_planted.npz (tests/golden/make_golden.py:planted_inputs, restated
    here because that file imports the live reference) and check their sha256.  Returns (queries, docs) as bf16 tensors."""
    import hashlib

    import torch
    import torch.nn.functional as F

    seed, n_q, Lq, n_d, lo, hi, n_pl = (int(v) for v in z[f"{tag}_params"])
    dim = 128
    g = torch.Generator().manual_seed(seed)

    def unit(n):
        return F.normalize(torch.randn(n, dim, generator=g), dim=-1).to(torch.bfloat16)

    qs = [unit(Lq) for _ in range(n_q)]
    lens = [lo] * n_d if lo == hi else torch.randint(lo, hi + 1, (n_d,), generator=g).tolist()
    ps = [unit(n).float() for n in lens]
    slots = torch.randperm(n_d, generator=g)[: n_q * n_pl].view(n_q, n_pl)
    for qi in range(n_q):
        for j in range(n_pl):
            d = int(slots[qi, j])
            sigma = 0.3 + 0.05 * j
            noisy = F.normalize(qs[qi].float() + sigma * torch.randn(Lq, dim, generator=g) / dim**0.5, dim=-1)
            rows = torch.randperm(lens[d], generator=g)[:Lq]
            ps[d][rows] = noisy
    ps = [p.to(torch.bfloat16) for p in ps]
    h = hashlib.sha256()
    for t in qs + ps:
        h.update(t.contiguous().view(torch.int16).numpy().tobytes())
    assert h.digest() == z[f"{tag}_sha256"].tobytes(), "torch RNG stream changed: regenerate tests/golden/topk_planted.npz"
    return qs, ps


def ranking_tolerance(got_scores, truth_scores, cap=2e-6):
    """Tolerance for the tie-aware ranking comparison: two documents may swap ranks only if their truth scores are closer
    than twice the largest relative score error actually measured (two computations that agree to e cannot disagree on the
    order of scores further apart than 2e).  The measured error itself must stay under cap / 2."""
    got = np.asarray(got_scores, dtype=np.float64)
    truth = np.asarray(truth_scores, dtype=np.float64)
    e = float(np.max(np.abs(got - truth) / np.maximum(np.abs(truth), 1.0)))     # same error measure as every score test
    assert 2 * e <= cap, f"score error {e:.3e} too large for a meaningful ranking comparison"
    return 2 * e + 1e-9


_REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
_SUITE = os.path.join(_REPO, "tests", "reference_suite")


def run_contract_checks(group, device, **env_extra):
    """tests/reference_suite/contract_checks.py <group> in a subprocess whose `colpali_engine` is the stub package (colpali_amd's scorers
    and loss classes); `device` is the default device of new tensors there.  Asserts a zero exit status and returns stdout."""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(_SUITE, "stub"), _REPO]), REFSUITE_DEVICE=device,
               PYTHONDONTWRITEBYTECODE="1", **env_extra)
    res = subprocess.run([sys.executable, os.path.join(_SUITE, "contract_checks.py"), group],
                         capture_output=True, text=True, env=env, cwd=_SUITE, timeout=600)
    assert res.returncode == 0, (res.stdout + res.stderr)[-3000:]
    return res.stdout


def pairs_bwd_truth(Q, D, d_off, pairs, g, argmax, chunk=1 << 15):
    """float64 (dQ [n_q, Lq, dim], dD [total_rows, dim]) of msim_pairs_bwd's contract (include/maxsim.h):
        dQ[b_p, i]                 += g[p] * D[d_off[c_p] + argmax[p, i]]
        dD[d_off[c_p] + argmax[p, i]] += g[p] * Q[b_p, i]
    for every (pair p, token i) whose routing is not -1 (-1: the zero padding row won the max).  Only the rows that carry entries
    are gathered, `chunk` entries at a time."""
    import torch

    Q, D = torch.as_tensor(Q).double(), torch.as_tensor(D).double()
    n_q, Lq, dim = Q.shape
    am, pr, off, gg = (torch.as_tensor(x).cpu() for x in (argmax, pairs, d_off, g))
    am, pr, off, gg = am.long().view(-1, Lq), pr.long().view(-1, 2), off.long(), gg.double()
    p, i = (am >= 0).nonzero(as_tuple=True)
    b, c = pr[p, 0], pr[p, 1]
    assert bool((am[p, i] < off[c + 1] - off[c]).all()), "routing beyond the document's rows"
    row = off[c] + am[p, i]
    dQ = torch.zeros(n_q * Lq, dim, dtype=torch.float64)
    dD = torch.zeros(D.shape[0], dim, dtype=torch.float64)
    for s in range(0, p.numel(), chunk):
        sl = slice(s, s + chunk)
        w = gg[p[sl]].unsqueeze(1)
        dQ.index_add_(0, b[sl] * Lq + i[sl], w * D[row[sl]])
        dD.index_add_(0, row[sl], w * Q[b[sl], i[sl]])
    return dQ.view(n_q, Lq, dim), dD


def _smooth_operands(Q, D, d_off, pairs):
    import torch

    Q, D = torch.as_tensor(Q).double(), torch.as_tensor(D).double()
    off = torch.as_tensor(d_off).cpu().long().tolist()
    pr = torch.as_tensor(pairs).cpu().long().view(-1, 2).tolist()
    return Q, D, off, pr


def _pair_chunks(pr, off, Lq, budget):
    """Runs of consecutive pairs whose documents have one length (one batched product each), at most `budget` similarities per run."""
    s = 0
    while s < len(pr):
        n = off[pr[s][1] + 1] - off[pr[s][1]]
        e = s + 1
        while e < len(pr) and off[pr[e][1] + 1] - off[pr[e][1]] == n and (e - s + 1) * Lq * max(n, 1) <= budget:
            e += 1
        yield s, e, n
        s = e


def smooth_truth(Q, D, d_off, pairs, tau, budget=1 << 22):
    """float64 (scores [n_pairs], lse [n_pairs, Lq]) of msim_smooth_pairs' contract (include/maxsim.h):
        lse[p, i] = log sum_{j < len(c_p)} exp(<Q[q_p, i], D[d_off[c_p] + j]> / tau),    scores[p] = sum_i tau * lse[p, i]
    on a ragged packed corpus; a document without rows gives -inf (torch.logsumexp over nothing).  Runs on the device of Q."""
    import torch

    Q, D, off, pr = _smooth_operands(Q, D, d_off, pairs)
    Lq = Q.shape[1]
    lse = torch.empty(len(pr), Lq, dtype=torch.float64, device=Q.device)
    for s, e, n in _pair_chunks(pr, off, Lq, budget):
        qi = torch.tensor([p[0] for p in pr[s:e]], device=Q.device)
        rows = torch.tensor([off[p[1]] for p in pr[s:e]], device=Q.device).unsqueeze(1) + torch.arange(n, device=Q.device)
        S = torch.einsum("pid,pjd->pij", Q[qi], D[rows]) / tau
        lse[s:e] = torch.logsumexp(S, dim=2)
    return tau * lse.sum(1), lse


def smooth_bwd_truth(Q, D, d_off, pairs, g, tau, budget=1 << 22):
    """float64 (dQ [n_q, Lq, dim], dD [rows, dim], AQ, AD) of msim_smooth_pairs_bwd's contract (include/maxsim.h):
        w[p, i, j] = exp(<Q[q_p, i], D[j]> / tau - lse[p, i])
        dQ[q, i]          = sum_{p: q_p = q} g[p] sum_j w[p, i, j] D[d_off[c_p] + j]
        dD[d_off[c] + j]  = sum_{p: c_p = c} g[p] sum_i w[p, i, j] Q[q_p, i]
    AQ / AD are the same sums over absolute values (sum |g| w |x|): the scale a rounding error of the weights is measured against.
    Runs on the device of Q."""
    import torch

    Q, D, off, pr = _smooth_operands(Q, D, d_off, pairs)
    gg = torch.as_tensor(g).double().to(Q.device)
    n_q, Lq, dim = Q.shape
    dev = Q.device
    out = [torch.zeros(n_q, Lq, dim, dtype=torch.float64, device=dev), torch.zeros(D.shape[0], dim, dtype=torch.float64, device=dev),
           torch.zeros(n_q, Lq, dim, dtype=torch.float64, device=dev), torch.zeros(D.shape[0], dim, dtype=torch.float64, device=dev)]
    for s, e, n in _pair_chunks(pr, off, Lq, budget):
        if n == 0:
            continue
        qi = torch.tensor([p[0] for p in pr[s:e]], device=dev)
        rows = torch.tensor([off[p[1]] for p in pr[s:e]], device=dev).unsqueeze(1) + torch.arange(n, device=dev)
        q, d = Q[qi], D[rows]
        S = torch.einsum("pid,pjd->pij", q, d) / tau
        w = torch.exp(S - torch.logsumexp(S, dim=2, keepdim=True))
        gw, aw = gg[s:e].view(-1, 1, 1) * w, gg[s:e].abs().view(-1, 1, 1) * w
        out[0].index_add_(0, qi, torch.einsum("pij,pjd->pid", gw, d))
        out[2].index_add_(0, qi, torch.einsum("pij,pjd->pid", aw, d.abs()))
        out[1].index_add_(0, rows.reshape(-1), torch.einsum("pij,pid->pjd", gw, q).reshape(-1, dim))
        out[3].index_add_(0, rows.reshape(-1), torch.einsum("pij,pid->pjd", aw, q.abs()).reshape(-1, dim))
    return tuple(out)
