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


# ---------------------------------------------------------------------------------------------------------------------------------
# Far-side inputs (the sign tier: tests/test_gpu_sign_edges.py, tests/test_host_sign_edges.py).  Queries sit at +0.7 u, document rows
# at -0.7 u, both with unit noise orthogonal to u scaled by sqrt(0.51): unit rows whose similarities are -0.49 + 0.51 <n, n'>, i.e.
# negative for every (token, row) pair (largest measured: -0.085 at width 32, -0.24 at 128, -0.33 at 320).  A zero that leaks into a
# per-token max -- a row past the document's end that was not masked, a clamp applied to the wrong document -- then moves a score by
# at least the margin the tests assert on their own float64 truth (0.05), where random unit rows would hide it bit for bit.

# every tail class of the 32-row slab, the 128-row chunk and the 16-row int8 chunk
SIGN_EDGE_LENS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 160, 255, 256, 257, 1023, 1024, 1030]
SIGN_MARGIN = 0.05


def far_side_axis(dim, g):
    """the fixed unit vector u (float64)"""
    import torch

    u = torch.randn(dim, generator=g, dtype=torch.float64)
    return u / u.norm()


def far_side_rows(n, u, side, g, dtype):
    """n rows  side * 0.7 u + sqrt(0.51) noise  (noise: unit, orthogonal to u), cast to dtype; side = +1 queries, -1 document rows"""
    import torch

    noise = torch.randn(n, u.numel(), generator=g, dtype=torch.float64)
    noise = noise - (noise @ u).unsqueeze(1) * u
    noise = noise / noise.norm(dim=1, keepdim=True).clamp_min(1e-300)
    return (side * 0.7 * u + 0.51**0.5 * noise).to(dtype)


def planted_positions(n):
    """where the planted winner may sit in a document of n rows: row 0, the last row, the first row of the last 32-row slab and the
    rows on either side of the first slab and chunk boundaries, where they exist"""
    want = [0, n - 1, (n - 1) // 32 * 32, 31, 32, 127, 128]
    out = []
    for p in want:
        if 0 <= p < n and p not in out:
            out.append(p)
    return out


def far_side_doc_lens(g, lens=SIGN_EDGE_LENS, copies=2, n_empty=4, max_len=None):
    """`copies` of every edge length (at most max_len) plus n_empty documents without rows, shuffled: short documents follow long ones
    and the other way round"""
    import torch

    lens = [n for n in lens if max_len is None or n <= max_len] * copies + [0] * n_empty
    return [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]


def far_side_case(seed, q_lens, d_lens, dim, dtype, planted=False):
    """(queries, documents, planted row per document or -1): lists of [n, dim] CPU tensors of `dtype`.  planted=True replaces one row
    of every non-empty document by a row on the queries' side (+0.7 u): the position cycles through planted_positions(n) with the
    document's index, so every position is taken by some document of every length class that has it."""
    import torch

    g = torch.Generator().manual_seed(seed)
    u = far_side_axis(dim, g)
    q_all = far_side_rows(sum(q_lens), u, +1, g, dtype)
    d_all = far_side_rows(max(sum(d_lens), 1), u, -1, g, dtype)[: sum(d_lens)]
    qs = [t.clone() for t in q_all.split(list(q_lens))]
    ps = [t.clone() for t in d_all.split(list(d_lens))]
    rows = [-1] * len(ps)
    if planted:
        for c, p in enumerate(ps):
            if p.shape[0]:
                pos = planted_positions(p.shape[0])
                rows[c] = pos[c % len(pos)]
                p[rows[c]] = far_side_rows(1, u, +1, g, dtype)[0]
    return qs, ps, rows


def maxsim_truth(q_tokens, D, d_off, device="cpu"):
    """float64 per-token truth of include/maxsim.h's contract on a packed corpus: for every token row i of q_tokens [T, dim] and every
    document c (rows d_off[c] .. d_off[c+1]-1 of D): M[i, c] = max_j <q_i, D_j> (-inf for a document without rows), A[i, c] = the first
    row (relative to the document) that attains it (-1 without rows), G[i, c] = M minus the second largest similarity (+inf for
    documents of fewer than two rows).  One product per document, on `device`; the results come back on the CPU."""
    import torch

    Q = torch.as_tensor(q_tokens).to(device).double()
    Dd = torch.as_tensor(D).to(device).double()
    off = [int(x) for x in d_off]
    T, n = Q.shape[0], len(off) - 1
    M = torch.full((T, n), float("-inf"), dtype=torch.float64, device=device)
    A = torch.full((T, n), -1, dtype=torch.int64, device=device)
    G = torch.full((T, n), float("inf"), dtype=torch.float64, device=device)
    for c in range(n):
        a, b = off[c], off[c + 1]
        if b == a:
            continue
        S = Q @ Dd[a:b].T
        top = torch.topk(S, min(2, b - a), dim=1).values
        M[:, c] = top[:, 0]
        A[:, c] = (S == top[:, :1]).to(torch.int8).argmax(dim=1)            # argmax of a 0/1 matrix: the first maximal row
        if b - a > 1:
            G[:, c] = top[:, 0] - top[:, 1]
    return M.cpu(), A.cpu(), G.cpu()


def token_sums(M, q_lens, clamp0=None):
    """scores float64 [n_q, n_d]: the sum over every query's tokens of M[i, c], after max(M, 0) on the documents clamp0 flags (the
    reference's zero padding row: include/maxsim.h, d_clamp0).  An empty document scores -inf, 0 when flagged."""
    import torch

    M = M.clone()
    if clamp0 is not None:
        f = torch.as_tensor(clamp0).bool()
        M[:, f] = M[:, f].clamp_min(0.0)
    out, o = [], 0
    for n in q_lens:
        out.append(M[o : o + int(n)].sum(dim=0))
        o += int(n)
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# Large-offset fixtures (tests/test_gpu_large_offsets.py, tests/test_large_offsets_host.py).  A shard is ONE block of P pages of random
# unit rows (R0 rows in all, R0 odd) repeated T times, so that the truth of the block, tiled, is the truth of the shard, and the shard
# crosses byte 2^31 / 2^32 and element 2^31 / 2^32.  R0 is odd and every wrap distance, taken modulo the block, lies at least one
# longest page away from 0 and from R0: a row index, element offset or byte offset that lost its high bits lands in ANOTHER page of
# the block (other random rows), never on an equal copy.  test_large_offsets_host.py asserts exactly that for the parameters below.

LARGE_EDGE_LENS = [1, 31, 32, 33, 64, 96, 129, 500, 1000, 1030, 0]
LARGE_PAGES = 60
LARGE_SEED = 1
# kind -> (torch dtype name, width, bytes per element, the row count the shard must exceed)
LARGE_SHARDS = {
    "bf16_128": ("bfloat16", 128, 2, 2**25),                 # 8.6 GB: byte 2^31 at row 2^23, byte 2^32 = element 2^31 at 2^24, element 2^32 at 2^25
    "bf16_320": ("bfloat16", 320, 2, 2**32 // 640 + 1),      # 4.3 GB: byte 2^31, byte 2^32 = element 2^31 (no whole row: 2^32 / 640 is no integer)
    "f32_128": ("float32", 128, 4, 2**24),                   # 8.6 GB: byte 2^31 at row 2^22, byte 2^32 at 2^23, element 2^31 at 2^24
}
# score matrices of more than 2^31 entries: n_q rows that repeat a 7-row block; ld = 4 x odd (the vector paths) and ld odd (the scalar ones)
LARGE_MATRIX_ROWS = 2049
LARGE_MATRIX_BLOCK = 7
LARGE_MATRIX_LD = {"vec": 4 * 262145, "odd": 4 * 262145 - 1}


def large_block_lens(seed=LARGE_SEED, n_pages=LARGE_PAGES):
    """The page lengths of the block: every edge length once (an empty page among them) and lengths of 2 .. 300 rows, shuffled; the
    total is odd and greater than 1."""
    rng = np.random.default_rng(seed)
    rand = rng.integers(2, 301, n_pages - len(LARGE_EDGE_LENS)).tolist()
    if (sum(LARGE_EDGE_LENS) + sum(rand)) % 2 == 0:
        rand[0] += 1
    lens = LARGE_EDGE_LENS + rand
    return [int(lens[i]) for i in rng.permutation(n_pages)]


def large_shard_spec(kind):
    """dict: dtype (name), width, row_bytes, elem_bytes, lens, offsets (int64 [P + 1] of the block), R0, P, T, rows, n and `bounds`:
    name -> the first ROW INDEX at or past the boundary, for the boundaries the shard reaches."""
    dtype, width, es, min_rows = LARGE_SHARDS[kind]
    lens = large_block_lens()
    off = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    R0 = int(off[-1])
    T = min_rows // R0 + 2                                  # at least one whole tile past the last boundary
    rb = width * es
    bounds = {}
    for name, nbytes in large_wrap_bytes(es).items():
        row = -(-nbytes // rb)
        if row < T * R0:
            bounds[name] = row
    return dict(kind=kind, dtype=dtype, width=width, elem_bytes=es, row_bytes=rb, lens=lens, offsets=off, R0=R0, P=len(lens), T=T,
                rows=T * R0, n=T * len(lens), bounds=bounds)


def large_wrap_bytes(elem_bytes):
    """name -> the distance in BYTES an address moves when an offset loses bit 31 / 32 as a byte count or as an element count"""
    return {"byte 2^31": 2**31, "byte 2^32": 2**32, "element 2^31": 2**31 * elem_bytes, "element 2^32": 2**32 * elem_bytes}


def large_page_at(spec, byte_addr):
    """the page of the BLOCK that owns byte `byte_addr` of the shard (any tile: the address is taken modulo the block)"""
    row = (int(byte_addr) % (spec["R0"] * spec["row_bytes"])) // spec["row_bytes"]
    return int(np.searchsorted(spec["offsets"], row, side="right")) - 1


def large_tiles_of_interest(spec):
    """sorted tile indices: tile 0, the last tile and, for every boundary the shard reaches, the tile that holds the boundary's row
    with the tile before it and the tile after it"""
    R0, T = spec["R0"], spec["T"]
    tiles = {0, T - 1}
    for row in spec["bounds"].values():
        t = row // R0
        tiles.update(x for x in (t - 1, t, t + 1) if 0 <= x < T)
    return sorted(tiles)


def large_block_rows(spec, seed=LARGE_SEED):
    """the block's rows: random unit rows [R0, width] as a CPU tensor of the shard's dtype, every value one the 13-bit image holds"""
    import torch

    g = torch.Generator().manual_seed(1000 + seed)
    rows = torch.nn.functional.normalize(torch.randn(spec["R0"], spec["width"], generator=g), dim=-1)
    rows = rows.to(getattr(torch, spec["dtype"]))
    rows[rows == 0] = 2.0**-10            # no exact zero: the 13-bit image of the corpus cannot hold one, and the block is to carry no flagged page
    return rows


def large_shard_tensors(spec, block, device):
    """(blob [T * R0, width] on `device`, offsets int32 [n + 1] on `device`, lengths int64 [n] on the host): the block written T
    times with one expanding copy, the block's offsets plus t * R0."""
    import torch

    T, R0, P, w = spec["T"], spec["R0"], spec["P"], spec["width"]
    blob = torch.empty((T * R0, w), dtype=block.dtype, device=device)
    blob.view(T, R0, w).copy_(block.to(device).unsqueeze(0).expand(T, R0, w))
    off = spec["offsets"][None, :-1] + (np.arange(T, dtype=np.int64) * R0)[:, None]
    off = np.concatenate([off.reshape(-1), [T * R0]])
    assert off[-1] < 2**31
    lengths = torch.from_numpy(np.tile(np.asarray(spec["lens"], dtype=np.int64), T))
    return blob, torch.from_numpy(off.astype(np.int32)).to(device), lengths


def large_matrix_block(ld, seed=7):
    """fp32 [7, ld] on the host: random scores drawn from 4096 distinct values (so every row is full of exact ties) with -inf, +0.0
    and -0.0 sprinkled in, and the largest value of a row repeated at both ends and in the middle"""
    rng = np.random.default_rng(seed)
    vals = rng.standard_normal(4096).astype(np.float32)
    blk = vals[rng.integers(0, 4096, (LARGE_MATRIX_BLOCK, ld))]
    kind = rng.integers(0, 64, blk.shape)
    blk[kind == 0] = -np.inf
    blk[kind == 1] = 0.0
    blk[kind == 2] = -0.0
    for r in range(LARGE_MATRIX_BLOCK):
        blk[r, [0, ld // 2 + r, ld - 1]] = np.float32(5.0 + r)
    return blk


def large_matrix_probe_rows(ld, n_q=LARGE_MATRIX_ROWS):
    """the rows checked element by element on the host: the first, the first one wholly past element 2^30 and 2^31, the last"""
    return sorted({0, -(-2**30 // ld), -(-2**31 // ld), n_q - 1})


def large_matrix_group_labels(ld):
    """int64 [ld] document ids: runs of 37 consecutive pages in the first half, pages strided by 1001 in the second (a document's
    pages need not be contiguous); the ids themselves are large and not contiguous"""
    col = np.arange(ld, dtype=np.int64)
    return np.where(col < ld // 2, 10 * (col // 37), 10**12 + col % 1001)


def group_reduce_truth_fast(scores, page_groups, id_base=0):
    """group_truth.reduce_truth, vectorised for a million columns (test_large_offsets_host.py holds the two equal): per document the
    page with the highest score (-0.0 and +0.0 tie, the lower page wins a tie, the winner keeps its bits; all -inf: (-inf, -1))."""
    scores = np.asarray(scores, dtype=np.float32)
    labels = np.asarray(page_groups, dtype=np.int64)
    group_ids, inv = np.unique(labels, return_inverse=True)
    n_q, n = scores.shape
    out_s = np.full((n_q, group_ids.size), -np.inf, dtype=np.float32)
    out_p = np.full((n_q, group_ids.size), -1, dtype=np.int64)
    cols = np.arange(n, dtype=np.int64)
    for q in range(n_q):
        key = scores[q].astype(np.float64) + 0.0                      # folds -0.0 onto +0.0
        order = np.lexsort((cols, -key, inv))                         # by document, then score descending, then page ascending
        first = order[np.concatenate([[True], inv[order][1:] != inv[order][:-1]])]
        win = ~np.isneginf(scores[q, first])
        g = inv[first]
        out_s[q, g[win]] = scores[q, first[win]]
        out_p[q, g[win]] = first[win] + id_base
    return group_ids, out_s, out_p
