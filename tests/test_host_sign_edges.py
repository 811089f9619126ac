"""Sign tier of the HOST scorer (msim_fwd_host / msim_fwd_host_lists, colpali_amd/csrc/maxsim_host.cpp); runs without a GPU.

Contract (include/maxsim.h): scores[q, c] = sum over the tokens i of query q of max over the rows j of document c of <Q_i, D_j>, fp32
products and sums of the exactly widened inputs; a document flagged in d_clamp0 also lets a similarity of exactly 0 take part in
every per-token max; a document without rows is a max over nothing (-inf), 0 when flagged.

The host scorer walks a document eight rows at a time and keeps sixteen query tokens in the lanes of a vector: a short last row
group computes fewer rows, and the lanes past a block's last token hold zero rows.  A zero that reaches a max from either tail
changes a score only where the true per-token maximum is negative, which random unit rows never produce over more than a few
document rows.  The far-side inputs of tests/helpers.py make EVERY similarity negative; each test asserts that on its own float64
truth (every per-token maximum <= -0.05) before it looks at the library's output, so a single leaked zero moves a score by at least
0.05 against a tolerance of 1e-5 * max(|truth|, 1).

Which clone of the scorer runs (AVX-512, AVX2 + FMA or baseline x86-64) is the loader's choice from the CPU's features; the test
prints the one this machine selects.
"""
import numpy as np
import pytest
import torch

import colpali_amd as amd
from tests.helpers import SIGN_MARGIN, far_side_case, maxsim_truth, token_sums

RTOL = 1e-5
CODE = {torch.bfloat16: 0, torch.float16: 1, torch.float32: 2}
# document lengths around the 8-row register block and the 16-lane vector, query lengths around the 16-token vector
D_LENS = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 0, 0]
Q_LENS = [1, 15, 16, 17, 31, 32, 33, 5]


def selected_clone():
    """the clone target_clones("avx512f", "avx2,fma", "default") resolves to on this CPU"""
    flags = set()
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("flags"):
                    flags = set(line.split(":", 1)[1].split())
                    break
    except OSError:
        return "unknown (no /proc/cpuinfo)"
    if "avx512f" in flags:
        return "AVX-512"
    if "avx2" in flags and "fma" in flags:
        return "AVX2 + FMA"
    return "baseline x86-64"


def _bits(t):
    return t.contiguous().view(torch.int32).numpy()


def _host_packed(qs, ps, clamp, dtype, dim, threads=4):
    """msim_fwd_host: the queries as a zero-padded box, the documents as one packed blob"""
    L = amd._lib.lib()
    lq = max(q.shape[0] for q in qs)
    box = torch.zeros((len(qs), lq, dim), dtype=dtype)
    for i, q in enumerate(qs):
        box[i, : q.shape[0]] = q
    blob = torch.cat(ps + [torch.zeros(1, dim, dtype=dtype)]).contiguous()
    off = np.zeros(len(ps) + 1, dtype=np.int32)
    np.cumsum([p.shape[0] for p in ps], out=off[1:])
    out = torch.full((len(qs), len(ps)), 7.0, dtype=torch.float32)
    rc = L.msim_fwd_host(CODE[dtype], box.data_ptr(), len(qs), lq, blob.data_ptr(), off.ctypes.data,
                         clamp.ctypes.data if clamp is not None else None, len(ps), dim, out.data_ptr(), len(ps), 0, threads)
    assert rc == 0, L.msim_host_last_error()
    return out


def _host_lists(qs, ps, clamp, dtype, dim, threads=4):
    """msim_fwd_host_lists: the caller's tensors as they are, ragged queries at their real lengths"""
    L = amd._lib.lib()
    keep = [t.contiguous() for t in qs + ps]
    spare = torch.zeros(1, dim, dtype=dtype)                      # a valid address for documents without rows
    q_ptr = np.asarray([t.data_ptr() for t in keep[: len(qs)]], dtype=np.uint64)
    d_ptr = np.asarray([t.data_ptr() if t.shape[0] else spare.data_ptr() for t in keep[len(qs):]], dtype=np.uint64)
    q_rows = np.asarray([q.shape[0] for q in qs], dtype=np.int64)
    d_rows = np.asarray([p.shape[0] for p in ps], dtype=np.int64)
    out = torch.full((len(qs), len(ps)), 7.0, dtype=torch.float32)
    rc = L.msim_fwd_host_lists(CODE[dtype], q_ptr.ctypes.data, q_rows.ctypes.data, len(qs), d_ptr.ctypes.data, d_rows.ctypes.data,
                               clamp.ctypes.data if clamp is not None else None, len(ps), dim, out.data_ptr(), len(ps), 0, threads)
    assert rc == 0, L.msim_host_last_error()
    return out


def _close(got, want):
    got, want = got.double(), want.double()
    fin = torch.isfinite(want)
    assert torch.equal(got[~fin], want[~fin]), "documents without rows"
    err = float(((got[fin] - want[fin]).abs() / want[fin].abs().clamp_min(1.0)).max())
    print(f"    largest error {err:.3e} (tolerance {RTOL:.0e})")
    assert err <= RTOL


@pytest.mark.parametrize("entry", [_host_packed, _host_lists], ids=["msim_fwd_host", "msim_fwd_host_lists"])
@pytest.mark.parametrize("dim", [32, 128, 320])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "fp16", "fp32"])
def test_host_scorer_on_all_negative_and_planted_documents(entry, dtype, dim):
    print(f"host clone selected on this CPU: {selected_clone()}")
    n_d = len(D_LENS)
    g = torch.Generator().manual_seed(900 + dim)
    d_lens = [D_LENS[i] for i in torch.randperm(n_d, generator=g).tolist()]
    flags = (torch.rand(n_d, generator=g) < 0.5).numpy().astype(np.uint8)
    flags[[i for i, n in enumerate(d_lens) if n == 0][0]] = 1               # at least one empty document with and one without the flag
    flags[[i for i, n in enumerate(d_lens) if n == 0][1]] = 0
    empty = torch.tensor([n == 0 for n in d_lens])
    f = torch.from_numpy(flags).bool()
    for planted in (False, True):
        qs, ps, rows = far_side_case(7000 + dim + planted, Q_LENS, d_lens, dim, dtype, planted=planted)
        off = np.concatenate([[0], np.cumsum(d_lens)])
        M, A, _ = maxsim_truth(torch.cat(qs), torch.cat(ps), off)
        live = M[:, ~empty]
        if planted:        # the planted row wins every token's max, well above 0
            assert float(live.min()) >= SIGN_MARGIN and torch.equal(A[:, ~empty], torch.tensor(rows)[~empty].expand(M.shape[0], -1))
        else:              # PRECONDITION on the inputs: every per-token maximum is negative by the margin
            assert float(live.max()) <= -SIGN_MARGIN, float(live.max())
        # 1. truth
        base = entry(qs, ps, None, dtype, dim)
        _close(base, token_sums(M, Q_LENS))
        assert bool(torch.isneginf(base[:, empty]).all())                   # 5. a max over nothing
        # 2. clamp0 on a random half of the documents
        clamped = entry(qs, ps, flags, dtype, dim)
        _close(clamped, token_sums(M, Q_LENS, flags))
        assert np.array_equal(_bits(clamped[:, ~f]), _bits(base[:, ~f]))    # an unflagged document keeps its bits
        assert bool((clamped[:, f & empty] == 0).all())                     # 5. the zero padding row alone
        if planted:
            assert np.array_equal(_bits(clamped[:, ~empty]), _bits(base[:, ~empty]))        # the flags change no bit
        else:
            assert bool((clamped[:, f] == 0).all())                         # a flagged document scores exactly 0
        # thread count and entry point change no bit
        assert np.array_equal(_bits(entry(qs, ps, flags, dtype, dim, threads=1)), _bits(clamped))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_host_scores_do_not_depend_on_the_neighbours(dtype):
    """3. placement: a permuted corpus gives the permuted scores bit for bit, through both entry points, which agree with each other."""
    dim = 128
    g = torch.Generator().manual_seed(31)
    qs, ps, _ = far_side_case(7100, Q_LENS, D_LENS, dim, dtype)
    perm = torch.randperm(len(ps), generator=g).tolist()
    a = _host_packed(qs, ps, None, dtype, dim)
    b = _host_packed(qs, [ps[i] for i in perm], None, dtype, dim)
    assert np.array_equal(_bits(b), _bits(a[:, perm]))
    c = _host_lists(qs, [ps[i] for i in perm], None, dtype, dim)
    assert np.array_equal(_bits(c), _bits(b))
