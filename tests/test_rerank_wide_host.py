"""The width-320 rerank entry without a GPU: msim_fwd_candidates_wide refuses bad arguments before any device work, its
workspace size, and its place in the ABI.  The wide entry takes dim == 320 only: width 128 stays with msim_fwd_candidates (which
keeps refusing width 320, tests/test_rerank_host.py)."""
import os
import re

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def _call(L, dtype=0, qt=FAKE, q_off=FAKE, q_off_host=None, n_q=2, d=FAKE, d_off=FAKE, n_d=10, dim=320, cand=FAKE, m=4, ld_cand=4,
          out=FAKE, ld=4, flags=0, ws=FAKE):
    oh = np.array([0, 3, 7], dtype=np.int32) if q_off_host is None else np.asarray(q_off_host, dtype=np.int32)
    return L.msim_fwd_candidates_wide(dtype, qt, q_off, oh.ctypes.data, n_q, d, d_off, None, n_d, dim, cand, m, ld_cand, 0, out, ld,
                                      None, flags, ws, None)


def test_wide_candidates_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert _call(L, n_q=0) == 0 and _call(L, m=0) == 0                     # nothing to do: no pointer is looked at
    assert _call(L, n_q=0, qt=None, cand=None, out=None, ws=None) == 0
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(qt=None), dict(q_off=None), dict(d_off=None), dict(cand=None),
               dict(out=None), dict(ws=None), dict(qt=FAKE + 8), dict(d=FAKE + 2), dict(ws=FAKE + 4), dict(ld_cand=3), dict(ld=3),
               dict(flags=0x2), dict(flags=1 << 8), dict(q_off_host=[1, 3, 7]), dict(q_off_host=[0, 5, 3])):
        assert _call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=128), dict(dim=64), dict(dim=96), dict(q_off_host=[0, 3, 3 + 129])):
        assert _call(L, **kw) == EUNSUPPORTED, kw
        assert b"msim_fwd_candidates_wide" in L.msim_last_error()


def test_wide_workspace_size_is_monotone():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_fwd_candidates_wide_workspace_bytes(0, 5, 10, 320) == 0
    assert L.msim_fwd_candidates_wide_workspace_bytes(3, 0, 10, 320) == 0
    assert L.msim_fwd_candidates_wide_workspace_bytes(-1, 5, 10, 320) == 0
    w = L.msim_fwd_candidates_wide_workspace_bytes(1000, 100, 125000, 320)
    assert w % 16 == 0 and w >= 125000 * 8 * 4 + 1000 * 100 * (4 + 8 + 16)
    assert L.msim_fwd_candidates_wide_workspace_bytes(1000, 200, 125000, 320) > w
    assert L.msim_fwd_candidates_wide_workspace_bytes(2000, 100, 125000, 320) > w
    assert L.msim_fwd_candidates_wide_workspace_bytes(1000, 100, 250000, 320) > w
    sizes = [L.msim_fwd_candidates_wide_workspace_bytes(n_q, m, n_d, 320) for n_d in (1, 1000, 50000) for n_q, m in ((1, 1), (4, 100), (100, 100))]
    for n_d_block in (sizes[0:3], sizes[3:6], sizes[6:9]):
        assert n_d_block == sorted(n_d_block) and len(set(n_d_block)) == 3           # grows with n_q * m
    assert sizes[0] < sizes[3] < sizes[6]                                             # grows with n_d


def test_the_wide_entry_is_an_addition_to_abi_22():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert L.msim_abi_version() == 22 and colpali_amd._lib.ABI_VERSION == 22
    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    assert re.search(r"\bsize_t\s+msim_fwd_candidates_wide_workspace_bytes\s*\(\s*int n_q,\s*int m,\s*int n_d,\s*int dim\s*\)\s*;", header)
    assert re.search(r"\bint\s+msim_fwd_candidates_wide\s*\(", header)
    assert re.search(r"\bint\s+msim_fwd_candidates\s*\(", header)                     # the width-128 pair is still there
