"""`device="cpu"` through the reference's own signature: the library's host-core scorer (msim_fwd_host / msim_sim_matrix_host,
colpali_amd/csrc/maxsim_host.cpp) against the live reference's golden outputs and the oracle.  The reference computes on whatever
device it is given (processing_utils.py:161, :172-179; torch_utils.py:12-31 answers "cpu" on a host without an accelerator), so a
CPU request must WORK -- BASELINE config 1 reads "score_multi_vector on CPU".  Runs without a GPU.

Tolerance: |got - truth| <= 1e-5 * max(|truth|, 1); literal tier within one bf16 ulp of the live reference's bf16 CPU output."""
import os

import numpy as np
import pytest
import torch

import colpali_amd as amd
from oracle import maxsim_oracle as mo
from tests.conftest import load_golden
from tests.helpers import config1_inputs, ragged_from_golden, run_contract_checks

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
RTOL = 1e-5


def close(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= RTOL


def bits_to_bf16(bits):
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def test_config1_on_cpu_truth_and_literal(monkeypatch):
    """BASELINE config 1 as written: 4 queries x 16 docs, bf16 [32,128] x [1024,128], device='cpu'."""
    z = load_golden("score_config1.npz")
    qs, ps = config1_inputs(z)
    got = amd.score_multi_vector(qs, ps, device="cpu")
    assert got.device.type == "cpu" and got.dtype == torch.float32 and got.shape == (4, 16)
    assert close(got.numpy(), z["truth"])
    monkeypatch.setenv("COLPALI_AMD_REF_ROUNDING", "1")
    lit = amd.score_multi_vector(qs, ps, device="cpu").numpy()
    ulp = 2.0 ** (np.floor(np.log2(np.abs(z["literal"]))) - 7)
    assert np.all(np.abs(lit - z["literal"]) <= ulp) and np.mean(lit == z["literal"]) > 0.9


def test_ragged_golden_all_block_sizes_on_cpu():
    z = load_golden("score_ragged_d128.npz")
    qs, ps = ragged_from_golden(z)
    qs, ps = [bits_to_bf16(q) for q in qs], [bits_to_bf16(p) for p in ps]
    for bs in z["batch_sizes"]:
        got = amd.score_multi_vector(qs, ps, batch_size=int(bs), device="cpu")
        assert close(got.numpy(), z[f"truth_bs{bs}"]), f"batch_size={bs}"


def test_negative_similarities_and_zero_padding_on_cpu():
    z = load_golden("score_negative_clamp.npz")
    q, short, long_ = (bits_to_bf16(z[k]) for k in ("q_bits", "short_bits", "long_bits"))
    assert close(amd.score_multi_vector([q], [short], device="cpu").numpy(), z["truth_alone"])
    assert close(amd.score_multi_vector([q], [short, long_], device="cpu").numpy(), z["truth_block"])
    assert close(amd.score_multi_vector([q], [short, long_], batch_size=1, device="cpu").numpy(), z["truth_split"])


def test_tensor3d_inputs_on_cpu():
    z = load_golden("score_tensor3d.npz")
    q = bits_to_bf16(z["q_bits"]).reshape(*z["q_shape"])
    p = bits_to_bf16(z["p_bits"]).reshape(*z["p_shape"])
    assert close(amd.score_multi_vector(q, p, device="cpu").numpy(), z["truth"])


@pytest.mark.parametrize("dtype,dim", [(torch.float32, 32), (torch.float16, 128), (torch.bfloat16, 320), (torch.float32, 5)])
def test_every_dtype_and_width_against_the_oracle_on_cpu(dtype, dim):
    g = torch.Generator().manual_seed(dim)
    qs = [torch.randn(n, dim, generator=g).to(dtype) for n in (1, 7, 33, 40)]
    ps = [torch.randn(n, dim, generator=g).to(dtype) for n in (1, 15, 16, 17, 100, 31, 64)]
    want = mo.score_multi_vector([q.float().numpy() for q in qs], [p.float().numpy() for p in ps], batch_size=3)
    got = amd.score_multi_vector(qs, ps, batch_size=3, device="cpu").numpy()
    assert np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)) <= 2e-5 * max(1.0, dim / 32)   # unnormalised rows: sums of dim products


def test_errors_keep_the_reference_contract_on_cpu():
    with pytest.raises(ValueError, match="No queries"):
        amd.score_multi_vector([], [torch.zeros(2, 8)], device="cpu")
    with pytest.raises(ValueError, match="No passages"):
        amd.score_multi_vector([torch.zeros(2, 8)], [], device="cpu")
    with pytest.raises(RuntimeError):
        amd.score_multi_vector([torch.zeros(2, 8)], [torch.zeros(2, 8, dtype=torch.bfloat16)], device="cpu")


def test_single_vector_scores_on_cpu():
    g = torch.Generator().manual_seed(3)
    qs, ps = [torch.randn(32, generator=g) for _ in range(4)], [torch.randn(32, generator=g) for _ in range(19)]
    got = amd.score_single_vector(qs, ps, device="cpu")
    assert got.shape == (4, 19) and got.dtype == torch.float32
    assert torch.allclose(got, torch.stack(qs) @ torch.stack(ps).T, atol=1e-5)


def test_packed_and_list_entry_points_agree_bit_for_bit():
    """msim_fwd_host (box + packed blob, the layout of the GPU entry points) and msim_fwd_host_lists (the caller's tensors as they are)
    are one implementation: equal queries give equal bits; zero padding rows of a box add exactly 0."""
    L = amd._lib.lib()
    g = torch.Generator().manual_seed(4)
    qs = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in (32, 32, 32)]
    ps = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in (40, 1, 17, 300, 8)]
    want = amd.score_multi_vector(qs, ps, batch_size=2, device="cpu")
    box = torch.stack(qs).contiguous()
    blob = torch.cat(ps).contiguous()
    off = np.zeros(len(ps) + 1, dtype=np.int32)
    np.cumsum([p.shape[0] for p in ps], out=off[1:])
    clamp0 = np.asarray([1, 1, 1, 0, 0], dtype=np.uint8)        # blocks of two: (40, 1) -> the 1-row page is padded; (17, 300); (8) alone
    clamp0[0] = 0
    out = torch.empty((3, len(ps)), dtype=torch.float32)
    rc = L.msim_fwd_host(0, box.data_ptr(), 3, 32, blob.data_ptr(), off.ctypes.data, clamp0.ctypes.data, len(ps), 128, out.data_ptr(),
                         len(ps), 0, 4)
    assert rc == 0 and torch.equal(out, want)
    assert L.msim_fwd_host(0, box.data_ptr(), 3, 32, blob.data_ptr(), off.ctypes.data, None, len(ps), 128, out.data_ptr(), 2, 0, 4) == -1
    assert L.msim_fwd_host(5, box.data_ptr(), 3, 32, blob.data_ptr(), off.ctypes.data, None, len(ps), 128, out.data_ptr(), len(ps), 0, 4) == -2
    assert b"bfloat16" in L.msim_host_last_error()


def test_results_do_not_depend_on_the_thread_count(monkeypatch):
    g = torch.Generator().manual_seed(8)
    qs = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in (32, 12, 40)]
    ps = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in torch.randint(1, 300, (200,), generator=g).tolist()]
    outs = []
    for nt in ("1", "3", "16"):
        monkeypatch.setenv("COLPALI_AMD_HOST_THREADS", nt)
        outs.append(amd.score_multi_vector(qs, ps, device="cpu"))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_concurrent_callers_share_the_thread_pool_without_deadlock():
    """One parallel region at a time: a second caller scores on its own thread instead of waiting for the pool (ctypes releases the
    GIL inside the call, so python threads really overlap).  Same bits as a lone call."""
    import threading

    g = torch.Generator().manual_seed(12)
    qs = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in (32, 20, 40, 12)]
    ps = [torch.randn(n, 128, generator=g).to(torch.bfloat16) for n in torch.randint(50, 400, (120,), generator=g).tolist()]
    want = amd.score_multi_vector(qs, ps, device="cpu")
    got, errs = [None] * 6, []

    def work(i):
        try:
            for _ in range(3):
                got[i] = amd.score_multi_vector(qs, ps, device="cpu")
        except Exception as e:      # pragma: no cover
            errs.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(6)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not errs and all(not th.is_alive() for th in threads)
    assert all(torch.equal(x, want) for x in got)


def test_the_reference_scorer_tests_pass_on_a_host_without_a_gpu():
    """tests/reference_suite/contract_checks.py's scorer checks in a subprocess that sees NO GPU: `device` defaults to
    get_torch_device("auto") = "cpu" there, and both scorers must work (round-3 review: the patched package used to raise)."""
    out = run_contract_checks("scorer", "cpu", HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    assert "2 passed" in out, out


def test_host_gather_range_copies_any_byte_range_of_the_virtual_concatenation():
    """msim_host_gather_range (the upload path's gather: bytes [lo, hi) of the concatenation of the caller's page tensors into one half
    of the pinned staging buffer, equal byte shares over a persistent pool): any range, any thread count, empty buffers in between."""
    import ctypes

    import numpy as np

    from colpali_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(3)
    sizes = [int(x) for x in rng.integers(0, 300_000, size=57)]
    sizes[5] = sizes[20] = 0
    sizes[33] = 9_000_001                               # one buffer larger than several shares
    bufs = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in sizes]
    whole = np.concatenate(bufs)
    srcs = np.asarray([b.ctypes.data if b.size else 0 for b in bufs], dtype=np.uint64)
    prefix = np.zeros(len(bufs) + 1, dtype=np.int64)
    np.cumsum(sizes, out=prefix[1:])
    total = int(prefix[-1])
    for lo, hi in ((0, total), (1, total - 1), (123_457, 5_000_000), (total - 10, total), (prefix[33] + 17, prefix[34] - 5), (40, 40)):
        lo, hi = int(lo), int(hi)
        for threads in (1, 3, 8, 64):
            dst = np.full(hi - lo + 16, 0xAB, dtype=np.uint8)
            rc = L.msim_host_gather_range(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), lo, hi, threads)
            assert rc == 0
            assert np.array_equal(dst[: hi - lo], whole[lo:hi]) and (dst[hi - lo:] == 0xAB).all()
    dst = np.zeros(16, dtype=np.uint8)
    assert L.msim_host_gather_range(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), 0, total + 1, 2) == -1
    assert L.msim_host_gather_range(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), 5, 4, 2) == -1


def test_host_gather_range_begin_wait_is_the_same_copy_on_a_native_thread():
    """msim_host_gather_range_begin / _wait (round 6: the upload path gathers chunk k + 1 while the Python thread issues chunk k's copy
    and launches): same bytes as the blocking call, one request in flight, failures reported by `wait`."""
    import numpy as np

    from colpali_amd import _lib

    L = _lib.lib()
    rng = np.random.default_rng(4)
    sizes = [int(x) for x in rng.integers(1, 400_000, size=41)]
    bufs = [rng.integers(0, 256, size=n, dtype=np.uint8) for n in sizes]
    whole = np.concatenate(bufs)
    srcs = np.asarray([b.ctypes.data for b in bufs], dtype=np.uint64)
    prefix = np.zeros(len(bufs) + 1, dtype=np.int64)
    np.cumsum(sizes, out=prefix[1:])
    total = int(prefix[-1])
    assert L.msim_host_gather_range_wait() == -1 and b"no gather in flight" in L.msim_host_last_error()
    for rep in range(20):                                 # back-to-back requests through the one driver thread
        lo = (rep * 7919) % (total // 2)
        hi = min(total, lo + 1 + (rep * 104729) % (total // 2))
        dst = np.full(hi - lo + 8, 0xCD, dtype=np.uint8)
        assert L.msim_host_gather_range_begin(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), lo, hi, 4) == 0
        if rep == 0:                                      # a second request before the wait is refused, the first one is unharmed
            assert L.msim_host_gather_range_begin(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), lo, hi, 4) == -1
        assert L.msim_host_gather_range_wait() == 0
        assert np.array_equal(dst[: hi - lo], whole[lo:hi]) and (dst[hi - lo:] == 0xCD).all()
    dst = np.zeros(16, dtype=np.uint8)
    assert L.msim_host_gather_range_begin(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, len(bufs), 0, total + 1, 2) == 0
    assert L.msim_host_gather_range_wait() == -1 and b"range beyond the image" in L.msim_host_last_error()
    assert L.msim_host_gather_range_wait() == -1          # nothing left in flight


def test_host_threads_affinity_and_the_page_node_query():
    """msim_host_threads_affinity moves the library's host threads (present and future) onto a CPU list and the gather still copies
    the same bytes; _lib.nodes_of_addresses (move_pages with a NULL node list) names a node for touched pages or returns []."""
    import ctypes
    import os

    import numpy as np

    from colpali_amd import _lib

    L = _lib.lib()
    assert L.msim_host_threads_affinity(None, 0) == -1
    bad = (ctypes.c_int32 * 1)(1 << 20)
    assert L.msim_host_threads_affinity(bad, 1) == -1 and b"out of range" in L.msim_host_last_error()
    allowed = sorted(os.sched_getaffinity(0))
    rng = np.random.default_rng(5)
    bufs = [rng.integers(0, 256, size=3_000_000, dtype=np.uint8) for _ in range(4)]
    whole = np.concatenate(bufs)
    srcs = np.asarray([b.ctypes.data for b in bufs], dtype=np.uint64)
    prefix = np.arange(5, dtype=np.int64) * 3_000_000
    for cpus in (allowed[:1], allowed[-2:], allowed):
        arr = (ctypes.c_int32 * len(cpus))(*cpus)
        assert L.msim_host_threads_affinity(arr, len(cpus)) == 0
        dst = np.zeros(whole.size, dtype=np.uint8)
        assert L.msim_host_gather_range_begin(dst.ctypes.data, srcs.ctypes.data, prefix.ctypes.data, 4, 0, whole.size, 4) == 0
        assert L.msim_host_gather_range_wait() == 0
        assert np.array_equal(dst, whole)
    nodes = _lib.nodes_of_addresses([b.ctypes.data for b in bufs])
    assert nodes == [] or (len(nodes) == 4 and all(n >= 0 for n in nodes))


def test_thread_counts_follow_what_the_container_grants():
    """_lib.effective_cpus(): affinity and cgroup CPU quota, never more than the host reports (a GPU box shows 256 CPUs and grants 16:
    native thread counts taken from the host's count ran the quota dry and froze the process -- profiles/r05_logs/dropin_stalls.log)."""
    import os

    from colpali_amd import _lib, corpus, scoring

    n = _lib.effective_cpus()
    assert 1 <= n <= (os.cpu_count() or 1)
    assert n <= len(os.sched_getaffinity(0))
    assert 1 <= corpus._COPY_THREADS <= max(1, n // 2) or corpus._COPY_THREADS == 1
    assert scoring._host_threads() <= max(n, int(os.environ.get("COLPALI_AMD_HOST_THREADS", "0")))
