"""Every corpus kernel on a shard past the 32-bit offset boundaries.

The fixtures (tests/helpers.py, "Large-offset fixtures") are ONE block of 60 pages of random unit rows -- R0 = 10067 rows, page
lengths 0, 1, 31, 32, 33, 64, 96, 129, 500, 1000, 1030 and 2 .. 300 -- written T times back to back:

    kind       rows         bytes    boundaries crossed (as a row index)
    bf16_128   33 573 445   8.6 GB   byte 2^31 (row 2^23), byte 2^32 = element 2^31 (row 2^24), element 2^32 (row 2^25)
    bf16_320    6 724 756   4.3 GB   byte 2^31, byte 2^32 = element 2^31 (row 6 710 887)
    f32_128    16 791 756   8.6 GB   byte 2^31 (row 2^22), byte 2^32 (row 2^23), element 2^31 (row 2^24)

and fp32 score matrices of 2049 rows x 1 048 580 (4 x odd: the vector paths) or 1 048 579 (odd: the scalar paths) columns, 8.6 GB,
which repeat a 7-row block and cross element 2^30 (byte 2^32) and element 2^31.  tests/test_large_offsets_host.py proves on the CPU
that no wrap of an offset by 2^31 or 2^32, in bytes or in elements, lands on an equal copy of the data.

The reference is never the code under test: the CPU truths of the suite (helpers.maxsim_truth, the *_truth modules, oracle.topk_oracle)
on the BLOCK alone, tiled T times, compared on the device with the tolerance the kernel's own parity test uses (`close` of
test_gpu_parity for scores, bit equality for ids, gathered rows, decoded rows, codes and masks).  Each test also asserts translation
invariance: the result for page p + t * P carries the bits of the result for page p (MaxSim of a page does not depend on where the
page lies), and a failure names the first tile that differs and the boundary it follows.  Output buffers the API lets the caller
pass are prefilled with NaN / -1.  Each scan asserts the kernel family that ran (msim_fwd_plan, the presence of the 13-bit image,
the dispatch rule of maxsim_abi.hip for width 320).

Out of scope, by size: the 2-bit residual array of the large shard is 1.1 GB (34 bytes per row) and does not reach its own 2^31
boundary; element 2^32 of a score matrix needs 17 GB.  Peak device memory of the module stays under 24 GB: one large object at a
time (`_shard` / `_release`), the module skips -- and says so -- where the device has less free memory.
"""
import time

import numpy as np
import pytest
import torch

from tests import helpers as h

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NEED_BYTES = 24 << 30
RTOL = 1e-5                                    # test_gpu_parity.close
NEG_INF = -float("inf")


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    assert torch.cuda.is_available()
    colpali_amd._lib.lib()  # must load: no fallback
    return colpali_amd


_STATE = {}
_PEAK = [0]


def _release():
    _STATE.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _budget():
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(DEV)
    if free < NEED_BYTES:
        pytest.skip(f"the large-offset module needs {NEED_BYTES >> 30} GB of free device memory, the device reports {free / 2**30:.1f} GB")
    t0 = time.perf_counter()
    yield
    _release()
    peak = _PEAK[0]
    print(f"\nlarge-offset module: peak device memory {peak / 1e9:.2f} GB (torch allocator), {time.perf_counter() - t0:.1f} s")
    assert peak <= NEED_BYTES


@pytest.fixture(autouse=True)
def _report(request):
    """wall time and peak device memory of every test (printed: reported, not gated)"""
    torch.cuda.synchronize(DEV)
    torch.cuda.reset_peak_memory_stats(DEV)
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize(DEV)
    peak = torch.cuda.max_memory_allocated(DEV)
    _PEAK[0] = max(_PEAK[0], peak)
    print(f"    [{request.node.name}] {time.perf_counter() - t0:.2f} s, peak device memory {peak / 1e9:.2f} GB")


def _shard(amd, kind):
    """the tiled shard of `kind`, built on first use; any other large object is released first"""
    if _STATE.get("kind") != kind:
        _release()
        spec = h.large_shard_spec(kind)
        block = h.large_block_rows(spec)
        blob, off, lengths = h.large_shard_tensors(spec, block, DEV)
        _STATE.update(kind=kind, spec=spec, block=block, corpus=amd.PackedCorpus(blob, off, None, lengths))
    s = _STATE
    assert s["corpus"].blob.numel() * s["corpus"].blob.element_size() > 2**32
    return s["spec"], s["block"], s["corpus"]


# ------------------------------------------------------------------------------------------------------------------- shared checks
def _boundary_before(spec, tile):
    """the name of the last boundary at or below the first row of `tile` (what a failure in that tile follows)"""
    below = [(row, name) for name, row in spec["bounds"].items() if row < (tile + 1) * spec["R0"]]
    return max(below)[1] if below else "none"


def _same_bits(a, b):
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


def _assert_tiles_repeat(spec, got, what, skip_cols=()):
    """got [n_q, T * P] (device, 4-byte entries): every tile carries the bits of tile 0"""
    T, P = spec["T"], spec["P"]
    n_q = got.shape[0]
    assert got.shape == (n_q, T * P)
    same = _same_bits(got.view(n_q, T, P), got[:, :P].unsqueeze(1).expand(n_q, T, P))
    for c in skip_cols:
        same.view(n_q, T * P)[:, c] = True
    bad = (~same.all(dim=2).all(dim=0)).nonzero()
    if bad.numel():
        t = int(bad[0])
        cols = (~same[:, t].all(dim=0)).nonzero().flatten().tolist()
        raise AssertionError(f"{what}: tile {t} (rows from {t * spec['R0']}) differs from tile 0 at pages {cols[:8]}; "
                             f"first boundary below it: {_boundary_before(spec, t)}; {int(bad.numel())} tiles differ")


def _assert_close_tile0(got0, want, what):
    """got0 fp32 [n_q, P] against the float64 truth: `close` of test_gpu_parity on the pages that have rows, -inf on the empty one"""
    got0 = got0.double().cpu().numpy()
    want = np.asarray(want, dtype=np.float64)
    empty = np.isneginf(want)
    assert empty.any() and np.array_equal(np.isneginf(got0), empty), what + ": the empty page must score -inf, no other"
    err = np.abs(got0[~empty] - want[~empty]) / np.maximum(np.abs(want[~empty]), 1.0)
    print(f"    {what}: max error vs the float64 truth {err.max():.2e}")
    assert not np.isnan(got0).any() and err.max() <= RTOL, what


def _plan(amd, q_lens):
    out = np.zeros(5, dtype=np.int32)
    off = np.zeros(len(q_lens) + 1, dtype=np.int32)
    np.cumsum(q_lens, out=off[1:])
    assert amd._lib.lib().msim_fwd_plan(off.ctypes.data, len(q_lens), 0, out.ctypes.data) == 0
    return tuple(int(x) for x in out)


def _wide_family(q_lens):
    """maxsim_abi.hip, msim_fwd_ragged at width 320: queries of one length and at most four 32-token tiles in all -> K1sP, else K1bPF"""
    tiles = len(q_lens) * ((q_lens[0] + 31) // 32)
    return "K1sP" if len(set(q_lens)) == 1 and tiles <= 4 else "K1bPF"


_TRUTH = {}


def _queries_and_truth(spec, block, q_lens, seed):
    """(list of [len, width] CPU query tensors of the shard's dtype, float64 [n_q, P] MaxSim truth of the block); computed once"""
    key = (spec["kind"], tuple(q_lens), seed)
    if key not in _TRUTH:
        g = torch.Generator().manual_seed(seed)
        rows = torch.nn.functional.normalize(torch.randn(sum(q_lens), spec["width"], generator=g), dim=-1).to(block.dtype)
        M, _A, _G = h.maxsim_truth(rows.double(), block.double(), spec["offsets"])
        _TRUTH[key] = ([t.clone() for t in rows.split(list(q_lens))], h.token_sums(M, q_lens).numpy())
    return _TRUTH[key]


def _scan(amd, corpus, qs, prefill=float("nan")):
    pq = amd.pack_queries(qs, DEV, layout="auto", compact=False)
    out = torch.full((len(qs), len(corpus)), prefill, dtype=torch.float32, device=DEV)
    got = amd.maxsim_scores(pq, corpus, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got


def _check_scan(amd, kind, q_lens, seed, what, skip_cols=(), extra=None):
    spec, block, corpus = _shard(amd, kind)
    qs, want = _queries_and_truth(spec, block, q_lens, seed)
    got = _scan(amd, corpus, qs)
    _assert_close_tile0(got[:, :spec["P"]], want, what)
    _assert_tiles_repeat(spec, got, what, skip_cols)
    return spec, corpus, qs, want, got


# ------------------------------------------------------------------------------------------------------ full scans, bf16 width 128
@pytest.mark.parametrize("q_lens", [[32] * 4, [16]], ids=["4x32", "1x16"])
def test_scan_k1s(amd, q_lens, monkeypatch):
    monkeypatch.setenv("COLPALI_AMD_PACK13", "0")
    assert _plan(amd, q_lens)[0] == 0, "not the K1s plan"
    _spec, corpus, *_ = _check_scan(amd, "bf16_128", q_lens, 11, f"K1s {len(q_lens)} x {q_lens[0]}")
    assert corpus._pack13 is None
    print("    kernel family: K1s (msim_fwd_plan kernel 0, no 13-bit image)")


@pytest.mark.parametrize("n_q", [16, 40])
def test_scan_k1b(amd, n_q):
    q_lens = [32 - (i % 5) for i in range(n_q)]
    plan = _plan(amd, q_lens)
    assert plan[0] == 1, "not the K1b plan"
    _check_scan(amd, "bf16_128", q_lens, 12, f"K1b {n_q} queries")
    print(f"    kernel family: K1b (msim_fwd_plan {plan})")


def test_scan_k1s13_and_pack13_round_trip(amd, monkeypatch):
    """K1s over the 13-bit image (7.7 GB: slab offsets cross 2^32 bytes too), two flagged pages past rows 2^24 and 2^25 (the
    list-driven launch scores them from the blob), then encode -> decode against the block, bit for bit, on the device."""
    monkeypatch.delenv("COLPALI_AMD_PACK13", raising=False)
    spec, block, corpus = _shard(amd, "bf16_128")
    P, R0, T = spec["P"], spec["R0"], spec["T"]
    off = spec["offsets"]
    # the flagged pages: page 7 (or the next page with rows) of the first tile wholly past row 2^24, and of the last tile
    p_flag = next(p for p in range(7, P) if spec["lens"][p] >= 2)
    tiles = [spec["bounds"]["element 2^31"] // R0 + 1, T - 1]
    assert tiles[0] * R0 >= 2**24 and tiles[1] * R0 >= 2**25
    flagged = [t * P + p_flag for t in tiles]
    rows = [t * R0 + int(off[p_flag]) + 1 for t in tiles]                   # its second row, column 5: an exact zero
    saved = [corpus.blob[r, 5].clone() for r in rows]
    try:
        for r in rows:
            corpus.blob[r, 5] = 0.0
        assert corpus.pack13() and corpus._pack13 is not None
        img = corpus._pack13
        assert img.image.numel() > 2**32 and img.n_flagged == 2 and img.ids.cpu().tolist() == flagged
        want_flags = torch.zeros(len(corpus), dtype=torch.uint8, device=DEV)
        want_flags[flagged] = 1
        assert torch.equal(img.flagged, want_flags)
        planted = block[int(off[p_flag]):int(off[p_flag + 1])].clone()
        planted[1, 5] = 0.0
        for q_lens in ([32] * 4, [16]):
            assert _plan(amd, q_lens)[0] == 0, "not the K1s plan"
            qs, want = _queries_and_truth(spec, block, q_lens, 11)
            got = _scan(amd, corpus, qs)
            assert corpus._pack13 is img, "the scan dropped the image"
            what = f"K1s13 {len(q_lens)} x {q_lens[0]}"
            _assert_close_tile0(got[:, :P], want, what)
            _assert_tiles_repeat(spec, got, what, skip_cols=flagged)
            M, _A, _G = h.maxsim_truth(torch.cat(qs).double(), planted.double(), [0, planted.shape[0]])
            want_f = h.token_sums(M, q_lens).numpy()[:, 0]
            for c in flagged:
                g = got[:, c].double().cpu().numpy()
                assert np.all(np.abs(g - want_f) <= RTOL * np.maximum(np.abs(want_f), 1.0)), (what, "flagged page", c)
        print("    kernel family: K1s13 (msim_fwd_plan kernel 0, the corpus holds a 13-bit image, 2 flagged pages on the list launch)")
        # the round trip: drop the blob (the image, the decoded rows and the blob together would pass 24 GB), decode, compare to the block
        image, slab_off, n_slabs, offsets, n = img.image, img.slab_off, img.n_slabs, corpus.offsets, len(corpus)
        shape = tuple(corpus.blob.shape)
        del img, corpus
        _release()
        out = torch.zeros(shape, dtype=torch.bfloat16, device=DEV)
        L = amd._lib
        L.check(L.lib().msim_pack13_decode(L.ptr(image), L.ptr(offsets), L.ptr(slab_off), n, n_slabs, L.ptr(out),
                                           L.current_stream_handle(DEV)), "msim_pack13_decode")
        blk = block.to(DEV).view(torch.int16)
        same = (out.view(torch.int16).view(T, R0, 128) == blk.unsqueeze(0)).all(dim=2)       # [T, R0]
        for t in tiles:                                                                          # flagged: whatever its codes decode to
            same[t, int(off[p_flag]):int(off[p_flag + 1])] = True
        bad = (~same.all(dim=1)).nonzero()
        assert bad.numel() == 0, (f"pack13 round trip: tile {int(bad[0])} differs from the block; first boundary below it: "
                                  f"{_boundary_before(spec, int(bad[0]))}")
        saved = []
    finally:
        if _STATE.get("kind") == "bf16_128":                                                     # a failure before the release
            for r, v in zip(rows, saved):
                _STATE["corpus"].blob[r, 5] = v
            _STATE["corpus"].drop_pack13()


# ---------------------------------------------------------------------------------------------------------------- lists of pages
def _list_ids(spec):
    """int64 [m] global ids: every page of every tile of interest (tile 0 first), then -1, the very last page and page 3 again"""
    P = spec["P"]
    tiles = h.large_tiles_of_interest(spec)
    ids = np.concatenate([t * P + np.arange(P, dtype=np.int64) for t in tiles])
    return tiles, np.concatenate([ids, [-1, spec["n"] - 1, 3]])


def _check_rerank(amd, kind, q_lens, seed, what):
    spec, block, corpus = _shard(amd, kind)
    P = spec["P"]
    qs, want = _queries_and_truth(spec, block, q_lens, seed)
    tiles, ids = _list_ids(spec)
    n_q, m = len(qs), len(ids)
    cand = torch.from_numpy(np.tile(ids, (n_q, 1))).to(DEV)
    out = torch.full((n_q, m), float("nan"), dtype=torch.float32, device=DEV)
    got, got_ids = amd.retrieval.rerank_scores(amd.pack_queries(qs, DEV, compact=False), corpus, cand, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got_ids, cand)
    _assert_close_tile0(got[:, :P], want, what)
    body = got[:, :len(tiles) * P].view(n_q, len(tiles), P)
    same = _same_bits(body, got[:, :P].unsqueeze(1).expand_as(body)).all(dim=2).all(dim=0).cpu().tolist()
    for t, ok in zip(tiles, same):
        assert ok, f"{what}: the pages of tile {t} differ from tile 0; first boundary below it: {_boundary_before(spec, t)}"
    tail = got[:, -3:].cpu()
    assert bool(torch.isneginf(tail[:, 0]).all())
    assert torch.equal(tail[:, 1].view(torch.int32), got[:, P - 1].cpu().view(torch.int32))         # the last page of the shard
    assert torch.equal(tail[:, 2].view(torch.int32), got[:, 3].cpu().view(torch.int32))             # the duplicate


def test_rerank_k1c(amd):
    _check_rerank(amd, "bf16_128", [32, 17, 1, 128], 21, "K1c")


def _check_gather(amd, spec, corpus, block_bits, what):
    """gather_pages of every listed page against mine_truth.gather of the block's rows (int16 bit patterns), bit for bit"""
    from tests import mine_truth as mt

    P, pad = spec["P"], 1030
    tiles, ids = _list_ids(spec)
    out = torch.full((len(ids), pad, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
    box, lens = amd.gather_pages(corpus, torch.from_numpy(ids).to(DEV), pad_to=pad, out=out)
    assert box.data_ptr() == out.data_ptr()
    want_box, want_len = mt.gather(block_bits, spec["offsets"], np.arange(P), pad)
    want_box = torch.from_numpy(np.ascontiguousarray(want_box)).to(DEV)
    want_len = torch.from_numpy(np.asarray(want_len, dtype=np.int32)).to(DEV)
    bits = box.view(torch.int16)
    for i, t in enumerate(tiles):
        where = f"{what}: tile {t}; first boundary below it: {_boundary_before(spec, t)}"
        assert torch.equal(bits[i * P:(i + 1) * P], want_box), where
        assert torch.equal(lens[i * P:(i + 1) * P], want_len), where
    assert int(lens[-3]) == 0 and not bool(bits[-3].any())                                         # id -1: zeros
    assert torch.equal(bits[-2], want_box[P - 1]) and torch.equal(bits[-1], want_box[3])


def test_gather_pages(amd):
    spec, block, corpus = _shard(amd, "bf16_128")
    _check_gather(amd, spec, corpus, block.view(torch.int16).numpy(), "gather_pages")


def _check_align(amd, kind, what, rc=None, block=None):
    """align(maps=True): tile 0 through test_gpu_align's own verify (float64 truth, derived bound), the other tiles bit for bit.
    With `rc` (a ResidualCorpus over the shard) the pages are the decoded rows `block` and the call is residual_align."""
    from colpali_amd import Alignment
    from tests.test_gpu_align import Case, verify

    if rc is None:
        spec, block, corpus = _shard(amd, kind)
    else:
        spec, corpus = h.large_shard_spec(kind), rc
    P = spec["P"]
    g = torch.Generator().manual_seed(31)
    q_lens = [1, 17, 33]
    rows = torch.nn.functional.normalize(torch.randn(sum(q_lens), spec["width"], generator=g), dim=-1).to(block.dtype)
    qs = [t.clone() for t in rows.split(q_lens)]
    pages = [block[int(a):int(b)].clone() for a, b in zip(spec["offsets"][:-1], spec["offsets"][1:])]
    case = Case(amd, qs, pages, None, id_base=0)                  # the block as a corpus of its own: the truth, computed on the CPU
    tiles, ids = _list_ids(spec)
    cand = torch.from_numpy(np.tile(ids, (len(qs), 1))).to(DEV)
    al = amd.align(case.pq, corpus, cand, maps=True)
    assert torch.equal(al.ids, cand)
    first = Alignment(best_sim=al.best_sim[:, :P], best_row=al.best_row[:, :P], ids=al.ids[:, :P], sims=al.sims[:, :P])
    verify(case, first, cand[:, :P].cpu().numpy(), maps=True)
    for name, x in (("best_sim", al.best_sim), ("best_row", al.best_row), ("sims", al.sims)):
        for i, t in enumerate(tiles):
            assert torch.equal(x[:, i * P:(i + 1) * P].view(torch.int32), x[:, :P].view(torch.int32)), \
                f"{what}: {name} of tile {t} differs from tile 0; first boundary below it: {_boundary_before(spec, t)}"
        assert torch.equal(x[:, -2].view(torch.int32), x[:, P - 1].view(torch.int32))
        assert torch.equal(x[:, -1].view(torch.int32), x[:, 3].view(torch.int32))
    assert bool(torch.isneginf(al.best_sim[:, -3, :1]).all()) and bool((al.best_row[:, -3] == -1).all())


def test_align_with_maps(amd):
    _check_align(amd, "bf16_128", "align")


# ------------------------------------------------------------------------------------------------------------------ first stages
FIRST_Q_LENS = [32, 17, 1, 64]


def _first_stage_queries(seed=61):
    g = torch.Generator().manual_seed(seed)
    rows = torch.nn.functional.normalize(torch.randn(sum(FIRST_Q_LENS), 128, generator=g), dim=-1).to(torch.bfloat16)
    return [t.clone() for t in rows.split(FIRST_Q_LENS)]


def _assert_rows_repeat(spec, x, want0, what):
    """x [T * R0, ...] on the device: every tile of R0 rows equals want0 [R0, ...] (device, same dtype)"""
    T, R0 = spec["T"], spec["R0"]
    same = (x.view(T, R0, -1) == want0.view(1, R0, -1)).all(dim=2).all(dim=1)
    bad = (~same).nonzero()
    assert bad.numel() == 0, (f"{what}: tile {int(bad[0])} differs from the block's; first boundary below it: "
                              f"{_boundary_before(spec, int(bad[0]))}; {int(bad.numel())} tiles differ")


def test_int8_index(amd):
    from tests import int8_truth as it

    spec, block, corpus = _shard(amd, "bf16_128")
    P, T = spec["P"], spec["T"]
    idx = amd.Int8Index.build(corpus)
    d8, sd = it.quantize_pages(block.float().numpy(), spec["offsets"])
    _assert_rows_repeat(spec, idx.codes, torch.from_numpy(d8).to(DEV), "int8 codes")
    want_sd = torch.from_numpy(np.asarray(sd, dtype=np.float32)).to(DEV).view(torch.int32)
    assert bool((idx.scales.view(torch.int32).view(T, P) == want_sd.view(1, P)).all()), "int8 scales"
    qs = _first_stage_queries()
    out = torch.full((len(qs), len(corpus)), float("nan"), dtype=torch.float32, device=DEV)
    got = amd.int8_scores(amd.pack_queries(qs, DEV, layout="flat", compact=False), idx, out=out)
    assert got.data_ptr() == out.data_ptr()
    q8, sq = it.quantize_tokens(torch.cat(qs).float().numpy())
    want = it.scores(q8, sq, np.cumsum([0] + FIRST_Q_LENS), d8, sd, spec["offsets"])
    np.testing.assert_array_equal(got[:, :P].cpu().numpy().view(np.int32), want.view(np.int32))
    _assert_tiles_repeat(spec, got, "int8_scores")


def test_fde_index(amd):
    from colpali_amd.fde import encode_corpus
    from tests.test_gpu_fde import _check_encoding

    spec, block, corpus = _shard(amd, "bf16_128")
    P, T, R0 = spec["P"], spec["T"], spec["R0"]
    config = amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=3)                         # F = 256: the encoding stays in the millisecond range
    codes = torch.full((corpus.blob.shape[0], config.reps), 255, dtype=torch.uint8, device=DEV)
    out = torch.full((len(corpus), config.dim), float("nan"), dtype=torch.bfloat16, device=DEV)
    Fd = encode_corpus(corpus, config, out=out, codes=codes)
    _check_encoding(Fd[:P], block, spec["offsets"], codes[:R0], config, doc=True)
    _assert_rows_repeat(spec, codes, codes[:R0].clone(), "FDE bucket codes")
    assert bool((Fd.view(torch.int16).view(T, P, -1) == Fd.view(torch.int16)[:P].unsqueeze(0)).all()), "FDE encodings differ between tiles"
    index = amd.FdeIndex(Fd, 0, config)
    pq = amd.pack_queries(_first_stage_queries(), DEV, layout="flat", compact=False)
    got = amd.fde_scores(pq, index, out=torch.full((len(pq), len(corpus)), float("nan"), dtype=torch.float32, device=DEV))
    Fq = amd.encode_queries(pq, index)
    q, d = Fq.double().cpu().numpy(), Fd[:P].double().cpu().numpy()
    assert (np.abs(got[:, :P].double().cpu().numpy() - q @ d.T) <= 1e-5 * (np.abs(q) @ np.abs(d).T) + 1e-30).all()      # test_gpu_fde._scores_check
    _assert_tiles_repeat(spec, got, "fde_scores")


def _centroids(K=256, seed=71):
    g = torch.Generator().manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(K, 128, generator=g), dim=-1).to(torch.bfloat16)


def test_centroid_index(amd):
    from tests import centroid_truth as ct
    from tests.test_gpu_centroid import _check_scores, _index

    spec, block, corpus = _shard(amd, "bf16_128")
    P, R0 = spec["P"], spec["R0"]
    C = _centroids()
    idx = amd.CentroidIndex.build(corpus, centroids=C.to(DEV))
    codes0 = idx.codes.view(torch.int16)[:R0].clone()
    c0 = codes0.cpu().numpy().view(np.uint16).astype(np.int64)
    sims = ct.sims64(block.float().numpy(), C.float().numpy())
    assert (sims[np.arange(R0), c0] >= sims.max(axis=1) - ct.encode_slack(block.float().numpy(), C.float().numpy())).all()
    _assert_rows_repeat(spec, idx.codes.view(torch.int16), codes0, "centroid codes")
    qs = _first_stage_queries()
    out = torch.full((len(qs), len(corpus)), float("nan"), dtype=torch.float32, device=DEV)
    got = amd.centroid_scores(amd.pack_queries(qs, DEV, layout="flat", compact=False), idx, out=out)
    _check_scores(got[:, :P], qs, C, _index(amd, C, c0.astype(np.uint16), spec["lens"]), "centroid_scores, tile 0")
    _assert_tiles_repeat(spec, got, "centroid_scores")


def test_residual_corpus(amd):
    """encode, decode_rows across every boundary, residual_scores, residual_rerank_scores, residual_align, residual_gather_pages"""
    from tests import residual_truth as rt

    spec, block, corpus = _shard(amd, "bf16_128")
    P, R0, T, off = spec["P"], spec["R0"], spec["T"], spec["offsets"]
    C = _centroids()
    idx = amd.CentroidIndex.build(corpus, centroids=C.to(DEV))
    c0 = idx.codes.view(torch.int16)[:R0].cpu().numpy().view(np.uint16)
    rows32, C32 = block.float().numpy(), C.float().numpy()
    cutoffs, weights = amd.train_residual_codec(torch.from_numpy(rows32 - C32[c0.astype(np.int64)]), 2)
    rc = amd.ResidualCorpus.build(corpus, index=idx, bits=2, cutoffs=cutoffs.to(DEV), weights=weights.to(DEV))
    want_res = rt.encode(rows32, C32, c0, cutoffs.numpy(), 2)
    _assert_rows_repeat(spec, rc.residuals, torch.from_numpy(want_res).to(DEV), "residual bytes")
    xhat_bits = rt.decode(C32, c0, want_res, weights.numpy(), 2, "bf16")                   # uint16 [R0, 128]
    xhat_dev = torch.from_numpy(xhat_bits.view(np.int16)).to(DEV)
    for name, b in spec["bounds"].items():                                                 # decode_rows over a range that straddles the boundary
        r0, r1 = b - 700, min(b + 700, spec["rows"])
        out = torch.full((r1 - r0, 128), float("nan"), dtype=torch.bfloat16, device=DEV)
        rc._decode(r0, r1, out)
        phase = torch.arange(r0, r1, device=DEV) % R0
        assert torch.equal(out.view(torch.int16), xhat_dev[phase]), f"decode_rows across {name}"
    qs = _first_stage_queries()
    pq = amd.pack_queries(qs, DEV, layout="flat", compact=False)
    want, tol = rt.maxsim64(torch.cat(qs).float().numpy(), np.cumsum([0] + FIRST_Q_LENS), rt.from_bits(xhat_bits, "bf16"), off)
    fin = np.isfinite(want)

    def check0(got0, what):
        g = got0.double().cpu().numpy()
        np.testing.assert_array_equal(g[~fin], want[~fin])
        err = np.abs(g[fin] - want[fin])
        print(f"    {what}: largest error {err.max():.3e} (its bound {tol[fin][err.argmax()]:.3e})")
        assert (err <= tol[fin]).all(), what

    out = torch.full((len(qs), len(rc)), float("nan"), dtype=torch.float32, device=DEV)
    got = amd.residual_scores(pq, rc, out=out)
    check0(got[:, :P], "residual_scores, tile 0")
    _assert_tiles_repeat(spec, got, "residual_scores")
    tiles, ids = _list_ids(spec)
    cand = torch.from_numpy(np.tile(ids, (len(qs), 1))).to(DEV)
    out = torch.full(tuple(cand.shape), float("nan"), dtype=torch.float32, device=DEV)
    rr, rr_ids = amd.residual_rerank_scores(pq, rc, cand, out=out)
    assert torch.equal(rr_ids, cand)
    check0(rr[:, :P], "residual_rerank_scores, tile 0")
    for i, t in enumerate(tiles):
        assert torch.equal(rr[:, i * P:(i + 1) * P].view(torch.int32), rr[:, :P].view(torch.int32)), \
            f"residual_rerank_scores: tile {t} differs from tile 0; first boundary below it: {_boundary_before(spec, t)}"
    assert bool(torch.isneginf(rr[:, -3]).all()) and torch.equal(rr[:, -2].view(torch.int32), rr[:, P - 1].view(torch.int32))
    _check_gather(amd, spec, rc, xhat_bits.view(np.int16), "residual_gather_pages")
    _check_align(amd, "bf16_128", "residual_align", rc=rc, block=torch.from_numpy(xhat_bits.view(np.int16)).view(torch.bfloat16))


# -------------------------------------------------------------------------------------------------------------------- end to end
def test_retriever_search_and_mine(amd, monkeypatch):
    """All T copies of a page tie exactly, so the top k (k <= T) of a plain scan is the best page of the block in every tile, ids
    ascending, equal scores; of a two-stage search (int8 prefilter, n_candidates = 1024 <= T) the int8-best page's first copies;
    and the hard negatives of a query whose positive is the best page of tile 0 are that page's other copies."""
    from tests import int8_truth as it

    monkeypatch.setenv("COLPALI_AMD_PACK13", "0")                           # the scans of this test read the blob (K1s), no image is built
    spec, block, corpus = _shard(amd, "bf16_128")
    P, T = spec["P"], spec["T"]
    q_lens = [32] * 4
    assert k_max_ok(T)
    qs, want = _queries_and_truth(spec, block, q_lens, 11)
    top2 = np.sort(want, axis=1)[:, -2:]
    assert ((top2[:, 1] - top2[:, 0]) > 4 * RTOL * np.abs(top2[:, 1])).all(), "the best page of the block must be clear of the second"
    best = want.argmax(axis=1)
    k = 64
    r = amd.ShardedRetriever(corpus)
    pq = amd.pack_queries(qs, DEV, compact=False)
    s, i = r.search(pq, k=k)
    want_ids = best[:, None] + P * np.arange(k)[None, :]
    np.testing.assert_array_equal(i.cpu().numpy(), want_ids)
    assert bool((s.view(torch.int32) == s.view(torch.int32)[:, :1]).all())
    assert np.all(np.abs(s[:, 0].double().cpu().numpy() - want[np.arange(4), best]) <= RTOL * np.abs(want[np.arange(4), best]))
    # two-stage: the int8 scores are exact integers times scales, so every copy ties in stage 1 as well
    idx = amd.Int8Index.build(corpus)
    d8, sd = it.quantize_pages(block.float().numpy(), spec["offsets"])
    q8, sq = it.quantize_tokens(torch.cat(qs).float().numpy())
    coarse = it.scores(q8, sq, np.cumsum([0] + q_lens), d8, sd, spec["offsets"])
    best8 = np.array([min(np.flatnonzero(row == row.max())) for row in coarse])
    s2, i2 = r.search(pq, k=k, prefilter=idx, n_candidates=1024)
    np.testing.assert_array_equal(i2.cpu().numpy(), best8[:, None] + P * np.arange(k)[None, :])
    assert bool((s2.view(torch.int32) == s2.view(torch.int32)[:, :1]).all())
    for q in range(4):                                                     # the exact score of that page: the bits the scan gave it
        if best8[q] == best[q]:
            assert torch.equal(s2[q, :1].view(torch.int32), s[q, :1].view(torch.int32))
    del idx
    # mining: positive = the best page of tile 0 -> its copies from tile 1 on; with the 0.95 rule they score above the bound and
    # the second-best page of the block takes over, in every tile
    pos = torch.from_numpy(best.astype(np.int64)).to(DEV)
    n_neg = 48
    ns, ni = r.mine(pq, pos, n_neg)
    np.testing.assert_array_equal(ni.cpu().numpy(), best[:, None] + P * (1 + np.arange(n_neg))[None, :])
    assert bool((ns.view(torch.int32) == s.view(torch.int32)[:, :1]).all())
    order = np.argsort(-want, axis=1)
    second = np.array([next(p for p in order[q] if want[q, p] <= 0.95 * want[q, best[q]] * (1 - 4 * RTOL)) for q in range(4)])
    for q in range(4):                                                     # no page of the block sits within rounding of the 0.95 cut
        assert not np.any(np.abs(want[q] - 0.95 * want[q, best[q]]) <= 4 * RTOL * np.abs(want[q, best[q]]))
    ns, ni = r.mine(pq, pos, n_neg, max_ratio=0.95)
    np.testing.assert_array_equal(ni.cpu().numpy(), second[:, None] + P * np.arange(n_neg)[None, :])
    assert bool((ns.view(torch.int32) == ns.view(torch.int32)[:, :1]).all())


# -------------------------------------------------------------------------------------------------------------------- live shards
def k_max_ok(T):
    """k and n_candidates of the end-to-end test stay at or below T: every returned page is a copy of ONE page of the block"""
    return 64 <= T and 1024 <= T and 49 <= T


def _without_empty_page(spec):
    """(offsets int64 [T * (P - 1) + 1] host, lengths int64 [T * (P - 1)]): the same rows with the 0-row page left out of the page
    table -- a live shard holds no page of 0 rows"""
    lens = [n for n in spec["lens"] if n]
    lengths = np.tile(np.asarray(lens, dtype=np.int64), spec["T"])
    off = np.zeros(lengths.size + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    assert off[-1] == spec["rows"]
    return off, lengths


def _live_history(spec, off):
    """the two deleted slots: slot 5 (tile 0) and the first slot that starts past row 2^24; alive uint8 [n]"""
    n = off.size - 1
    dead = [5, int(np.searchsorted(off, spec["bounds"]["element 2^31"], side="left"))]
    assert off[dead[1]] >= 2**24 and dead[1] < n
    alive = np.ones(n, dtype=np.uint8)
    alive[dead] = 0
    return dead, alive


def _assert_compacted(rows_now, rows_then, off, dead, what):
    """rows_now[: survivors] equals the surviving slices of rows_then ([rows, w], 8 bytes per piece where the row allows it),
    compared slice by slice on the device -- torch.cat of 8.6 GB would not fit the module's budget"""
    a, b = (int(off[dead[0]]), int(off[dead[0] + 1])), (int(off[dead[1]]), int(off[dead[1] + 1]))
    total = int(off[-1])
    pieces = [(0, 0, a[0]), (a[0], a[1], b[0] - a[1]), (a[0] + b[0] - a[1], b[1], total - b[1])]         # (destination, source, rows)
    for dst, src, n in pieces:
        for c0 in range(0, n, 1 << 22):                                                                # 4 M rows at a time
            c1 = min(n, c0 + (1 << 22))
            assert torch.equal(rows_now[dst + c0:dst + c1], rows_then[src + c0:src + c1]), f"{what}: rows {dst + c0} .. {dst + c1} after the compaction"


@pytest.mark.parametrize("bounce_mb", [4, 512])
def test_live_compaction(amd, bounce_mb):
    from tests import live_truth as lt

    spec, block, corpus = _shard(amd, "bf16_128")
    off, lengths = _without_empty_page(spec)
    dead, alive = _live_history(spec, off)
    packed = amd.PackedCorpus(corpus.blob, torch.from_numpy(off.astype(np.int32)).to(DEV), None, torch.from_numpy(lengths))
    live = amd.LiveCorpus.from_packed(packed, 0, 0, bounce_bytes=bounce_mb << 20)
    live.delete(dead)
    live.compact()
    n = lengths.size
    np.testing.assert_array_equal(live.offsets[:n + 1].cpu().numpy().astype(np.int64), lt.compact_offsets(off, alive))
    assert live.rows_used == int(off[-1]) - int(lengths[dead].sum())
    _assert_compacted(live.blob.view(torch.int64), corpus.blob.view(torch.int64), off, dead, f"LiveCorpus, {bounce_mb} MiB bounce buffer")
    live.check()


def test_live_residual_compaction(amd):
    from tests import live_truth as lt

    spec, block, corpus = _shard(amd, "bf16_128")
    off, lengths = _without_empty_page(spec)
    dead, alive = _live_history(spec, off)
    idx = amd.CentroidIndex.build(corpus, centroids=_centroids().to(DEV))
    cut = torch.tensor([-0.03, 0.0, 0.03], dtype=torch.float32, device=DEV)
    wts = torch.tensor([-0.05, -0.015, 0.015, 0.05], dtype=torch.float32, device=DEV)
    rc = amd.ResidualCorpus.build(corpus, index=idx, bits=2, cutoffs=cut, weights=wts)
    rc59 = amd.ResidualCorpus(rc.centroids, rc.codes, rc.residuals, rc.cutoffs, rc.weights, torch.from_numpy(off.astype(np.int32)).to(DEV),
                              None, torch.from_numpy(lengths), 0, 2)
    live = amd.LiveResidualCorpus.from_residual(rc59, 0, 0, bounce_bytes=4 << 20)
    live.delete(dead)
    live.compact()
    n = lengths.size
    np.testing.assert_array_equal(live.offsets[:n + 1].cpu().numpy().astype(np.int64), lt.compact_offsets(off, alive))
    _assert_compacted(live.codes.view(torch.int16).unsqueeze(1), rc.codes.view(torch.int16).unsqueeze(1), off, dead, "LiveResidualCorpus codes")
    _assert_compacted(live.residuals, rc.residuals, off, dead, "LiveResidualCorpus residuals")
    live.check()


# ----------------------------------------------------------------------------------------------------------- width 320 and fp32
@pytest.mark.parametrize("q_lens", [[32] * 4, [33, 47, 12, 40, 21, 38, 9, 27, 44]], ids=["K1sP", "K1bPF"])
def test_scan_wide(amd, q_lens, request):
    family = request.node.callspec.id
    assert _wide_family(q_lens) == family
    _check_scan(amd, "bf16_320", q_lens, 41, family)
    print(f"    kernel family: {family} (width 320; the dispatch rule of msim_fwd_ragged)")


def test_rerank_wide_k1cp(amd):
    _check_rerank(amd, "bf16_320", [32, 17, 1, 128], 42, "K1cP")


def test_align_wide_with_maps(amd):
    _check_align(amd, "bf16_320", "align at width 320")


def test_scan_generic_fp32(amd):
    spec, block, corpus = _shard(amd, "f32_128")
    q_lens = [32, 20, 7]
    qs, want = _queries_and_truth(spec, block, q_lens, 51)
    box = torch.nn.utils.rnn.pad_sequence(qs, batch_first=True).to(DEV).contiguous()      # fp32: the box layout, the generic kernel
    assert isinstance(amd.pack_queries(qs, DEV), torch.Tensor), "fp32 queries must take the box layout (the generic kernel)"
    out = torch.full((len(qs), len(corpus)), float("nan"), dtype=torch.float32, device=DEV)
    got = amd.maxsim_scores(box, corpus, out=out)
    _assert_close_tile0(got[:, :spec["P"]], want, "K1g fp32")
    _assert_tiles_repeat(spec, got, "K1g fp32")
    print("    kernel family: K1g (fp32 rows: the generic kernel is the only one that takes them)")


# --------------------------------------------------------------------------------------- score matrices of more than 2^31 entries

def _matrix(form):
    """(block fp32 [7, ld] numpy, the matrix [2049, ld] on the device, freshly written)"""
    ld, n_q, b = h.LARGE_MATRIX_LD[form], h.LARGE_MATRIX_ROWS, h.LARGE_MATRIX_BLOCK
    if _STATE.get("kind") != ("matrix", form):
        _release()
        blk = h.large_matrix_block(ld)
        _STATE.update(kind=("matrix", form), blk=blk, blk_dev=torch.from_numpy(blk).to(DEV),
                      mat=torch.empty((n_q, ld), dtype=torch.float32, device=DEV))
    blk_dev, mat = _STATE["blk_dev"], _STATE["mat"]
    whole = n_q // b * b
    mat[:whole].view(n_q // b, b, ld).copy_(blk_dev.unsqueeze(0).expand(n_q // b, b, ld))
    mat[whole:].copy_(blk_dev[:n_q - whole])
    assert mat.numel() > 2**31 and mat.is_contiguous()
    return _STATE["blk"], mat


def _assert_matrix_is_tiled(mat, want_blk, what):
    """mat [2049, ld] on the device repeats want_blk [7, ld] (numpy fp32) bit for bit; the probe rows again on the CPU"""
    n_q, ld = mat.shape
    b = h.LARGE_MATRIX_BLOCK
    want = torch.from_numpy(np.ascontiguousarray(want_blk)).to(DEV).view(torch.int32)
    bits = mat.view(torch.int32)
    row_ok = torch.empty((n_q,), dtype=torch.bool, device=DEV)
    for r0 in range(0, n_q, 7 * 32):                                           # 224 rows (0.9 GB) at a time
        r1 = min(n_q, r0 + 7 * 32)
        idx = torch.arange(r0, r1, device=DEV) % b
        row_ok[r0:r1] = (bits[r0:r1] == want[idx]).all(dim=1)
    bad = (~row_ok).nonzero()
    if bad.numel():
        r = int(bad[0])
        cols = (bits[r] != want[r % b]).nonzero().flatten()
        raise AssertionError(f"{what}: row {r} (element offset {r * ld}) differs from row {r % b} of the block at {int(cols.numel())} "
                             f"columns, the first {int(cols[0])}; {int(bad.numel())} rows differ; "
                             f"2^30 = row {2**30 // ld}, 2^31 = row {2**31 // ld}")
    for r in h.large_matrix_probe_rows(ld, n_q):
        assert np.array_equal(mat[r].cpu().numpy().view(np.int32), np.ascontiguousarray(want_blk[r % b]).view(np.int32)), (what, "probe row", r)


def _tile_rows(x, n_q=h.LARGE_MATRIX_ROWS):
    """[7, ...] numpy -> [n_q, ...]: row q is row q % 7"""
    return x[np.arange(n_q) % h.LARGE_MATRIX_BLOCK]


@pytest.mark.parametrize("form", ["vec", "odd"])
def test_matrix_topk(amd, form):
    from oracle import topk_oracle

    blk, mat = _matrix(form)
    n_q = mat.shape[0]
    for k in (10, 256):
        want_s, want_i = topk_oracle.topk(blk, k, id_base=1000)
        out = (torch.full((n_q, k), float("nan"), dtype=torch.float32, device=DEV), torch.full((n_q, k), -7, dtype=torch.int64, device=DEV))
        got_s, got_i = amd.topk(mat, k, id_base=1000, out=out)
        assert got_s.data_ptr() == out[0].data_ptr()
        np.testing.assert_array_equal(got_i.cpu().numpy(), _tile_rows(want_i), err_msg=f"topk k={k} ids")
        np.testing.assert_array_equal(got_s.cpu().numpy().view(np.int32), _tile_rows(want_s).view(np.int32), err_msg=f"topk k={k} scores")
    _assert_matrix_is_tiled(mat, blk, "topk must not write its input")


def _positives(ld, n_q):
    """CSR positives: query q has the in-range columns of [1, ld // 3 + q % 7, ld - 2] and, every third query, an id off the shard"""
    ids, off = [], [0]
    for q in range(n_q):
        ids += [1, ld // 3 + q % h.LARGE_MATRIX_BLOCK, ld - 2] + ([ld + 5] if q % 3 == 0 else [])
        off.append(len(ids))
    return np.asarray(ids, dtype=np.int64), np.asarray(off, dtype=np.int32)


@pytest.mark.parametrize("form", ["vec", "odd"])
def test_matrix_mine_mask(amd, form):
    from colpali_amd import mine
    from tests import mine_truth as mt

    blk, mat = _matrix(form)
    n_q, ld = mat.shape
    ids, off = _positives(ld, n_q)
    csr = (torch.from_numpy(ids).to(DEV), torch.from_numpy(off).to(DEV))
    pos7 = [[1, ld // 3 + r, ld - 2] for r in range(h.LARGE_MATRIX_BLOCK)]
    bounds = mine.mine_bounds(mat, csr)
    np.testing.assert_array_equal(bounds.cpu().numpy().view(np.int32), _tile_rows(mt.bounds(blk, pos7)).view(np.int32))
    for ratio in (None, 0.5):
        if ratio is not None:
            blk, mat = _matrix(form)
        mine.mine_mask(mat, csr, bounds=bounds if ratio is not None else None, max_ratio=ratio)
        _assert_matrix_is_tiled(mat, mt.masked(blk, pos7, max_ratio=ratio), f"mine_mask max_ratio={ratio}")


@pytest.mark.parametrize("form", ["vec", "odd"])
def test_matrix_filter_mask(amd, form):
    from colpali_amd.filter import filter_mask
    from tests import filter_truth as ft

    blk, mat = _matrix(form)
    n_q, ld = mat.shape
    rng = np.random.default_rng(5)
    shared = rng.random(ld) < 0.5
    shared[[0, ld - 1]] = [False, True]
    filter_mask(mat, amd.PageFilter.from_mask(torch.from_numpy(shared).to(DEV)))
    _assert_matrix_is_tiled(mat, ft.masked(blk, ft.allowed(("shared", shared), h.LARGE_MATRIX_BLOCK, ld)), "filter_mask, shared bits")
    blk, mat = _matrix(form)
    page_labels = rng.integers(0, 3, ld).astype(np.int32)
    q7 = np.arange(h.LARGE_MATRIX_BLOCK, dtype=np.int32) % 3
    flt = amd.PageFilter.from_labels(torch.from_numpy(page_labels).to(DEV), torch.from_numpy(_tile_rows(q7)).to(DEV))
    filter_mask(mat, flt)
    _assert_matrix_is_tiled(mat, ft.masked(blk, ft.allowed(("labels", page_labels, q7), h.LARGE_MATRIX_BLOCK, ld)), "filter_mask, labels")


@pytest.mark.parametrize("form", ["vec", "odd"])
def test_matrix_mask_scores(amd, form):
    from colpali_amd.live import mask_scores
    from tests import live_truth as lt

    blk, mat = _matrix(form)
    ld = mat.shape[1]
    alive = (np.random.default_rng(6).random(ld) < 0.7).astype(np.uint8)
    alive[[0, ld - 1]] = [1, 0]
    mask_scores(mat, torch.from_numpy(alive).to(DEV))
    _assert_matrix_is_tiled(mat, lt.mask(blk, alive), "mask_scores")


@pytest.mark.parametrize("form", ["vec", "odd"])
def test_matrix_group_reduce(amd, form):
    blk, mat = _matrix(form)
    n_q, ld = mat.shape
    labels = h.large_matrix_group_labels(ld)
    gids, want_s, want_p = h.group_reduce_truth_fast(blk, labels, id_base=0)
    groups = amd.PageGroups.from_labels(torch.from_numpy(labels).to(DEV))
    got_s, got_p = amd.group_reduce(mat, groups)
    np.testing.assert_array_equal(groups.group_ids.cpu().numpy(), gids)
    b = h.LARGE_MATRIX_BLOCK
    ws, wp = torch.from_numpy(want_s).to(DEV).view(torch.int32), torch.from_numpy(want_p).to(DEV)
    idx = torch.arange(n_q, device=DEV) % b
    bad = (~((got_s.view(torch.int32) == ws[idx]).all(dim=1) & (got_p == wp[idx]).all(dim=1))).nonzero()
    assert bad.numel() == 0, f"group_reduce: row {int(bad[0])} (element offset {int(bad[0]) * ld}) differs from the truth of row {int(bad[0]) % b}"
    for r in h.large_matrix_probe_rows(ld, n_q):
        np.testing.assert_array_equal(got_p[r].cpu().numpy(), want_p[r % b])
        np.testing.assert_array_equal(got_s[r].cpu().numpy().view(np.int32), want_s[r % b].view(np.int32))
    _assert_matrix_is_tiled(mat, blk, "group_reduce must not write its input")
