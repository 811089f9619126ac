"""Persistence on the MI355X: msim_digest against msim_digest_host, and save / load of every shard and index class through HBM.

Everything here is a bit identity, nothing has a tolerance.  Files are written with chunk_bytes=4096, so tensors end mid-chunk and
range loads cut inside chunks; the digest cases are the word-structure edges of tests/test_persist_host.py plus what only the
kernel has: a pointer 8 bytes off a 16-byte boundary, a range of several workgroups and strides, reruns and a graph replay."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_persist_host import POSITIONS, SIZES, assert_same_object

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
M64 = 2**64 - 1
CHUNK = 4096
LENS = (1, 33, 700, 1024, 5)


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _rows(g, n, dtype=torch.bfloat16, width=128):
    return torch.nn.functional.normalize(torch.randn(n, width, generator=g), dim=-1).to(dtype)


def _host(amd, data: torch.Tensor, pos=0):
    """msim_digest_host over a host uint8 tensor"""
    a = (ctypes.c_uint64 * 2)(0, 0)
    assert data.data_ptr() % 8 == 0
    assert amd._lib.lib().msim_digest_host(data.data_ptr() if data.numel() else None, data.numel(), pos, a) == 0
    return int(a[0]), int(a[1])


def _pair(acc):
    return tuple(int(v) & M64 for v in acc.cpu())


# ------------------------------------------------------------------------------------------------------------------- the digest
@pytest.mark.parametrize("pos", POSITIONS)
def test_device_digest_equals_the_host_entry(amd, pos):
    g = torch.Generator().manual_seed(pos % 1000)
    for nbytes in SIZES:
        data = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.int32).to(torch.uint8)
        assert _pair(amd.digest(data.to(DEV), pos)) == _host(amd, data, pos), (nbytes, pos)


def test_a_pointer_8_bytes_off_a_16_byte_boundary(amd):
    g = torch.Generator().manual_seed(1)
    base = torch.randint(0, 256, (8 + 8 * 3000 + 16,), generator=g, dtype=torch.int32).to(torch.uint8)
    dbase = base.to(DEV)
    assert dbase.data_ptr() % 16 == 0
    for nbytes in (8, 9, 16, 8 * 2 + 3, 8 * 1000, 8 * 1001, 8 * 1001 + 5, 8 * 3000 + 7):     # the head word, an odd and an even body, a tail
        part, dpart = base[8:8 + nbytes].clone(), dbase[8:8 + nbytes]
        assert dpart.data_ptr() % 16 == 8
        assert _pair(amd.digest(dpart, 2**32 + 8)) == _host(amd, part, 2**32 + 8), nbytes


def test_several_workgroups_and_strides_rerun_and_replay(amd):
    nbytes = (64 << 20) + 13                                              # 4M 16-byte pairs: 2048 workgroups, 8 strides, a byte tail
    g = torch.Generator(device=DEV).manual_seed(2)
    data = torch.randint(0, 256, (nbytes,), generator=g, dtype=torch.uint8, device=DEV)
    want = _host(amd, data.cpu(), 2**40)
    first, second = amd.digest(data, 2**40), amd.digest(data, 2**40)
    assert _pair(first) == want and _pair(second) == want                 # rerun identity: integer atomics commute
    # capture and replay: the call is one launch on the capturing stream, and every replay adds again
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    small = data[:8 * 5000 + 3]
    one = _pair(amd.digest(small, 16))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        amd.digest(small, 16, acc)
    acc.zero_()
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    assert _pair(acc) == ((2 * one[0]) & M64, (2 * one[1]) & M64)


def test_one_launch_past_4_gib_is_the_sum_of_launches_below_it(amd):
    """nbytes > 2^32 in ONE call: a byte offset or word index kept in 32 bits would wrap inside the launch.  No host pass over
    4 GiB: by the contract the digest is the sum of the digests of 64 MiB pieces, and launches of that size are what
    test_several_workgroups_and_strides_rerun_and_replay holds against the host entry."""
    piece = 64 << 20
    nbytes = 2**32 + 24
    g = torch.Generator(device=DEV).manual_seed(3)
    block = torch.randint(0, 256, (piece,), generator=g, dtype=torch.uint8, device=DEV)
    data = block.repeat(65)[:nbytes]                                      # the same bytes at other positions digest differently
    del block
    pos = 2**33 + 8
    whole = _pair(amd.digest(data, pos))
    acc = torch.zeros(2, dtype=torch.int64, device=DEV)
    for p0 in range(0, nbytes, piece):
        amd.digest(data[p0:min(nbytes, p0 + piece)], pos + p0, acc)
    assert whole == _pair(acc)
    assert whole != _pair(amd.digest(data[:2**32], pos))                  # ... and the 24 bytes past 2^32 took part


# ------------------------------------------------------------------------------------------------------------------ round trips
@pytest.fixture(scope="module")
def pages():
    g = torch.Generator().manual_seed(10)
    return [_rows(g, n) for n in LENS]


@pytest.fixture(scope="module")
def queries(amd):
    g = torch.Generator().manual_seed(11)
    return amd.pack_queries([_rows(g, n) for n in (32, 9, 20)], DEV)


def _codec(bits):
    g = torch.Generator().manual_seed(12 + bits)
    nb = 1 << bits
    return (torch.sort(torch.randn(nb - 1, generator=g) * 0.05).values.contiguous().to(DEV),
            torch.sort(torch.randn(nb, generator=g) * 0.08).values.contiguous().to(DEV))


def _centroids():
    return _rows(torch.Generator().manual_seed(13), 256).to(DEV)


def _equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("clamp", [True, False], ids=["clamp0", "noclamp"])
def test_round_trip_of_the_corpus_and_its_indexes(amd, tmp_path, pages, queries, clamp):
    pc = amd.pack_passages(pages, DEV, batch_size=2 if clamp else None, id_base=40)
    assert (pc.clamp0 is not None) == clamp
    cents = _centroids()
    objs = {
        "corpus": pc,
        "int8": amd.Int8Index.build(pc),
        "binary": amd.BinaryIndex.build(pc),
        "centroid": amd.CentroidIndex.build(pc, centroids=cents),
        "fde": amd.FdeIndex.build(pc, amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=5)),
    }
    back = {}
    for name, obj in objs.items():
        path = str(tmp_path / (name + ".msim"))
        obj.save(path, chunk_bytes=CHUNK)
        back[name] = amd.load(path, DEV)
        assert_same_object(back[name], obj)                                # every tensor torch.equal; dtype, device, id_base kept
        assert amd.verify_file(path)["kind"] == type(obj).__name__         # what the GPU wrote, the host entry verifies
    a, b = amd.ShardedRetriever(pc), amd.ShardedRetriever(back["corpus"])
    cand = torch.tensor([[40, 44, 41, -1], [43, 42, 99, 40], [44, 44, 40, 41]], dtype=torch.int64, device=DEV)
    assert _equal(a.search(queries, 3), b.search(queries, 3))
    assert _equal(a.search(queries, 3, candidates=cand), b.search(queries, 3, candidates=cand))
    for name in ("int8", "binary", "centroid", "fde"):
        assert _equal(a.search(queries, 3, prefilter=objs[name], n_candidates=4), b.search(queries, 3, prefilter=back[name], n_candidates=4)), name


@pytest.mark.parametrize("bits", [2, 4])
def test_round_trip_of_a_residual_corpus(amd, tmp_path, pages, queries, bits):
    pc = amd.pack_passages(pages, DEV, batch_size=2, id_base=40)
    cut, w = _codec(bits)
    rc = amd.ResidualCorpus.build(pc, index=amd.CentroidIndex.build(pc, centroids=_centroids()), bits=bits, cutoffs=cut, weights=w)
    path = str(tmp_path / "rc.msim")
    rc.save(path, chunk_bytes=CHUNK)
    got = amd.ResidualCorpus.load(path, DEV)
    assert_same_object(got, rc)
    assert got.index.codes.data_ptr() == got.codes.data_ptr() and got.index.centroids.data_ptr() == got.centroids.data_ptr()
    assert {e["name"] for e in amd.verify_file(path)["tensors"]} == {"centroids", "codes", "residuals", "cutoffs", "weights", "offsets",
                                                                     "clamp0", "lengths"}           # each once
    cand = torch.tensor([[40, 44, 41, -1], [43, 42, 99, 40], [44, 44, 40, 41]], dtype=torch.int64, device=DEV)
    a, b = (amd.ShardedRetriever(x, score_fn=amd.residual_scores) for x in (rc, got))
    assert _equal(a.search(queries, 3), b.search(queries, 3))
    assert _equal(a.search(queries, 3, candidates=cand), b.search(queries, 3, candidates=cand))
    assert _equal(a.search(queries, 3, prefilter=rc.index, n_candidates=4), b.search(queries, 3, prefilter=got.index, n_candidates=4))


@pytest.mark.parametrize("dtype,width", [(torch.bfloat16, 320), (torch.float32, 40)], ids=["bf16-320", "f32-40"])
def test_round_trip_at_other_formats(amd, tmp_path, dtype, width):
    g = torch.Generator().manual_seed(14)
    ps = [_rows(g, n, dtype, width) for n in LENS]
    qs = [_rows(g, n, dtype, width) for n in (32, 9, 20)]
    pc = amd.pack_passages(ps, DEV, batch_size=2, id_base=3)
    path = str(tmp_path / "pc.msim")
    pc.save(path, chunk_bytes=CHUNK)
    got = amd.load(path, DEV)
    assert_same_object(got, pc)
    assert got.dtype == dtype and got.width == width
    a, b = amd.ShardedRetriever(pc), amd.ShardedRetriever(got)
    assert _equal(a.search(qs, 3), b.search(qs, 3))
    if width == 320:
        cand = torch.tensor([[3, 7, 4, -1], [6, 5, 99, 3], [7, 7, 3, 4]], dtype=torch.int64, device=DEV)
        assert _equal(a.search(qs, 3, candidates=cand), b.search(qs, 3, candidates=cand))


def test_save_refuses_a_stream_capture(amd, tmp_path, pages):
    pc = amd.pack_passages(pages, DEV, batch_size=None)
    scratch = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scratch.add_(1)
        with pytest.raises(RuntimeError, match="capture"):
            pc.save(str(tmp_path / "x.msim"))
    assert not (tmp_path / "x.msim").exists() and not (tmp_path / "x.msim.tmp").exists()


# ------------------------------------------------------------------------------------------------------------------ live shards
def _history(live, g, dtype=torch.bfloat16):
    """add, delete, compact, add, delete (no compact); returns the ids deleted"""
    live.add([_rows(g, n, dtype) for n in (1, 300, 17, 64, 257, 40, 9)])
    live.delete([live.id_base + 0, live.id_base + 3, live.id_base + 4])
    live.compact()
    live.add([_rows(g, n, dtype) for n in (33, 5, 120)])
    live.delete([live.id_base + 8, live.id_base + 1])
    return [live.id_base + s for s in (0, 3, 4, 8, 1)]


def _live_answers(live, queries, stage1, scan=True):
    cand = torch.arange(live.id_base - 1, live.id_base + 11, dtype=torch.int64, device=DEV).repeat(3, 1)
    out = [live.search(queries, 4, candidates=cand), live.search(queries, 4, prefilter=stage1(live), n_candidates=6)]
    if scan:
        out.append(live.search(queries, 4))
    return out


def _check_live(amd, live, got, gone, queries, stage1, g, tmp_path):
    assert (got.n_slots, got.rows_used, got.id_base, got.n_live) == (live.n_slots, live.rows_used, live.id_base, live.n_live)
    assert (got.capacity_rows, got.capacity_docs) == (live.capacity_rows + 1000, live.capacity_docs + 7)
    for x, y in zip(_live_answers(live, queries, stage1), _live_answers(got, queries, stage1)):
        assert _equal(x, y)
        assert not np.isin(y[1].cpu().numpy(), gone).any()                 # deleted ids stay gone
    more = [_rows(g, n) for n in (12, 70)]
    assert got.add(more).tolist() == live.add(more).tolist() == [live.id_base + 10, live.id_base + 11]
    with pytest.raises(KeyError):
        got.delete([gone[0]])
    for x in (live, got):
        x.compact()
        x.check()
    assert got.rows_used == live.rows_used
    for x, y in zip(_live_answers(live, queries, stage1), _live_answers(got, queries, stage1)):
        assert _equal(x, y)
    with pytest.raises(ValueError, match="pages="):
        amd.load(str(tmp_path / "live.msim"), DEV, pages=(0, 2))
    with pytest.raises(ValueError, match="smaller"):
        amd.load(str(tmp_path / "live.msim"), DEV, capacity_rows=10)


def test_a_live_corpus_comes_back_with_its_slots(amd, tmp_path, queries):
    g = torch.Generator().manual_seed(20)
    live = amd.LiveCorpus(3000, 20, DEV, id_base=500)
    gone = _history(live, g)
    path = str(tmp_path / "live.msim")
    live.save(path, chunk_bytes=CHUNK)
    assert {e["name"] for e in amd.verify_file(path)["tensors"]} == {"blob", "offsets", "alive", "lengths"}     # no int8 index, no workspace
    got = amd.LiveCorpus.load(path, DEV, capacity_rows=4000, capacity_docs=27)
    assert torch.equal(got.blob[:live.rows_used], live.blob[:live.rows_used]) and not got.blob[live.rows_used:].any()
    assert torch.equal(got.offsets[:live.n_slots + 1], live.offsets[:live.n_slots + 1]) and torch.equal(got.alive[:20], live.alive[:20])
    _check_live(amd, live, got, gone, queries, lambda x: x.int8_index(), g, tmp_path)
    same = amd.load(path, DEV)                                             # the saved capacity by default
    assert (same.capacity_rows, same.capacity_docs) == (3000, 20)


@pytest.mark.parametrize("bits", [2, 4])
def test_a_live_residual_corpus_comes_back_with_its_slots(amd, tmp_path, queries, bits):
    g = torch.Generator().manual_seed(21)
    cut, w = _codec(bits)
    live = amd.LiveResidualCorpus(_centroids(), cut, w, bits, 3000, 20, id_base=500, score_fn=amd.residual_scores)
    gone = _history(live, g)
    path = str(tmp_path / "live.msim")
    live.save(path, chunk_bytes=CHUNK)
    got = amd.LiveResidualCorpus.load(path, DEV, capacity_rows=4000, capacity_docs=27, score_fn=amd.residual_scores)
    r = live.rows_used
    assert torch.equal(got.codes.view(torch.int16)[:r], live.codes.view(torch.int16)[:r]) and torch.equal(got.residuals[:r], live.residuals[:r])
    assert torch.equal(got.centroids, live.centroids) and torch.equal(got.cutoffs, live.cutoffs) and got.bits == bits
    _check_live(amd, live, got, gone, queries, lambda x: x.index, g, tmp_path)


# ------------------------------------------------------------------------------------------------------------------ range loads
def test_range_loads_equal_the_pack_of_those_pages_and_serve_virtual_shards(amd, tmp_path, pages, queries):
    g = torch.Generator().manual_seed(30)
    ps = list(pages) + [_rows(g, n) for n in (64, 2, 130, 16)]             # 9 pages; 256-byte rows: 16 rows per chunk
    base = 70
    pc = amd.pack_passages(ps, DEV, batch_size=None, id_base=base)
    path = str(tmp_path / "pc.msim")
    pc.save(path, chunk_bytes=CHUNK)
    for lo, hi in [(0, 9), (1, 3), (2, 4), (3, 3), (0, 0), (9, 9), (8, 9), (4, 8)]:       # page 1 starts at row 1, page 2 at row 34: inside chunks
        got = amd.PackedCorpus.load(path, DEV, pages=(lo, hi))
        assert got.id_base == base + lo and len(got) == hi - lo and got.device == DEV
        if lo == hi:
            assert got.blob.shape == (1, 128) and not got.blob.any() and got.offsets.tolist() == [0]
        else:
            assert_same_object(got, amd.pack_passages(ps[lo:hi], DEV, batch_size=None, id_base=base + lo))
    k, world = 4, 3
    whole = amd.ShardedRetriever(pc).search(queries, k)
    parts = [amd.ShardedRetriever(amd.PackedCorpus.load(path, DEV, pages=amd.shard_range(len(ps), world, r))).search(queries, k)
             for r in range(world)]
    merged = amd.merge_gathered(torch.stack([s for s, _ in parts]), torch.stack([i for _, i in parts]), k)
    assert _equal(whole, merged)
    # the indexes cut the same way: rows at offsets[lo] .. offsets[hi], pages at lo .. hi, an FdeIndex by rows of Fd
    for obj in (amd.Int8Index.build(pc), amd.FdeIndex.build(pc, amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=5))):
        p = str(tmp_path / "idx.msim")
        obj.save(p, chunk_bytes=CHUNK)
        got = type(obj).load(p, DEV, pages=(2, 7))
        sub = amd.pack_passages(ps[2:7], DEV, batch_size=None, id_base=base + 2)
        want = amd.Int8Index.build(sub) if isinstance(obj, amd.Int8Index) else amd.FdeIndex.build(sub, obj.config)
        assert_same_object(got, want)


# ------------------------------------------------------------------------------------------------------------------- corruption
def test_a_flipped_byte_is_caught_where_it_landed(amd, tmp_path, pages):
    pc = amd.pack_passages(pages, DEV, batch_size=None)
    path = str(tmp_path / "pc.msim")
    pc.save(path, chunk_bytes=CHUNK)
    blob = next(e for e in amd.verify_file(path)["tensors"] if e["name"] == "blob")
    with open(path, "r+b") as f:
        f.seek(blob["offset"] + 5 * CHUNK + 100)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 0x80]))
    with pytest.raises(amd.ShardFileError, match=r"'blob', chunk 5 \(bytes 20480 \.\. 24576"):
        amd.load(path, DEV)
    with pytest.raises(amd.ShardFileError, match=r"'blob', chunk 5"):
        amd.PackedCorpus.load(path, DEV, pages=(2, 4))                     # rows 34 .. 1757 cover chunk 5
    got = amd.load(path, DEV, verify=False)                                # the same file, unverified: loads, one byte off
    diff = (got.blob.view(torch.uint8) != pc.blob.view(torch.uint8)).sum().item()
    assert diff == 1 and torch.equal(got.offsets, pc.offsets)
