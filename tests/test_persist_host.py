"""Persistence without a GPU: msim_digest_host against its contract (tests/digest_truth.py), and the file format with CPU tensors.

Everything here is a bit identity.  The digest cases are the edges of the word structure (a byte tail, one word, one word and a
tail, two words, the 4096-byte chunk and its neighbours) at positions on both sides of 2^32 and beyond 2^40."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import digest_truth as dt

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097]
POSITIONS = [0, 8, 2**32 - 8, 2**32, 2**40 + 16]
EINVAL = -1
M64 = 2**64 - 1


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _host_digest(amd, data: np.ndarray, pos=0, acc=(0, 0)):
    """msim_digest_host over a uint8 array (its buffer is 8-byte aligned: a fresh numpy allocation)"""
    a = (ctypes.c_uint64 * 2)(*acc)
    buf = np.ascontiguousarray(data)
    assert buf.ctypes.data % 8 == 0
    rc = amd._lib.lib().msim_digest_host(buf.ctypes.data if buf.size else None, buf.size, pos, a)
    assert rc == 0, amd._lib.lib().msim_last_error()
    return int(a[0]), int(a[1])


def _bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- the digest
@pytest.mark.parametrize("pos", POSITIONS)
@pytest.mark.parametrize("nbytes", SIZES)
def test_host_digest_is_the_contract(amd, nbytes, pos):
    data = _bytes(nbytes + 1, nbytes)
    assert _host_digest(amd, data, pos) == dt.digest(data.tobytes(), pos)


def test_chunks_compose_over_random_aligned_cuts(amd):
    rng = np.random.default_rng(5)
    data = _bytes(6, 8 * 1000 + 5)
    whole = _host_digest(amd, data, 2**32 - 64)
    assert whole == dt.digest(data.tobytes(), 2**32 - 64)
    for _ in range(5):
        cuts = [0] + sorted(8 * int(c) for c in rng.choice(np.arange(1, 1000), size=7, replace=False)) + [data.size]
        acc = (0, 0)
        for a, b in zip(cuts[:-1], cuts[1:]):
            acc = _host_digest(amd, data[a:b].copy(), 2**32 - 64 + a, acc)
        assert acc == whole


def test_a_seeded_acc_is_added_to(amd):
    data = _bytes(7, 100)
    seed = (M64 - 3, 12345)                                                # lane 0 wraps
    want = dt.digest(data.tobytes(), 16)
    assert _host_digest(amd, data, 16, seed) == ((want[0] + seed[0]) & M64, (want[1] + seed[1]) & M64) == dt.digest(data.tobytes(), 16, seed)


@pytest.mark.parametrize("where", ["first byte", "last byte", "byte tail"])
def test_one_flipped_bit_changes_both_lanes(amd, where):
    n = 4096 + (5 if where == "byte tail" else 0)
    data = _bytes(8, n)
    base = _host_digest(amd, data)
    flipped = data.copy()
    flipped[{"first byte": 0, "last byte": n - 1, "byte tail": n - 3}[where]] ^= 0x10
    got = _host_digest(amd, flipped)
    assert got[0] != base[0] and got[1] != base[1] and got == dt.digest(flipped.tobytes())


def test_swapped_words_and_zero_lengths_are_told_apart(amd):
    words = np.arange(1, 65, dtype=np.uint64)
    swapped = words.copy()
    swapped[[3, 40]] = swapped[[40, 3]]
    a, b = _host_digest(amd, words.view(np.uint8)), _host_digest(amd, swapped.view(np.uint8))
    assert a[0] != b[0] and a[1] != b[1]
    z8, z16, z9 = (_host_digest(amd, np.zeros(n, dtype=np.uint8)) for n in (8, 16, 9))
    assert len({z8, z16, z9}) == 2 and z16 == z9 and z8 != z16             # a zero-padded tail IS a zero word; a further word counts
    assert _host_digest(amd, np.zeros(8, dtype=np.uint8), 8) != z8         # ... and so does the position


def test_refusals(amd):
    L = amd._lib.lib()
    buf = np.zeros(64, dtype=np.uint8)
    acc = (ctypes.c_uint64 * 2)(11, 22)
    p = buf.ctypes.data
    for fn, extra in ((L.msim_digest_host, ()), (L.msim_digest, (None,))):     # the device entry refuses before any device work
        assert fn(p, 16, 0, None, *extra) == EINVAL and b"acc" in L.msim_last_error()
        assert fn(None, 16, 0, acc, *extra) == EINVAL and b"NULL" in L.msim_last_error()
        assert fn(p, 16, 4, acc, *extra) == EINVAL and b"pos" in L.msim_last_error()
        assert fn(p + 4, 16, 0, acc, *extra) == EINVAL and b"aligned" in L.msim_last_error()
        assert fn(None, 0, 0, acc, *extra) == 0 and fn(p, 0, 8, acc, *extra) == 0           # nbytes == 0: a successful no-op
    assert (acc[0], acc[1]) == (11, 22)


def test_header_declares_both_entries_and_the_abi_stays_22(amd):
    text = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"int msim_digest\(const void \*data, size_t nbytes, uint64_t pos, uint64_t \*acc[^)]*, void \*stream\);", text)
    assert re.search(r"int msim_digest_host\(const void \*data, size_t nbytes, uint64_t pos, uint64_t acc\[2\]\);", text)
    assert "#define MSIM_ABI_VERSION 22" in text and amd._lib.ABI_VERSION == 22 and amd._lib.lib().msim_abi_version() == 22
    assert "NOT a cryptographic hash" in text
    consts = {name: int(v, 16) for name, v in re.findall(r"#define (MSIM_DIGEST_\w+) (0x[0-9A-Fa-f]+)ull", text)}
    assert consts == {"MSIM_DIGEST_C0": int(dt.C0), "MSIM_DIGEST_C1": int(dt.C1), "MSIM_DIGEST_K": int(dt.K)}
    assert len(set(consts.values())) == 3 and all(v & 1 for v in consts.values())
    for name in ("save", "load", "verify_file", "digest", "ShardFileError"):
        assert name in amd.__all__ and hasattr(amd, name)
    assert issubclass(amd.ShardFileError, ValueError)


def test_python_digest_wrapper_on_cpu_tensors(amd):
    t = torch.arange(300, dtype=torch.float32).to(torch.bfloat16)         # 600 bytes: 75 words
    acc = amd.digest(t, 2**32)
    assert tuple(int(v) & M64 for v in acc) == dt.digest(t.view(torch.uint8).numpy().tobytes(), 2**32)
    again = amd.digest(t, 2**32, acc)
    assert again is acc and tuple(int(v) & M64 for v in acc) == dt.digest(t.view(torch.uint8).numpy().tobytes(), 2**32, dt.digest(t.view(torch.uint8).numpy().tobytes(), 2**32))
    with pytest.raises(ValueError, match="pos"):
        amd.digest(t, 3)


# ------------------------------------------------------------------------------------------------------------------- the format
def _rows(g, n, dtype=torch.bfloat16, width=128):
    return torch.nn.functional.normalize(torch.randn(n, width, generator=g), dim=-1).to(dtype)


def _corpus(amd, clamp=True, dtype=torch.bfloat16, width=128, id_base=7):
    g = torch.Generator().manual_seed(3)
    ps = [_rows(g, n, dtype, width) for n in (1, 33, 70, 24, 5)]
    return amd.pack_passages(ps, "cpu", batch_size=2 if clamp else None, id_base=id_base), ps


def _frozen_objects(amd):
    """one object of each frozen class, built through its constructor from CPU tensors"""
    g = torch.Generator().manual_seed(4)
    pc, _ = _corpus(amd)
    rows, n = int(pc.blob.shape[0]), len(pc)
    cl = lambda t: None if t is None else t.clone()
    u16 = torch.randint(0, 256, (rows,), generator=g, dtype=torch.int32).to(torch.int16).view(torch.uint16)
    cents = _rows(g, 256)
    cfg = amd.FdeConfig(reps=2, ksim=3, dproj=16, seed=9, fill_empty=False)
    G, S = cfg.params()
    return {
        "PackedCorpus": pc,
        "PackedCorpus-f32-w40": _corpus(amd, clamp=False, dtype=torch.float32, width=40)[0],
        "Int8Index": amd.Int8Index(torch.randint(-128, 128, (rows, 128), generator=g, dtype=torch.int32).to(torch.int8),
                                   torch.rand(n, generator=g), pc.offsets.clone(), cl(pc.clamp0), pc.lengths.clone(), 7),
        "BinaryIndex": amd.BinaryIndex(torch.randint(0, 256, (rows, 16), generator=g, dtype=torch.int32).to(torch.uint8), pc.offsets.clone(),
                                       None, pc.lengths.clone(), 3),
        "CentroidIndex": amd.CentroidIndex(cents, u16.clone(), pc.offsets.clone(), cl(pc.clamp0), pc.lengths.clone(), 7),
        "FdeIndex": amd.FdeIndex(_rows(g, n, width=cfg.dim), 11, cfg, params=(G + 1.0, S)),      # NOT what the seed would re-draw
        "ResidualCorpus": amd.ResidualCorpus(cents, u16.clone(), torch.randint(0, 256, (rows, 64), generator=g, dtype=torch.int32).to(torch.uint8),
                                             torch.sort(torch.randn(15, generator=g)).values.contiguous(),
                                             torch.sort(torch.randn(16, generator=g)).values.contiguous(), pc.offsets.clone(), cl(pc.clamp0),
                                             pc.lengths.clone(), 7, 4),
    }


def _tensors(obj):
    """name -> tensor (or None) of everything an object stores, plus its scalars under "_meta" """
    if type(obj).__name__ == "FdeIndex":
        return {"Fd": obj.Fd, "G": obj.params[0], "S": obj.params[1], "_meta": (obj.id_base, obj.config)}
    names = [n for n in ("blob", "centroids", "codes", "residuals", "scales", "cutoffs", "weights", "offsets", "clamp0", "lengths") if hasattr(obj, n)]
    return dict({n: getattr(obj, n) for n in names}, _meta=(obj.id_base, getattr(obj, "bits", None)))


def assert_same_object(got, want):
    assert type(got) is type(want)
    a, b = _tensors(got), _tensors(want)
    assert a.keys() == b.keys() and a["_meta"] == b["_meta"]
    for name in a:
        if name == "_meta":
            continue
        x, y = a[name], b[name]
        assert (x is None) == (y is None), name
        if x is not None:
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device, name
            assert torch.equal(x.reshape(-1).view(torch.uint8), y.reshape(-1).view(torch.uint8)), name


@pytest.mark.parametrize("name", ["PackedCorpus", "PackedCorpus-f32-w40", "Int8Index", "BinaryIndex", "CentroidIndex", "FdeIndex", "ResidualCorpus"])
def test_round_trip_of_every_frozen_class(amd, tmp_path, name):
    obj = _frozen_objects(amd)[name]
    path = str(tmp_path / "x.msim")
    obj.save(path, chunk_bytes=4096)                                       # tensors end mid-chunk
    assert not os.path.exists(path + ".tmp")
    header = amd.verify_file(path)
    assert header["kind"] == type(obj).__name__ and header["abi"] == 22 and header["chunk_bytes"] == 4096
    assert os.path.getsize(path) == header["file_bytes"] and all(e["offset"] % 4096 == 0 for e in header["tensors"])
    assert_same_object(amd.load(path, "cpu"), obj)                         # dispatch on kind
    assert_same_object(type(obj).load(path, "cpu", verify=False), obj)
    other = amd.BinaryIndex if name != "BinaryIndex" else amd.Int8Index
    with pytest.raises(amd.ShardFileError, match="not a"):
        other.load(path, "cpu")
    if name == "ResidualCorpus":                                           # .index shares codes and centroids, as __init__ builds it
        rc = amd.load(path, "cpu")
        assert rc.index.codes.data_ptr() == rc.codes.data_ptr() and rc.index.centroids.data_ptr() == rc.centroids.data_ptr()
    if name == "FdeIndex":                                                 # the parameters come from the file, not from the seed
        assert not torch.equal(amd.load(path, "cpu").params[0], obj.config.params()[0])


def test_the_file_holds_json_and_bytes_only(amd, tmp_path):
    pc, _ = _corpus(amd)
    path = str(tmp_path / "x.msim")
    amd.save(pc, path, chunk_bytes=4096)
    raw = open(path, "rb").read()
    magic, version, zero, hlen = struct.unpack("<8sIIQ", raw[:24])
    assert (magic, version, zero) == (b"MSIMSHRD", 1, 0)
    header = json.loads(raw[24:24 + hlen].decode("utf-8"))
    assert raw[24 + hlen:header["tensors"][0]["offset"]].strip(b"\0") == b""
    blob = next(e for e in header["tensors"] if e["name"] == "blob")
    assert blob["role"] == "rows" and blob["dtype"] == "bfloat16" and blob["shape"] == list(pc.blob.shape)
    assert raw[blob["offset"]:blob["offset"] + blob["nbytes"]] == pc.blob.view(torch.uint8).numpy().tobytes()
    for c, pair in enumerate(blob["chunks"]):                              # every chunk's digest is the contract's, with pos = its offset
        part = raw[blob["offset"] + c * 4096:blob["offset"] + min(blob["nbytes"], (c + 1) * 4096)]
        assert tuple(int(v, 16) for v in pair) == dt.digest(part, c * 4096)
    assert tuple(int(v, 16) for v in blob["digest"]) == dt.digest(raw[blob["offset"]:blob["offset"] + blob["nbytes"]])
    assert b"pickle" not in raw and not raw.startswith(b"\x80") and b"PK" != raw[:2]


def test_chunk_size_does_not_change_a_tensor_digest(amd, tmp_path):
    rc = _frozen_objects(amd)["ResidualCorpus"]
    a, b = str(tmp_path / "a.msim"), str(tmp_path / "b.msim")
    rc.save(a, chunk_bytes=4096)
    rc.save(b, chunk_bytes=65536)
    ha, hb = amd.verify_file(a), amd.verify_file(b)
    assert {e["name"]: e["digest"] for e in ha["tensors"]} == {e["name"]: e["digest"] for e in hb["tensors"]}
    assert [len(e["chunks"]) for e in ha["tensors"]] != [len(e["chunks"]) for e in hb["tensors"]]
    with pytest.raises(ValueError, match="chunk_bytes"):
        rc.save(a, chunk_bytes=1000)


def test_a_flipped_data_byte_fails_verification_and_names_the_chunk(amd, tmp_path):
    pc, _ = _corpus(amd)
    path = str(tmp_path / "x.msim")
    pc.save(path, chunk_bytes=4096)
    amd.verify_file(path)
    blob = next(e for e in amd.verify_file(path)["tensors"] if e["name"] == "blob")
    with open(path, "r+b") as f:
        f.seek(blob["offset"] + 2 * 4096 + 17)
        byte = f.read(1)
        f.seek(-1, 1)
        f.write(bytes([byte[0] ^ 0x01]))
    for call in (lambda: amd.verify_file(path), lambda: amd.load(path, "cpu")):
        with pytest.raises(amd.ShardFileError, match=r"'blob', chunk 2 \(bytes 8192 \.\. 12288"):
            call()
    assert torch.equal(amd.load(path, "cpu", verify=False).offsets, pc.offsets)


def test_bad_files_are_refused_before_any_tensor_is_allocated(amd, tmp_path, monkeypatch):
    from colpali_amd import persist

    pc, _ = _corpus(amd)
    good = str(tmp_path / "good.msim")
    pc.save(good, chunk_bytes=4096)
    raw = open(good, "rb").read()
    hlen = struct.unpack("<Q", raw[16:24])[0]

    def variant(name, data):
        p = str(tmp_path / name)
        open(p, "wb").write(data)
        return p

    def reheadered(**changes):
        header = json.loads(raw[24:24 + hlen].decode())
        header.update(changes)
        blob = json.dumps(header, sort_keys=True, separators=(",", ":")).encode()
        assert 24 + len(blob) <= 4096
        return raw[:16] + struct.pack("<Q", len(blob)) + blob + b"\0" * (4096 - 24 - len(blob)) + raw[4096:]

    bad = {
        "truncated": (variant("t.msim", raw[:-4096]), "truncated"),
        "cut inside the header": (variant("h.msim", raw[:100]), "does not fit"),
        "wrong magic": (variant("m.msim", b"MSIMSHRX" + raw[8:]), "magic"),
        "format_version 2": (variant("v.msim", raw[:8] + struct.pack("<I", 2) + raw[12:]), "format_version 2 is newer"),
        "unknown kind": (variant("k.msim", reheadered(kind="Mystery")), "unknown kind 'Mystery'"),
        "not json": (variant("j.msim", raw[:24] + b"{" * hlen + raw[24 + hlen:]), "JSON"),
    }

    def no_alloc(*a, **kw):
        raise AssertionError("a tensor was allocated for a file that must be refused first")

    monkeypatch.setattr(persist, "_alloc", no_alloc)
    for what, (path, match) in bad.items():
        for call in (amd.load, amd.PackedCorpus.load):
            with pytest.raises(amd.ShardFileError, match=match):
                call(path, "cpu")
        with pytest.raises(amd.ShardFileError, match=match):
            amd.verify_file(path)


def test_a_failed_save_leaves_nothing_and_keeps_the_older_file(amd, tmp_path, monkeypatch):
    from colpali_amd import persist

    pc, _ = _corpus(amd)
    other, _ = _corpus(amd, clamp=False, id_base=99)
    path, fresh = str(tmp_path / "x.msim"), str(tmp_path / "never.msim")
    pc.save(path, chunk_bytes=4096)
    before = open(path, "rb").read()
    real, calls = persist._write_chunk, []

    def failing(fd, buf, offset):
        calls.append(offset)
        if len(calls) == 3:
            raise OSError("disk full (injected)")
        return real(fd, buf, offset)

    monkeypatch.setattr(persist, "_write_chunk", failing)
    for target in (path, fresh):
        calls.clear()
        with pytest.raises(OSError, match="injected"):
            other.save(target, chunk_bytes=4096)
        assert len(calls) == 3 and not os.path.exists(target + ".tmp")
    assert not os.path.exists(fresh) and open(path, "rb").read() == before
    monkeypatch.setattr(persist, "_write_chunk", real)
    other.save(path, chunk_bytes=4096)                                     # and a good save replaces it
    assert amd.load(path, "cpu").id_base == 99


# ------------------------------------------------------------------------------------------------------------------ range loads
@pytest.mark.parametrize("lo,hi", [(0, 5), (1, 3), (2, 2), (4, 5), (0, 1)])
def test_range_load_equals_the_pack_of_those_pages(amd, tmp_path, lo, hi):
    pc, ps = _corpus(amd, clamp=False)
    path = str(tmp_path / "x.msim")
    pc.save(path, chunk_bytes=4096)                                        # page 2 starts inside chunk 2: the cuts fall inside chunks
    got = amd.PackedCorpus.load(path, "cpu", pages=(lo, hi))
    assert got.id_base == 7 + lo and len(got) == hi - lo
    if lo == hi:
        assert got.blob.shape == (1, 128) and not got.blob.any() and got.offsets.tolist() == [0] and got.clamp0 is None
        return
    assert_same_object(got, amd.pack_passages(ps[lo:hi], "cpu", batch_size=None, id_base=7 + lo))


def test_range_load_cuts_every_role_of_every_class(amd, tmp_path):
    objs = _frozen_objects(amd)
    off = objs["PackedCorpus"].offsets.tolist()
    lo, hi = 1, 4
    for name, obj in objs.items():
        path = str(tmp_path / (name + ".msim"))
        obj.save(path, chunk_bytes=4096)
        got = amd.load(path, "cpu", pages=(lo, hi))
        assert type(got) is type(obj) and len(got) == hi - lo and got.id_base == obj.id_base + lo
        if name == "FdeIndex":
            assert torch.equal(got.Fd, obj.Fd[lo:hi]) and torch.equal(got.params[0], obj.params[0]) and got.config == obj.config
            continue
        o = obj.offsets.tolist()
        assert got.offsets.tolist() == [x - o[lo] for x in o[lo:hi + 1]] and torch.equal(got.lengths, obj.lengths[lo:hi])
        assert (got.clamp0 is None) == (obj.clamp0 is None) and (obj.clamp0 is None or torch.equal(got.clamp0, obj.clamp0[lo:hi]))
        for attr in ("blob", "codes", "residuals"):
            if hasattr(obj, attr):
                a, b = getattr(got, attr), getattr(obj, attr)[o[lo]:o[hi]]
                assert a.dtype == b.dtype and torch.equal(a.reshape(-1).view(torch.uint8), b.reshape(-1).view(torch.uint8)), (name, attr)
        if hasattr(obj, "scales"):
            assert torch.equal(got.scales, obj.scales[lo:hi])
        if hasattr(obj, "centroids"):
            assert torch.equal(got.centroids, obj.centroids)
    assert off[lo] % 16 != 0                                               # (the cut is not on a chunk boundary of any of them)
    with pytest.raises(ValueError, match="outside"):
        amd.load(str(tmp_path / "PackedCorpus.msim"), "cpu", pages=(2, 6))
    # a flipped byte in a chunk the range only touches is still caught: covering chunks are verified whole
    path = str(tmp_path / "PackedCorpus.msim")
    blob = next(e for e in amd.verify_file(path)["tensors"] if e["name"] == "blob")
    with open(path, "r+b") as f:
        f.seek(blob["offset"] + 3)                                         # page 0's bytes, in the chunk page 1 starts in
        f.write(b"\xff")
    with pytest.raises(amd.ShardFileError, match="'blob', chunk 0"):
        amd.load(path, "cpu", pages=(lo, hi))


# ------------------------------------------------------------------------------------------------------------------ live shards
def test_a_live_corpus_on_the_host_keeps_its_slots(amd, tmp_path):
    g = torch.Generator().manual_seed(12)
    live = amd.LiveCorpus(400, 12, "cpu", torch.float32, 40, id_base=30)
    assert live.add([_rows(g, n, torch.float32, 40) for n in (3, 50, 1, 20)]).tolist() == [30, 31, 32, 33]
    live.delete([31, 33])
    path = str(tmp_path / "live.msim")
    live.save(path, chunk_bytes=4096)
    with pytest.raises(ValueError, match="smaller"):
        amd.LiveCorpus.load(path, "cpu", capacity_rows=73)
    with pytest.raises(ValueError, match="smaller"):
        amd.load(path, "cpu", capacity_docs=3)
    with pytest.raises(ValueError, match="pages="):
        amd.load(path, "cpu", pages=(0, 2))
    for caps in ({}, dict(capacity_rows=1000, capacity_docs=40)):
        got = amd.LiveCorpus.load(path, "cpu", **caps)
        assert (got.capacity_rows, got.capacity_docs) == (caps.get("capacity_rows", 400), caps.get("capacity_docs", 12))
        assert (got.n_slots, got.rows_used, got.id_base, got.dtype, got.dim, got.width) == (4, 74, 30, torch.float32, 40, 40)
        assert torch.equal(got.blob[:74], live.blob[:74]) and torch.equal(got.offsets[:5], live.offsets[:5])
        assert got.alive[:4].tolist() == [1, 0, 1, 0] and got._lengths[:4].tolist() == [3, 50, 1, 20] and got.n_live == 2
        with pytest.raises(KeyError):
            got.delete([31])                                               # deleted ids stay gone
        assert got.add([_rows(g, 2, torch.float32, 40)]).tolist() == [34]  # the next id is the saved shard's
    assert amd.verify_file(path)["meta"]["capacity_rows"] == 400


# ----------------------------------------------------------------------------------------------------------------------- golden
def test_the_committed_format_1_file_still_loads(amd):
    """tests/golden/persist_v1_packed.msim was written by `PackedCorpus.save(chunk_bytes=4096)` (tests/golden/make_persist_golden.py)
    and is never rewritten: a change that cannot read it has changed format 1."""
    path = os.path.join(GOLDEN, "persist_v1_packed.msim")
    want = np.load(os.path.join(GOLDEN, "persist_v1_packed.npz"))
    header = amd.verify_file(path)
    assert header["kind"] == "PackedCorpus" and header["chunk_bytes"] == 4096
    pc = amd.load(path, "cpu")
    assert pc.blob.dtype == torch.bfloat16 and pc.id_base == int(want["id_base"])
    np.testing.assert_array_equal(pc.blob.view(torch.int16).numpy().view(np.uint16), want["blob_bits"])
    np.testing.assert_array_equal(pc.offsets.numpy(), want["offsets"])
    np.testing.assert_array_equal(pc.clamp0.numpy(), want["clamp0"])
    np.testing.assert_array_equal(pc.lengths.numpy(), want["lengths"])
    assert {e["name"]: e["digest"] for e in header["tensors"]} == json.loads(str(want["digests"]))
