"""Save and load shards and indexes: one flat, versioned, self-describing file per object, verified by an on-device digest.

    bytes 0 .. 23      magic "MSIMSHRD", format_version (uint32), 0 (uint32), header length in bytes (uint64), little-endian
    bytes 24 ..        the header: UTF-8 JSON, zero-padded to a multiple of 4096 bytes
    then               every tensor's raw little-endian bytes, each starting on a multiple of 4096

The header holds `kind` (the class), `abi`, `chunk_bytes`, `file_bytes`, the scalar metadata (`meta`) and the tensor table: per
tensor its name, dtype, shape, role (`rows` | `pages` | `offsets` | `whole`), file offset, `nbytes`, one digest pair per chunk of
`chunk_bytes` (include/maxsim.h: msim_digest, with `pos` the chunk's byte offset in the tensor) and the tensor's own digest -- their
sum, which therefore does not depend on `chunk_bytes`.  No pickle anywhere: a loader reads JSON and bytes only.

A tensor on the GPU is streamed through the pinned double buffer of the drop-in path (corpus._Staging), a chunk at a time: `save`
digests the source in HBM, copies it to one pinned half and writes it out while the next chunk is on its way; `load` reads into a
pinned half, uploads, and digests what has landed in HBM -- one read-back at the end decides.  Tensors on the CPU take the same
route through msim_digest_host, so the format needs no GPU.  The digest detects corruption, truncation and misplacement; it is not
a cryptographic hash.
"""
from __future__ import annotations

import json
import os
import struct
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from .binary_index import BinaryIndex
from .centroid import CentroidIndex
from .corpus import PackedCorpus, _staging
from .fde import FdeConfig, FdeIndex
from .fde_wide import FdeWideIndex
from .fp4_index import Fp4Index
from .fp4_wide_index import Fp4WideIndex
from .int8_index import Int8Index
from .live import LiveCorpus
from .live_residual import LiveResidualCorpus
from .residual import ResidualCorpus
from .residual_wide import CentroidWideIndex, ResidualWideCorpus

MAGIC = b"MSIMSHRD"
FORMAT_VERSION = 1
ALIGN = 4096
DEFAULT_CHUNK_BYTES = 64 << 20
_PRE = struct.Struct("<8sIIQ")
_MASK = (1 << 64) - 1

_DTYPES = {"bfloat16": torch.bfloat16, "float16": torch.float16, "float32": torch.float32, "int8": torch.int8, "uint8": torch.uint8,
           "uint16": torch.uint16, "int32": torch.int32, "int64": torch.int64}
_DTYPE_NAMES = {v: k for k, v in _DTYPES.items()}

# per kind: the tensors in file order, (attribute, role).  `rows` tensors are cut at offsets[lo] .. offsets[hi] by a range load
# (at lo .. hi where the kind has no offsets), `pages` tensors at lo .. hi, `offsets` is rebased, `whole` is kept.
_FP4_FIELDS = (("codes", "rows"), ("scales", "rows"), ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))
_CENT_FIELDS = (("centroids", "whole"), ("codes", "rows"), ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))
_RES_FIELDS = (("centroids", "whole"), ("codes", "rows"), ("residuals", "rows"), ("cutoffs", "whole"), ("weights", "whole"),
               ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))
_FROZEN = {
    "PackedCorpus": (PackedCorpus, (("blob", "rows"), ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))),
    "Int8Index": (Int8Index, (("codes", "rows"), ("scales", "pages"), ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))),
    "BinaryIndex": (BinaryIndex, (("codes", "rows"), ("offsets", "offsets"), ("clamp0", "pages"), ("lengths", "pages"))),
    "Fp4Index": (Fp4Index, _FP4_FIELDS),
    "Fp4WideIndex": (Fp4WideIndex, _FP4_FIELDS),
    "CentroidIndex": (CentroidIndex, _CENT_FIELDS),
    "CentroidWideIndex": (CentroidWideIndex, _CENT_FIELDS),
    "FdeIndex": (FdeIndex, (("Fd", "rows"), ("G", "whole"), ("S", "whole"))),
    "FdeWideIndex": (FdeWideIndex, (("Fd", "rows"), ("G", "whole"), ("S", "whole"))),
    "ResidualCorpus": (ResidualCorpus, _RES_FIELDS),
    "ResidualWideCorpus": (ResidualWideCorpus, _RES_FIELDS),
}
_LIVE = {"LiveCorpus": LiveCorpus, "LiveResidualCorpus": LiveResidualCorpus}
_HOST_TENSORS = ("lengths",)          # host tensors by contract: loaded to the host whatever the device
_FDE_FIELDS = ("reps", "ksim", "dproj", "seed", "fill_empty")


class ShardFileError(ValueError):
    """The file is not a shard file this library can load, or its bytes do not match its digests."""


def _round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def _alloc(shape, dtype: torch.dtype, device, zero: bool = False) -> torch.Tensor:
    """a tensor of any file dtype, allocated as bytes (uint16 has few device kernels of its own)"""
    nbytes = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    raw = (torch.zeros if zero else torch.empty)((nbytes,), dtype=torch.uint8, device=device)
    return raw.view(dtype).reshape(list(shape))


def _hex(pair) -> list:
    return [f"{int(v) & _MASK:016x}" for v in pair]


# ---------------------------------------------------------------------------------------------------------------------- digest
def _digest_raw(ptr: int, nbytes: int, pos: int, acc: torch.Tensor, device: torch.device) -> None:
    L = _lib.lib()
    if device.type == "cuda":
        with torch.cuda.device(device):
            rc = L.msim_digest(ptr, nbytes, pos, acc.data_ptr(), _lib.current_stream_handle(device))
        _lib.check(rc, "msim_digest")
    else:
        _lib.check(L.msim_digest_host(ptr, nbytes, pos, acc.data_ptr()), "msim_digest_host")


def _byte_view(t: torch.Tensor) -> torch.Tensor:
    """the tensor's bytes as a flat uint8 view (a copy only where it is not contiguous or not 8-byte aligned)"""
    t = t.detach()
    b = (t if t.is_contiguous() else t.contiguous()).reshape(-1).view(torch.uint8)
    return b.clone() if b.data_ptr() % 8 else b


def digest(t: torch.Tensor, pos: int = 0, acc: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Add the digest of the bytes of `t` (include/maxsim.h: msim_digest on the GPU, msim_digest_host on the CPU), taken as the
    part that starts at byte `pos` (a multiple of 8) of some object, into `acc` -- an int64 [2] tensor on the device of `t` holding
    the two uint64 lanes; None: a zeroed one.  Returns `acc`.  On the GPU: asynchronous on torch's current stream, no
    synchronisation, hipGraph-capturable when `acc` is given."""
    b = _byte_view(t)
    if acc is None:
        acc = torch.zeros((2,), dtype=torch.int64, device=b.device)
    elif acc.dtype != torch.int64 or acc.shape != (2,) or acc.device != b.device or not acc.is_contiguous():
        raise ValueError(f"acc must be a contiguous int64 [2] tensor on {b.device}")
    _digest_raw(b.data_ptr(), b.numel(), int(pos), acc, b.device)
    return acc


# ------------------------------------------------------------------------------------------------------------------------ save
def _write_chunk(fd: int, buf, offset: int) -> None:
    """one chunk of tensor bytes -> the file (the whole of it: pwrite may write less than it was handed)"""
    mv = memoryview(buf).cast("B")
    done = 0
    while done < len(mv):
        done += os.pwrite(fd, mv[done:], offset + done)


def _pinned_halves(st, want: int) -> Tuple[int, torch.Tensor]:
    """(piece, buffer): two pieces of `piece` bytes at 0 and `piece` of the staging buffer, idle (earlier uploads have left it)"""
    half = st._halves(want)
    for ev in st.events:
        if ev is not None:
            ev.synchronize()
    return min(want, half // ALIGN * ALIGN), st.buf


def _stream_out(fd: int, b: torch.Tensor, entry: dict, chunk_bytes: int) -> None:
    """the bytes `b` of one tensor -> the file at entry["offset"]; fills in the entry's digests"""
    nbytes, dev = b.numel(), b.device
    n_chunks = (nbytes + chunk_bytes - 1) // chunk_bytes
    table = torch.zeros((max(n_chunks, 1), 2), dtype=torch.int64, device=dev)
    chunks = [(c * chunk_bytes, min(nbytes, (c + 1) * chunk_bytes)) for c in range(n_chunks)]
    if dev.type != "cuda":
        host = b.numpy()
        for c, (c0, c1) in enumerate(chunks):
            _digest_raw(b.data_ptr() + c0, c1 - c0, c0, table[c], dev)
            _write_chunk(fd, host[c0:c1], entry["offset"] + c0)
    elif n_chunks:
        st = _staging.of(dev)
        with st.lock, torch.cuda.device(dev):
            piece, pinned = _pinned_halves(st, chunk_bytes)
            stream = torch.cuda.current_stream(dev)
            pending, h = None, 0

            def flush(p):
                host, off, ev = p
                ev.synchronize()
                _write_chunk(fd, host.numpy(), off)

            try:
                for c, (c0, c1) in enumerate(chunks):
                    _digest_raw(b.data_ptr() + c0, c1 - c0, c0, table[c], dev)
                    for p0 in range(c0, c1, piece):
                        p1 = min(c1, p0 + piece)
                        host = pinned[h * piece:h * piece + (p1 - p0)]
                        host.copy_(b[p0:p1], non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(stream)
                        if pending is not None:           # written while the copy just queued is in flight
                            flush(pending)
                        pending = (host, entry["offset"] + p0, ev)
                        h ^= 1
                if pending is not None:
                    flush(pending)
            finally:
                stream.synchronize()                      # never leave with a copy still writing the pinned halves
    got = table.cpu().numpy().astype(np.uint64)[:n_chunks]
    entry["chunks"] = [_hex(row) for row in got]
    entry["digest"] = _hex(got.sum(axis=0, dtype=np.uint64)) if n_chunks else _hex((0, 0))


def _header_bytes(header: dict) -> bytes:
    return json.dumps(header, sort_keys=True, separators=(",", ":")).encode("utf-8")


def _write_file(path: str, kind: str, meta: dict, tensors, chunk_bytes: int) -> None:
    chunk_bytes = int(chunk_bytes)
    if chunk_bytes < ALIGN or chunk_bytes % ALIGN:
        raise ValueError(f"chunk_bytes must be a positive multiple of {ALIGN} (got {chunk_bytes})")
    views, entries = [], []
    for name, role, t in tensors:
        if t is None:
            continue
        if t.dtype not in _DTYPE_NAMES:
            raise NotImplementedError(f"{kind}.{name}: dtype {t.dtype} has no place in the file format")
        if name in _HOST_TENSORS:
            t = t.cpu()
        if t.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("save synchronises with the host: it cannot run under stream capture")
        b = _byte_view(t)
        n_chunks = (b.numel() + chunk_bytes - 1) // chunk_bytes
        views.append(b)
        entries.append(dict(name=name, role=role, dtype=_DTYPE_NAMES[t.dtype], shape=[int(s) for s in t.shape], offset=0,
                            nbytes=int(b.numel()), chunks=[_hex((0, 0))] * n_chunks, digest=_hex((0, 0))))
    header = dict(kind=kind, abi=_lib.ABI_VERSION, chunk_bytes=chunk_bytes, file_bytes=0, meta=meta, tensors=entries)
    data_start = 0
    while True:          # the offsets are part of the header whose length places them: settle both (digests have a fixed width)
        start = _round_up(_PRE.size + len(_header_bytes(header)), ALIGN)
        if start == data_start:
            break
        data_start = off = start
        for e in entries:
            e["offset"] = off
            off += _round_up(e["nbytes"], ALIGN)
        header["file_bytes"] = off
    path = os.fspath(path)
    tmp = path + ".tmp"
    fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        os.ftruncate(fd, header["file_bytes"])
        for b, e in zip(views, entries):
            _stream_out(fd, b, e, chunk_bytes)
        blob = _header_bytes(header)
        if _round_up(_PRE.size + len(blob), ALIGN) != data_start:
            raise RuntimeError("the header outgrew the space reserved for it")
        os.pwrite(fd, _PRE.pack(MAGIC, FORMAT_VERSION, 0, len(blob)) + blob, 0)
        os.fsync(fd)
    except BaseException:
        os.close(fd)
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    os.close(fd)
    os.replace(tmp, path)


def _kind_of(obj) -> str:
    for kind, (cls, _) in _FROZEN.items():
        if type(obj) is cls:
            return kind
    for kind, cls in _LIVE.items():
        if type(obj) is cls:
            return kind
    raise TypeError(f"save takes a {', '.join(list(_FROZEN) + list(_LIVE))}, not a {type(obj).__name__}")


def save(obj, path, *, chunk_bytes: int = DEFAULT_CHUNK_BYTES) -> None:
    """Write `obj` -- a `PackedCorpus`, `Int8Index`, `BinaryIndex`, `Fp4Index`, `Fp4WideIndex`, `CentroidIndex`, `CentroidWideIndex`, `FdeIndex`, `FdeWideIndex`, `ResidualCorpus`, `ResidualWideCorpus`, `LiveCorpus` or
    `LiveResidualCorpus` -- to `path` (see the module docstring).  Written to `path + ".tmp"`, fsynced and renamed: a failed save
    leaves nothing under `path` and an older file there untouched.  Holds two pinned chunks of host memory at most, whatever the
    object's size.  Synchronises with the host; raises under stream capture."""
    kind = _kind_of(obj)
    if kind in _FROZEN:
        meta = dict(id_base=int(obj.id_base))
        if kind in ("FdeIndex", "FdeWideIndex"):
            G, S = obj.params
            meta["config"] = {f: getattr(obj.config, f) for f in _FDE_FIELDS}
            tensors = [("Fd", "rows", obj.Fd), ("G", "whole", G), ("S", "whole", S)]
        else:
            if kind in ("ResidualCorpus", "ResidualWideCorpus"):
                meta["bits"] = int(obj.bits)
            tensors = [(name, role, getattr(obj, name)) for name, role in _FROZEN[kind][1]]
    else:
        obj._sync_host()
        n, r = obj.n_slots, obj.rows_used
        meta = dict(id_base=int(obj.id_base), capacity_rows=int(obj.capacity_rows), capacity_docs=int(obj.capacity_docs), n_slots=int(n),
                    rows_used=int(r), dtype=_DTYPE_NAMES[obj.dtype])
        tail = [("offsets", "offsets", obj.offsets[:n + 1]), ("alive", "pages", obj.alive[:n]),
                ("lengths", "pages", torch.from_numpy(obj._lengths[:n].copy()))]
        if kind == "LiveCorpus":
            meta.update(dim=int(obj.dim), width=int(obj.width))
            tensors = [("blob", "rows", obj.blob[:r])] + tail
        else:
            meta.update(bits=int(obj.bits))
            tensors = [("centroids", "whole", obj.centroids), ("cutoffs", "whole", obj.cutoffs), ("weights", "whole", obj.weights),
                       ("codes", "rows", obj.codes[:r]), ("residuals", "rows", obj.residuals[:r])] + tail
    _write_file(path, kind, meta, tensors, chunk_bytes)


# ------------------------------------------------------------------------------------------------------------------------ load
def _read_exact(fd: int, buf, offset: int, what: str) -> None:
    mv = memoryview(buf).cast("B")
    done = 0
    while done < len(mv):
        got = os.preadv(fd, [mv[done:]], offset + done)
        if got <= 0:
            raise ShardFileError(f"{what}: the file ends at byte {offset + done}")
        done += got


def _read_header(fd: int, path: str) -> dict:
    """The checked header.  Everything that can be refused without reading a tensor is refused here, before anything is allocated."""
    size = os.fstat(fd).st_size
    if size < _PRE.size:
        raise ShardFileError(f"{path}: {size} bytes is too short for a shard file")
    pre = bytearray(_PRE.size)
    _read_exact(fd, pre, 0, path)
    magic, version, _, hlen = _PRE.unpack(bytes(pre))
    if magic != MAGIC:
        raise ShardFileError(f"{path}: wrong magic {magic!r} (a shard file starts with {MAGIC!r})")
    if version > FORMAT_VERSION:
        raise ShardFileError(f"{path}: format_version {version} is newer than this library reads ({FORMAT_VERSION})")
    if version < 1 or hlen < 2 or _PRE.size + hlen > size:
        raise ShardFileError(f"{path}: a header of {hlen} bytes (format_version {version}) does not fit the file's {size} bytes")
    raw = bytearray(hlen)
    _read_exact(fd, raw, _PRE.size, path)
    try:
        header = json.loads(raw.decode("utf-8"))
        kind, chunk_bytes, entries = header["kind"], int(header["chunk_bytes"]), header["tensors"]
        file_bytes, _ = int(header["file_bytes"]), header["meta"]["id_base"]
    except (ValueError, KeyError, TypeError) as exc:
        raise ShardFileError(f"{path}: the header is not the JSON of a shard file ({exc})") from None
    if kind not in _FROZEN and kind not in _LIVE:
        raise ShardFileError(f"{path}: unknown kind {kind!r}")
    if chunk_bytes < ALIGN or chunk_bytes % ALIGN:
        raise ShardFileError(f"{path}: chunk_bytes={chunk_bytes} is not a positive multiple of {ALIGN}")
    if file_bytes != size:
        raise ShardFileError(f"{path}: the header describes a file of {file_bytes} bytes, this one has {size} (truncated?)")
    end = _round_up(_PRE.size + hlen, ALIGN)
    try:
        for e in entries:
            name, dt, off, nbytes = e["name"], _DTYPES.get(e["dtype"]), int(e["offset"]), int(e["nbytes"])
            if dt is None or e["role"] not in ("rows", "pages", "offsets", "whole"):
                raise ShardFileError(f"{path}: tensor {name!r} has an unknown dtype or role ({e['dtype']!r}, {e['role']!r})")
            want = int(np.prod(e["shape"], dtype=np.int64)) * torch.empty((), dtype=dt).element_size()
            n_chunks = (nbytes + chunk_bytes - 1) // chunk_bytes
            if any(int(s) < 0 for s in e["shape"]) or want != nbytes or off % ALIGN or off < end or off + nbytes > size:
                raise ShardFileError(f"{path}: tensor {name!r} ({nbytes} bytes at {off}, shape {e['shape']}) disagrees with its shape or "
                                     f"with the file's {size} bytes")
            if len(e["chunks"]) != n_chunks or len(e["digest"]) != 2 or any(len(c) != 2 for c in e["chunks"]):
                raise ShardFileError(f"{path}: tensor {name!r} carries {len(e['chunks'])} chunk digests, its size asks for {n_chunks}")
            e["_want"] = np.array([[int(v, 16) for v in c] for c in e["chunks"]], dtype=np.uint64).reshape(n_chunks, 2)
            if [f"{int(v):016x}" for v in e["_want"].sum(axis=0, dtype=np.uint64)] != [str(v) for v in e["digest"]]:
                raise ShardFileError(f"{path}: the digest of tensor {name!r} is not the sum of its chunks' digests")
            e["offset"], e["nbytes"], e["shape"] = off, nbytes, [int(x) for x in e["shape"]]
            end = off + _round_up(nbytes, ALIGN)
    except (KeyError, TypeError, ValueError) as exc:
        if isinstance(exc, ShardFileError):
            raise
        raise ShardFileError(f"{path}: malformed tensor table ({exc})") from None
    return header


class _Reader:
    """One open file: fetches (parts of) tensors to the host or to the GPU and keeps what is still to be verified."""

    def __init__(self, path, verify: bool):
        self.path = os.fspath(path)
        self.fd = os.open(self.path, os.O_RDONLY)
        try:
            self.header = _read_header(self.fd, self.path)
        except BaseException:
            os.close(self.fd)
            raise
        self.verify = verify
        self.chunk_bytes = int(self.header["chunk_bytes"])
        self.entries = {e["name"]: e for e in self.header["tensors"]}
        self._pending = []            # (entry, first chunk, device table int64 [k, 2]) read back once, in finish()

    def close(self) -> None:
        if self.fd is not None:
            os.close(self.fd)
            self.fd = None

    def _mismatch(self, e: dict, c: int) -> ShardFileError:
        c0 = c * self.chunk_bytes
        c1 = min(e["nbytes"], c0 + self.chunk_bytes)
        return ShardFileError(f"{self.path}: tensor {e['name']!r}, chunk {c} (bytes {c0} .. {c1} of the tensor, {e['offset'] + c0} .. "
                              f"{e['offset'] + c1} of the file) does not match its digest")

    def fetch(self, e: dict, dst: torch.Tensor, want0: int = 0, want1: Optional[int] = None) -> None:
        """Bytes want0 .. want1 of tensor `e` -> `dst` (a flat uint8 view of that length, on the host or the GPU).  The chunks that
        cover the range are read and verified WHOLE: straight into `dst` when the range is the tensor, else through a bounce buffer
        of two chunks from which the wanted part is copied."""
        nbytes, cb = e["nbytes"], self.chunk_bytes
        want1 = nbytes if want1 is None else want1
        if want1 <= want0:
            return
        full = want0 == 0 and want1 == nbytes
        dev, cuda = dst.device, dst.device.type == "cuda"
        c_lo, c_hi = want0 // cb, (want1 + cb - 1) // cb
        bounce = None if full else torch.empty((2 * cb,), dtype=torch.uint8, device=dev)
        table = torch.zeros((c_hi - c_lo, 2), dtype=torch.int64, device=dev) if self.verify else None
        what = f"{self.path}: tensor {e['name']!r}"

        def chunks():
            for c in range(c_lo, c_hi):
                c0, c1 = c * cb, min(nbytes, (c + 1) * cb)
                yield c, c0, c1, (dst[c0:c1] if full else bounce[(c & 1) * cb:(c & 1) * cb + (c1 - c0)])

        def landed(c, c0, c1, target):
            if self.verify:
                _digest_raw(target.data_ptr(), c1 - c0, c0, table[c - c_lo], dev)
                if not cuda and not np.array_equal(table[c - c_lo].numpy().astype(np.uint64), e["_want"][c]):
                    raise self._mismatch(e, c)
            if not full:
                a, b = max(c0, want0), min(c1, want1)
                dst[a - want0:b - want0].copy_(target[a - c0:b - c0])

        if not cuda:
            for c, c0, c1, target in chunks():
                _read_exact(self.fd, target.numpy(), e["offset"] + c0, what)
                landed(c, c0, c1, target)
            return
        st = _staging.of(dev)
        with st.lock, torch.cuda.device(dev):
            piece, pinned = _pinned_halves(st, cb)
            stream = torch.cuda.current_stream(dev)
            events, h = [None, None], 0
            try:
                for c, c0, c1, target in chunks():
                    for p0 in range(c0, c1, piece):
                        p1 = min(c1, p0 + piece)
                        if events[h] is not None:
                            events[h].synchronize()       # the upload before last has left this half
                        host = pinned[h * piece:h * piece + (p1 - p0)]
                        _read_exact(self.fd, host.numpy(), e["offset"] + p0, what)
                        target[p0 - c0:p1 - c0].copy_(host, non_blocking=True)
                        events[h] = torch.cuda.Event()
                        events[h].record(stream)
                        h ^= 1
                    landed(c, c0, c1, target)
            finally:
                for ev in events:
                    if ev is not None:
                        ev.synchronize()                  # never leave with an upload still reading the pinned halves
        if self.verify:
            self._pending.append((e, c_lo, table))

    def tensor(self, name: str, device, out: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None,
               keep_one: bool = False) -> Optional[torch.Tensor]:
        """Tensor `name` on `device` (None where the file has none): whole, into `out` when given, or its rows r0 .. r1 only
        (`keep_one`: an empty range gives one zero row, the valid pointer `pack_passages` keeps)."""
        e = self.entries.get(name)
        if e is None:
            return None
        dt, shape = _DTYPES[e["dtype"]], list(e["shape"])
        device = torch.device("cpu") if name in _HOST_TENSORS else torch.device(device)
        if rows is None:
            t = _alloc(shape, dt, device) if out is None else out
            if list(t.shape) != shape or t.dtype != dt or not t.is_contiguous():
                raise ShardFileError(f"{self.path}: tensor {name!r} is {e['dtype']} {shape}, the object it goes into expects {t.dtype} {list(t.shape)}")
            self.fetch(e, t.reshape(-1).view(torch.uint8))
            return t
        r0, r1 = rows
        if not shape or not 0 <= r0 <= r1 <= shape[0]:
            raise ShardFileError(f"{self.path}: rows {r0} .. {r1} (from the file's offsets) are outside tensor {name!r} of shape {shape}")
        row_bytes = e["nbytes"] // shape[0] if shape[0] else 0
        t = _alloc([max(r1 - r0, 1 if keep_one else 0)] + shape[1:], dt, device, zero=r1 == r0)
        self.fetch(e, t.reshape(-1).view(torch.uint8)[:(r1 - r0) * row_bytes], r0 * row_bytes, r1 * row_bytes)
        return t

    def finish(self) -> None:
        """the one read-back: every digest computed on the GPU against the header's"""
        pending, self._pending = self._pending, []
        if not pending:
            return
        got = torch.cat([t for _, _, t in pending]).cpu().numpy().astype(np.uint64)
        at = 0
        for e, c_lo, t in pending:
            for i in range(int(t.shape[0])):
                if not np.array_equal(got[at + i], e["_want"][c_lo + i]):
                    raise self._mismatch(e, c_lo + i)
            at += int(t.shape[0])


def _load_frozen(rd: _Reader, kind: str, device, pages):
    cls, spec = _FROZEN[kind]
    meta = rd.header["meta"]
    id_base = int(meta["id_base"])
    roles = {name: role for name, role in spec}
    key = "lengths" if "lengths" in rd.entries else "Fd"
    if key not in rd.entries:
        raise ShardFileError(f"{rd.path}: a {kind} without its {key!r} tensor")
    n = int(rd.entries[key]["shape"][0])
    got = {}
    if pages is None:
        for name, _ in spec:
            got[name] = rd.tensor(name, device)
    else:
        lo, hi = (int(p) for p in pages)
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"pages=({lo}, {hi}) is outside the file's {n} pages")
        r0, r1 = lo, hi
        if "offsets" in roles:
            off = rd.tensor("offsets", "cpu").numpy().astype(np.int64)
            r0, r1 = int(off[lo]), int(off[hi])
            got["offsets"] = torch.from_numpy((off[lo:hi + 1] - r0).astype(np.int32)).to(device)
        for name, role in spec:
            if role == "rows":
                got[name] = rd.tensor(name, device, rows=(r0, r1), keep_one="offsets" in roles)
            elif role == "whole":
                got[name] = rd.tensor(name, device)
            elif role == "pages":                          # small: read whole and verified on the host
                t = rd.tensor(name, "cpu")
                got[name] = None if t is None else (t[lo:hi].clone() if name in _HOST_TENSORS else t[lo:hi].to(device))
        id_base += lo
    rd.finish()
    try:
        if kind == "PackedCorpus":
            return PackedCorpus(blob=got["blob"], offsets=got["offsets"], clamp0=got["clamp0"], lengths=got["lengths"], id_base=id_base)
        if kind == "Int8Index":
            return Int8Index(got["codes"], got["scales"], got["offsets"], got["clamp0"], got["lengths"], id_base)
        if kind == "BinaryIndex":
            return BinaryIndex(got["codes"], got["offsets"], got["clamp0"], got["lengths"], id_base)
        if kind in ("Fp4Index", "Fp4WideIndex"):
            return cls(got["codes"], got["scales"], got["offsets"], got["clamp0"], got["lengths"], id_base)
        if kind in ("CentroidIndex", "CentroidWideIndex"):
            return cls(got["centroids"], got["codes"], got["offsets"], got["clamp0"], got["lengths"], id_base)
        if kind in ("FdeIndex", "FdeWideIndex"):
            return cls(got["Fd"], id_base, FdeConfig(**{f: meta["config"][f] for f in _FDE_FIELDS}), params=(got["G"], got["S"]))
        return cls(got["centroids"], got["codes"], got["residuals"], got["cutoffs"], got["weights"], got["offsets"], got["clamp0"],
                   got["lengths"], id_base, int(meta["bits"]))
    except (KeyError, AttributeError, TypeError) as exc:
        raise ShardFileError(f"{rd.path}: the tensors of this {kind} are incomplete ({exc})") from None


def _load_live(rd: _Reader, kind: str, device, capacity_rows, capacity_docs, kw):
    meta = rd.header["meta"]
    try:
        n, r = int(meta["n_slots"]), int(meta["rows_used"])
        cap_rows = int(meta["capacity_rows"]) if capacity_rows is None else int(capacity_rows)
        cap_docs = int(meta["capacity_docs"]) if capacity_docs is None else int(capacity_docs)
        dtype = _DTYPES[meta["dtype"]]
        id_base = int(meta["id_base"])
    except (KeyError, TypeError, ValueError) as exc:
        raise ShardFileError(f"{rd.path}: the metadata of this {kind} is incomplete ({exc})") from None
    if cap_rows < r or cap_docs < n:
        raise ValueError(f"capacity_rows={cap_rows}, capacity_docs={cap_docs} is smaller than what the saved shard uses ({r} rows, {n} slots)")
    if kind == "LiveCorpus":
        live = LiveCorpus(cap_rows, cap_docs, device, dtype, int(meta["dim"]), id_base, **kw)
        rd.tensor("blob", device, out=live.blob[:r])
    else:
        codec = [rd.tensor(name, device) for name in ("centroids", "cutoffs", "weights")]
        live = LiveResidualCorpus(*codec, int(meta["bits"]), cap_rows, cap_docs, id_base, **kw)
        rd.tensor("codes", device, out=live.codes[:r])
        rd.tensor("residuals", device, out=live.residuals[:r])
    offsets, alive, lengths = (rd.tensor(name, "cpu") for name in ("offsets", "alive", "lengths"))   # small: verified on the host
    rd.finish()
    if offsets is None or alive is None or lengths is None or offsets.shape != (n + 1,) or alive.shape != (n,) or lengths.shape != (n,):
        raise ShardFileError(f"{rd.path}: the slot table of this {kind} does not cover its {n} slots")
    live.offsets[:n + 1].copy_(offsets)
    live.alive[:n].copy_(alive)
    live._lengths[:n] = lengths.numpy()
    live._alive_h[:n] = alive.numpy().astype(bool)
    live.n_slots, live._rows_used = n, r
    return live


def load(path, device, *, verify: bool = True, pages: Optional[Tuple[int, int]] = None, capacity_rows: Optional[int] = None,
         capacity_docs: Optional[int] = None, expect=None, **kw):
    """The object saved at `path`, on `device` -- whichever class its `kind` names (`expect`: refuse any other).  With `verify`
    (default) every chunk is digested where it landed (in HBM by msim_digest; on the host by msim_digest_host) and compared with
    the header in one read-back at the end: a mismatch raises `ShardFileError` naming the tensor, the chunk and its byte range, and
    nothing is returned.  `pages=(lo, hi)` loads pages lo .. hi - 1 of a frozen class only (`id_base` becomes the saved one plus
    `lo`): one file serves any world size through `shard_range`.  A live shard keeps its saved capacity or takes a larger one
    (`capacity_rows`, `capacity_docs`), and further keywords go to its constructor (hooks, `bounce_bytes`); its slot ids,
    tombstones and the next id handed out are those of the saved shard.  An unknown kind, a newer format, a wrong magic and a
    header that disagrees with the file's size are refused before anything is allocated."""
    rd = _Reader(path, bool(verify))
    try:
        kind = rd.header["kind"]
        if expect is not None and (_FROZEN[kind][0] if kind in _FROZEN else _LIVE[kind]) is not expect:
            raise ShardFileError(f"{rd.path} holds a {kind}, not a {expect.__name__}")
        if kind in _LIVE:
            if pages is not None:
                raise ValueError(f"pages= cuts a frozen shard: a {kind} is loaded whole (its ids are slots)")
            return _load_live(rd, kind, device, capacity_rows, capacity_docs, kw)
        if capacity_rows is not None or capacity_docs is not None or kw:
            raise ValueError(f"capacity_rows, capacity_docs and constructor keywords go with a live shard, not a {kind}")
        return _load_frozen(rd, kind, torch.device(device), pages)
    finally:
        rd.close()


def verify_file(path) -> dict:
    """Check every chunk of the file at `path` against its digest with msim_digest_host: no GPU, one chunk of host memory.  Returns
    the header (kind, meta, the tensor table with its digests); raises `ShardFileError` as `load` does."""
    rd = _Reader(path, True)
    try:
        buf = torch.empty((rd.chunk_bytes,), dtype=torch.uint8)
        acc = torch.zeros((2,), dtype=torch.int64)
        for e in rd.header["tensors"]:
            for c in range(len(e["chunks"])):
                c0 = c * rd.chunk_bytes
                c1 = min(e["nbytes"], c0 + rd.chunk_bytes)
                _read_exact(rd.fd, buf.numpy()[:c1 - c0], e["offset"] + c0, f"{rd.path}: tensor {e['name']!r}")
                acc.zero_()
                _digest_raw(buf.data_ptr(), c1 - c0, c0, acc, buf.device)
                if not np.array_equal(acc.numpy().astype(np.uint64), e["_want"][c]):
                    raise rd._mismatch(e, c)
        for e in rd.header["tensors"]:
            del e["_want"]
        return rd.header
    finally:
        rd.close()
