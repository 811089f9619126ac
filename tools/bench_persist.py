"""Persistence (msim_digest, colpali_amd.save / load) on the headline shard; one JSON object on stdout (not part of bench.py).

    python tools/bench_persist.py [--out FILE] [--docs 125000 --doc-len 1024] [--file-gib 4] [--dir DIR] [--repeats 3]

Four things, every figure a median with its range:
  * digest: msim_digest over the whole resident shard, beside the read-only stream probe (tools/probe: msim_probe_stream) over
    the same bytes in the same run -- the probe, not the 8 TB/s peak, is what the digest is measured against -- and the digest of
    one 64 MiB chunk, which is what save and load launch.
  * pinned: this box's pinned H2D and D2H rates in 32 MiB pieces (the staging buffer's halves), as the drop-in leg reports them.
  * disk: the file system's own rate under --dir for a file of --file-gib: pwrite of 64 MiB pieces + fsync, and preadv of the
    same file, once from the page cache and once after posix_fadvise(DONTNEED) has asked the kernel to drop the file's pages.
  * save / load: PackedCorpus.save of the first --file-gib of the shard, PackedCorpus.load with and without verify (again warm
    and after DONTNEED), and verify_file (the host digest, one thread).
The file is removed at the end.  Nothing here is a pass/fail check.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_legs.common import make_shard  # noqa: E402
from bench_legs.resident import stream_ceiling  # noqa: E402

PIECE = 64 << 20


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def gbs(nbytes, seconds):
    """GB/s of `nbytes` moved in each of `seconds`: median, min, max"""
    return stats([nbytes / s / 1e9 for s in seconds])


def fs_type(path):
    """the file system `path` lives on, from /proc/mounts (longest mount point that is a prefix), or None"""
    try:
        real, best = os.path.realpath(path), ("", None)
        for line in open("/proc/mounts"):
            _, mnt, typ = line.split()[:3]
            if (real == mnt or real.startswith(mnt.rstrip("/") + "/")) and len(mnt) > len(best[0]):
                best = (mnt, typ)
        return best[1]
    except Exception:
        return None


def digest_leg(amd, t, repeats=7, warm=2):
    acc = torch.zeros(2, dtype=torch.int64, device=t.device)
    secs = []
    for i in range(warm + repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        amd.digest(t, 0, acc)
        b.record()
        torch.cuda.synchronize()
        if i >= warm:
            secs.append(a.elapsed_time(b) / 1e3)
    return gbs(t.numel() * t.element_size(), secs)


def pinned_leg(dev, nbytes=1 << 30, piece=32 << 20):
    host = torch.empty((piece,), dtype=torch.uint8, pin_memory=True)
    devb = torch.empty((piece,), dtype=torch.uint8, device=dev)
    out = {}
    for name, (dst, src) in {"h2d": (devb, host), "d2h": (host, devb)}.items():
        secs = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(nbytes // piece):
                dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        out[name] = gbs(nbytes, secs)
    return out


def drop_pages(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
    finally:
        os.close(fd)


def disk_leg(path, nbytes, repeats):
    buf = torch.zeros((PIECE,), dtype=torch.uint8).numpy()
    buf[::4096] = 7
    w, r_warm, r_cold = [], [], []

    def read_all():
        fd = os.open(path, os.O_RDONLY)
        t0 = time.perf_counter()
        for off in range(0, nbytes, PIECE):
            os.preadv(fd, [memoryview(buf)[:min(PIECE, nbytes - off)]], off)
        dt = time.perf_counter() - t0
        os.close(fd)
        return dt

    for _ in range(repeats):
        fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        t0 = time.perf_counter()
        for off in range(0, nbytes, PIECE):
            os.pwrite(fd, memoryview(buf)[:min(PIECE, nbytes - off)], off)
        os.fsync(fd)
        w.append(time.perf_counter() - t0)
        os.close(fd)
        r_warm.append(read_all())
        drop_pages(path)
        r_cold.append(read_all())
    os.unlink(path)
    return {"write_fsync": gbs(nbytes, w), "read_page_cache": gbs(nbytes, r_warm), "read_after_dontneed": gbs(nbytes, r_cold)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--docs", type=int, default=125000)
    ap.add_argument("--doc-len", type=int, default=1024)
    ap.add_argument("--file-gib", type=float, default=4.0)
    ap.add_argument("--dir", default=None, help="where the file goes (default: a fresh directory under the system's temporary one)")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import colpali_amd as amd

    dev = torch.device("cuda:0")
    corpus = make_shard(args.docs, args.doc_len, dev, seed=1)
    res = {"shard_gb": corpus.nbytes / 1e9, "device": torch.cuda.get_device_name(0)}
    res["digest_whole_shard"] = digest_leg(amd, corpus.blob)
    probe = stream_ceiling(amd, corpus)
    res["stream_probe_gbs"] = None if probe is None else probe["gbs"]
    res["digest_share_of_probe"] = None if probe is None else res["digest_whole_shard"]["median"] / probe["gbs"]
    res["digest_one_64MiB_chunk"] = digest_leg(amd, corpus.blob.view(torch.uint8).view(-1)[:PIECE], repeats=21)
    res["pinned"] = pinned_leg(dev)

    n_docs = max(1, min(args.docs, int(args.file_gib * (1 << 30)) // (args.doc_len * 256)))
    rows = n_docs * args.doc_len
    part = amd.PackedCorpus(blob=corpus.blob[:rows], offsets=corpus.offsets[:n_docs + 1].clone(), clamp0=None,
                            lengths=corpus.lengths[:n_docs].clone())
    work = args.dir or tempfile.mkdtemp(prefix="persist_bench_")
    path = os.path.join(work, "shard.msim")
    res["file_gb"] = part.nbytes / 1e9
    res["dir"] = "--dir" if args.dir else "system temporary directory"
    res["fs_type"] = fs_type(work)
    res["disk"] = disk_leg(os.path.join(work, "raw.bin"), part.nbytes, args.repeats)
    legs = {"save": [], "load_verify_page_cache": [], "load_noverify_page_cache": [], "load_verify_after_dontneed": [],
            "load_noverify_after_dontneed": [], "verify_file_host_one_thread": []}
    try:
        for rep in range(args.repeats):
            legs["save"].append(timed(lambda: part.save(path))[0])
            for cold in (False, True):
                for verify in (True, False):
                    if cold:
                        drop_pages(path)
                    dt, got = timed(lambda: amd.PackedCorpus.load(path, dev, verify=verify))
                    legs[f"load_{'verify' if verify else 'noverify'}_{'after_dontneed' if cold else 'page_cache'}"].append(dt)
                    if rep == 0 and verify and not cold:
                        res["round_trip_equal"] = bool(torch.equal(got.blob, part.blob))
                    del got
            if rep == 0:
                legs["verify_file_host_one_thread"].append(timed(lambda: amd.verify_file(path))[0])
    finally:
        if os.path.exists(path):
            os.unlink(path)
        if not args.dir:
            os.rmdir(work)
    res.update({name: gbs(part.nbytes, secs) for name, secs in legs.items() if secs})
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
