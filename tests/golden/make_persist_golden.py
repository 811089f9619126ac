"""Writes tests/golden/persist_v1_packed.msim and persist_v1_packed.npz: the file that pins format 1 (tests/test_persist_host.py).

Run once, when format 1 was defined; a later run must reproduce the committed bytes, or the format has changed:
    python tests/golden/make_persist_golden.py
Needs the built library (the digests come from msim_digest_host), no GPU."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

import colpali_amd  # noqa: E402


def main():
    g = torch.Generator().manual_seed(1)
    ps = [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16) for n in (5, 1, 19, 3)]
    pc = colpali_amd.pack_passages(ps, "cpu", batch_size=2, id_base=1000)       # rows end mid-chunk; clamp0 is [0, 1, 0, 1]
    path = os.path.join(HERE, "persist_v1_packed.msim")
    pc.save(path, chunk_bytes=4096)
    header = colpali_amd.verify_file(path)
    np.savez(os.path.join(HERE, "persist_v1_packed.npz"), blob_bits=pc.blob.view(torch.int16).numpy().view(np.uint16),
             offsets=pc.offsets.numpy(), clamp0=pc.clamp0.numpy(), lengths=pc.lengths.numpy(), id_base=np.int64(pc.id_base),
             digests=json.dumps({e["name"]: e["digest"] for e in header["tensors"]}))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
