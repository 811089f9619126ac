"""Token-to-patch alignment without a GPU: the C ABI's declaration, export and argument checks (refused before any device work),
`align`'s error classes, `Alignment.similarity_maps` (axis order, row selection, its ValueError) and the sharded host logic of
ShardedRetriever.align over gloo worlds of 2 and 3 with a numpy truth injected as align_fn: every rank must get the unsharded
answer."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


def _call(L, dtype=0, qt=FAKE, q_off=FAKE, n_q=2, q_rows=7, T=4, d=FAKE, d_off=FAKE, n_d=10, d_rows=100, dim=128, cand=FAKE, m=4,
          ld_cand=4, bs=FAKE, br=FAKE, sims=None, max_rows=16):
    return L.msim_align_candidates(dtype, qt, q_off, n_q, q_rows, T, d, d_off, None, n_d, d_rows, dim, cand, m, ld_cand, 0, bs, br, sims,
                                   max_rows, None)


def test_the_header_declares_the_entry_and_the_library_exports_it():
    import colpali_amd

    header = open(os.path.join(ROOT, "include", "maxsim.h")).read()
    assert re.search(r"\bint\s+msim_align_candidates\s*\(", header)
    assert re.search(r"#define\s+MSIM_ABI_VERSION\s+22\b", header)
    L = colpali_amd._lib.lib()
    assert L.msim_abi_version() == 22
    assert hasattr(L, "msim_align_candidates")
    assert colpali_amd.align is colpali_amd.retrieval.align and colpali_amd.Alignment is colpali_amd.retrieval.Alignment


def test_align_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert _call(L, n_q=0, qt=None, q_off=None, d=None, d_off=None, cand=None, bs=None, br=None) == 0    # nothing to do: no pointer
    assert _call(L, m=0, qt=None, q_off=None, d=None, d_off=None, cand=None, bs=None, br=None) == 0      # is looked at
    for kw in (dict(n_q=-1), dict(m=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(T=-1), dict(max_rows=-1), dict(qt=None),
               dict(q_off=None), dict(d=None), dict(d_off=None), dict(cand=None), dict(bs=None), dict(br=None), dict(qt=FAKE + 8),
               dict(d=FAKE + 2), dict(bs=FAKE + 2), dict(br=FAKE + 1), dict(sims=FAKE + 2), dict(cand=FAKE + 4), dict(ld_cand=3)):
        assert _call(L, **kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dtype=2), dict(dtype=7), dict(dim=64), dict(dim=96), dict(dim=256), dict(T=129)):
        assert _call(L, **kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()


def _unit(g, n, dim=128, dtype=torch.bfloat16):
    return torch.nn.functional.normalize(torch.randn(n, dim, generator=g), dim=-1).to(dtype)


def test_align_error_classes_match_rerank():
    import colpali_amd as amd

    g = torch.Generator().manual_seed(0)
    cpu = torch.device("cpu")
    corpus = amd.pack_passages([_unit(g, 5) for _ in range(6)], cpu, batch_size=None)
    ids = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError):                                  # a CPU corpus: the GPU-only error, as rerank
        amd.align([_unit(g, 4)] * 2, corpus, ids)
    with pytest.raises(RuntimeError):
        amd.rerank([_unit(g, 4)] * 2, corpus, ids)
    with pytest.raises(ValueError):                                    # maps of a sharded corpus stay with the holder
        amd.ShardedRetriever(corpus, world=2, rank=0, dist=object(), align_fn=lambda *a, **k: None).align(None, ids, maps=True)


def _alignment(sims, q_lens, p_lens, ids, id_base=0):
    import colpali_amd as amd

    n_q, m, T, _ = sims.shape
    return amd.Alignment(best_sim=sims.amax(dim=3), best_row=sims.argmax(dim=3).to(torch.int32), ids=ids, sims=sims,
                         query_lengths=torch.tensor(q_lens), page_lengths=torch.tensor(p_lens), id_base=id_base)


def test_similarity_maps_axis_order_and_value_error():
    nx, ny = 3, 5                                                      # n_patches = (x, y): the rows of a page are "(h w)", h = y
    T, R = 4, 20
    sims = torch.full((2, 2, T, R), -float("inf"))
    # entry (1, 0): page 7 -- 2 leading non-image rows, then the 15 patches, then one trailing row; query 1 has 3 tokens
    block = torch.arange(3 * 18, dtype=torch.float32).view(3, 18)
    sims[1, 0, :3, :18] = block
    ids = torch.tensor([[-1, -1], [7 + 100, -1]])
    al = _alignment(sims, [4, 3], [1] * 7 + [18], ids, id_base=100)
    got = al.similarity_maps(1, 0, (nx, ny), rows=slice(2, 17))
    assert got.shape == (3, nx, ny) and got.dtype == torch.float32
    for t in range(3):
        for x in range(nx):
            for y in range(ny):
                assert got[t, x, y] == block[t, 2 + y * nx + x]        # "(h w) -> w h": patch (h = y, w = x) is row y * nx + x
    mask = torch.zeros(18, dtype=torch.bool)
    mask[2:17] = True
    assert torch.equal(al.similarity_maps(1, 0, (nx, ny), rows=mask), got)
    # the reference's own rearrangement of the same rows (similarity_map_utils.py: "(h w) c" patches, "n (h w) -> n w h")
    want = block[:, 2:17].view(3, ny, nx).permute(0, 2, 1)
    assert torch.equal(got, want)
    with pytest.raises(ValueError, match="does not match the number of non-padded image tokens"):
        al.similarity_maps(1, 0, (nx, ny))                             # all 18 rows are not 15 patches
    with pytest.raises(ValueError, match="does not match"):
        al.similarity_maps(1, 0, (4, 4), rows=slice(2, 17))
    with pytest.raises(ValueError):                                    # no page behind the entry
        al.similarity_maps(0, 1, (nx, ny))
    with pytest.raises(ValueError):                                    # a mask of the wrong length
        al.similarity_maps(1, 0, (nx, ny), rows=torch.ones(17, dtype=torch.bool))
    al.sims = None
    with pytest.raises(ValueError):                                    # made without maps
        al.similarity_maps(1, 0, (nx, ny), rows=slice(2, 17))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _numpy_align(queries, corpus, ids, maps=False):
    """The contract of msim_align_candidates on host tensors, float64 products: a dense [n_q, Lq, dim] query box, every row a token."""
    import colpali_amd as amd

    Q = queries.double().numpy()
    D = corpus.blob.double().numpy()
    off = corpus.offsets.numpy()
    n_q, T, _ = Q.shape
    m = ids.shape[1]
    best = np.full((n_q, m, T), -np.inf, dtype=np.float32)
    row = np.full((n_q, m, T), -1, dtype=np.int32)
    out_ids = np.full((n_q, m), -1, dtype=np.int64)
    for q in range(n_q):
        for j in range(m):
            c = int(ids[q, j]) - corpus.id_base
            if int(ids[q, j]) < 0 or not (0 <= c < len(corpus)):
                continue
            out_ids[q, j] = int(ids[q, j])
            if off[c + 1] > off[c]:
                S = Q[q] @ D[off[c]:off[c + 1]].T
                best[q, j] = S.max(axis=1).astype(np.float32)
                row[q, j] = S.argmax(axis=1)                           # numpy's argmax: the first maximum
    return amd.Alignment(torch.from_numpy(best), torch.from_numpy(row), torch.from_numpy(out_ids), None, torch.full((n_q,), T),
                         corpus.lengths, corpus.id_base)


def _worker(rank, world, port, n_docs, m, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd

    g = torch.Generator().manual_seed(11)
    lens = torch.randint(0, 40, (n_docs,), generator=g).tolist()       # pages of 0 rows included: (-inf, -1) from their holder
    lens[3] = 0
    docs = [_unit(g, n) for n in lens]
    docs[4] = docs[2].clone()                                          # the same page on two shards
    q = torch.stack([_unit(g, 8) for _ in range(4)])
    ids = torch.randint(-3, n_docs + 3, (4, m), generator=g)           # -1 .. -3 and ids past the corpus: no page
    ids[1, :] = -1
    ids[2, 0] = ids[2, 1]                                              # a duplicate
    ids[0, 0] = 3
    cpu = torch.device("cpu")
    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    part = docs[lo:hi] if hi > lo else [docs[0][:0]]
    shard = colpali_amd.pack_passages(part, cpu, batch_size=None, id_base=lo)
    if hi == lo:
        shard.id_base = n_docs + 100                                   # a rank without pages holds no listed id
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, align_fn=_numpy_align)
    al = r.align(q, ids)
    assert al.sims is None
    with pytest.raises(ValueError):
        r.align(q, ids, maps=True)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), s=al.best_sim.numpy(), r=al.best_row.numpy(), i=al.ids.numpy())
    if rank == 0:                                                      # unsharded truth
        full = colpali_amd.pack_passages(docs, cpu, batch_size=None)
        t = colpali_amd.ShardedRetriever(full, align_fn=_numpy_align).align(q, ids)
        np.savez(os.path.join(out_dir, "truth.npz"), s=t.best_sim.numpy(), r=t.best_row.numpy(), i=t.ids.numpy())
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,m", [(2, 37, 9), (3, 50, 12), (3, 8, 4)])
def test_sharded_align_equals_unsharded(tmp_path, world, n_docs, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    assert (truth["i"][1] == -1).all() and np.isneginf(truth["s"][1]).all() and (truth["r"][1] == -1).all()
    assert truth["i"][0, 0] == 3 and np.isneginf(truth["s"][0, 0]).all()       # a page of 0 rows
    assert (truth["r"] >= 0).any()
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("i", "r"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
        np.testing.assert_array_equal(got["s"].view(np.int32), truth["s"].view(np.int32), err_msg=f"rank {r}: best_sim bits")
