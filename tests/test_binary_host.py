"""The 1-bit sign index without a GPU: the truth helper (tests/binary_truth.py) on its own edge cases, the ABI's argument checks
(no device work), the Python class's refusals, and ShardedRetriever.search(prefilter=<BinaryIndex>) plumbing over gloo worlds of
2 and 3 with the truth injected as binary_score_fn.  Every rank must get the unsharded answer."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import binary_truth as bt
from tests import int8_truth as it

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

EINVAL, EUNSUPPORTED = -1, -2
FAKE = 1 << 20            # a 16-byte aligned non-null address: every call below is refused before it could touch it


# ------------------------------------------------------------------------------------------------------------ the truth helper
def test_truth_pack_unpack_round_trip_and_bit_order():
    rng = np.random.default_rng(0)
    signs = rng.choice(np.array([-1, 1], dtype=np.int8), size=(37, 128))
    codes = bt.pack(signs)
    assert codes.dtype == np.uint8 and codes.shape == (37, 16)
    np.testing.assert_array_equal(bt.unpack(codes), signs)
    one = -np.ones((1, 128), dtype=np.int8)
    one[0, 19] = 1                                   # dimension 19: bit 3 of byte 2
    want = np.zeros((1, 16), dtype=np.uint8)
    want[0, 2] = 1 << 3
    np.testing.assert_array_equal(bt.pack(one), want)
    np.testing.assert_array_equal(bt.unpack(np.zeros((1, 16), np.uint8)), -np.ones((1, 128), np.int8))   # zero bits: the all-(-1) row


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_truth_sign_is_the_stored_sign_bit(dtype):
    x = torch.zeros(1, 128, dtype=dtype)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3] = 0.0, -0.0, 1.5, -1.5
    raw = bt.raw_bits(x).copy()
    raw[0, 4] = 0xffc0 if dtype == torch.bfloat16 else 0xfe00      # a negative NaN
    raw[0, 5] = 0x7fc0 if dtype == torch.bfloat16 else 0x7e00      # a positive NaN
    raw[0, 6], raw[0, 7] = 0x8001, 0x0001                          # the smallest subnormals, negative and positive
    s = bt.sign_bits(raw)[0]
    assert s[:8].tolist() == [1, -1, 1, -1, -1, 1, -1, 1]
    assert (s[8:] == 1).all()                                      # +0.0 codes as +1
    assert bt.encode(raw)[0, 0] == 0b10100101


def test_truth_planted_copy_ranks_first():
    """A page that holds exact copies of a query's tokens ranks first: a copy attains sum |q8|, the maximum of sum q8 s."""
    rng = np.random.default_rng(1)

    def unit(n):
        x = rng.standard_normal((n, 128)).astype(np.float32)
        return torch.from_numpy(x / np.linalg.norm(x, axis=1, keepdims=True)).to(torch.bfloat16)

    qs = [unit(n) for n in (5, 12, 32)]
    pages = [unit(n) for n in rng.integers(1, 40, size=50)]
    planted = {0: 7, 1: 23, 2: 41}
    for q, p in planted.items():
        pages[p] = torch.cat([pages[p][:3], qs[q], pages[p][3:]])
    d_off = np.cumsum([0] + [len(p) for p in pages])
    raw = bt.raw_bits(torch.cat(pages))
    q8, sq = it.quantize_tokens(torch.cat(qs).float().numpy())
    q_off = np.cumsum([0] + [len(q) for q in qs])
    S = bt.scores(q8, sq, q_off, bt.encode(raw), d_off)
    for q, p in planted.items():
        assert int(np.argmax(S[q])) == p
        top = np.float32(0)
        for i in range(q_off[q], q_off[q + 1]):                    # the attained maximum, in the documented order
            top = np.float32(top + np.float32(np.float32(np.abs(q8[i].astype(np.int64)).sum()) * sq[i]))
        assert S[q, p] == top


# ------------------------------------------------------------------------------------------------------------------- the ABI
def test_abi_refuses_bad_arguments_before_device_work():
    import colpali_amd

    L = colpali_amd._lib.lib()
    assert colpali_amd._lib.ABI_VERSION == 22 == L.msim_abi_version()

    def rows(dtype=0, x=FAKE, n=40, dim=128, codes=FAKE):
        return L.msim_bin_encode_rows(dtype, x, n, dim, codes, None)

    def score(q8=FAKE, sq=FAKE, qo=FAKE, n_q=4, q_rows=40, maxq=32, codes=FAKE, do=FAKE, c0=None, n_d=10, d_rows=90, dim=128,
              out=FAKE, ld=10):
        return L.msim_bin_scores(q8, sq, qo, n_q, q_rows, maxq, codes, do, c0, n_d, d_rows, dim, out, ld, None)

    assert rows(n=0) == 0 and rows(n=0, x=None, codes=None) == 0
    assert score(n_q=0) == 0 and score(n_d=0, q8=None, codes=None, out=None) == 0
    for kw in (dict(n=-1), dict(x=None), dict(codes=None), dict(x=FAKE + 8), dict(codes=FAKE + 4)):
        assert rows(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=320), dict(dtype=2), dict(dtype=7)):
        assert rows(**kw) == EUNSUPPORTED, kw
        assert L.msim_last_error()
    for kw in (dict(n_q=-1), dict(n_d=-1), dict(q_rows=-1), dict(d_rows=-1), dict(maxq=-1), dict(q8=None), dict(sq=None),
               dict(qo=None), dict(codes=None), dict(do=None), dict(out=None), dict(q8=FAKE + 4), dict(codes=FAKE + 8),
               dict(sq=FAKE + 2), dict(out=FAKE + 2), dict(qo=FAKE + 1), dict(do=FAKE + 2), dict(ld=9)):
        assert score(**kw) == EINVAL, kw
        assert L.msim_last_error()
    for kw in (dict(dim=64), dict(dim=320)):
        assert score(**kw) == EUNSUPPORTED, kw
    assert L.msim_bin_scores_plan(4, 32, 10, 90, None) == EINVAL and L.msim_bin_scores_plan(-1, 32, 10, 90, FAKE) == EINVAL


# ------------------------------------------------------------------------------------------------------------ the Python class
def _index(shard):
    from colpali_amd import BinaryIndex

    return BinaryIndex(torch.from_numpy(bt.encode(bt.raw_bits(shard.blob))), shard.offsets.clone(), shard.clamp0, shard.lengths.clone(),
                       shard.id_base)


def _truth_fn(queries, index):
    qb = [x.float().numpy() for x in queries]
    q8, sq = it.quantize_tokens(np.concatenate(qb))
    q_off = np.cumsum([0] + [len(x) for x in qb])
    c0 = None if index.clamp0 is None else index.clamp0.numpy()
    return torch.from_numpy(bt.scores(q8, sq, q_off, index.codes.numpy(), index.offsets.numpy(), c0))


def _shard(n=5, rows=3, width=128, dtype=torch.bfloat16, id_base=7):
    import colpali_amd

    return colpali_amd.pack_passages([torch.randn(rows, width).to(dtype) for _ in range(n)], torch.device("cpu"), batch_size=None,
                                     id_base=id_base)


def test_class_refusals_without_a_gpu():
    import colpali_amd
    from colpali_amd import BinaryIndex

    shard = _shard()
    idx = _index(shard)
    assert len(idx) == 5 and idx.device == torch.device("cpu") and idx.nbytes == 15 * 16 + 6 * 4
    assert "BinaryIndex" in colpali_amd.__all__ and "binary_scores" in colpali_amd.__all__
    for codes in (torch.zeros(15, 16, dtype=torch.int8), torch.zeros(15, 128, dtype=torch.uint8), torch.zeros(15 * 16, dtype=torch.uint8),
                  torch.zeros(16, 15, dtype=torch.uint8).t()):
        with pytest.raises(ValueError, match="codes must be"):
            BinaryIndex(codes, shard.offsets, None, shard.lengths)
    with pytest.raises(ValueError, match="offsets must be"):
        BinaryIndex(idx.codes, shard.offsets[:-1], None, shard.lengths)
    with pytest.raises(ValueError, match="clamp0 must be"):
        BinaryIndex(idx.codes, shard.offsets, torch.zeros(4, dtype=torch.uint8), shard.lengths)
    with pytest.raises(NotImplementedError, match="the binary index takes bfloat16 / float16 pages of width 128"):
        BinaryIndex.build(_shard(width=320))
    with pytest.raises(NotImplementedError, match="the binary index takes bfloat16 / float16 pages of width 128"):
        BinaryIndex.build(_shard(dtype=torch.float32))


def test_prefilter_index_checks_without_a_gpu():
    import colpali_amd

    shard = _shard()
    calls = []
    r = colpali_amd.ShardedRetriever(shard, score_fn=lambda q, c: calls.append("score"), binary_score_fn=lambda q, i: calls.append("bin"),
                                     rerank_fn=lambda q, c, x: calls.append("rr"))
    q = torch.randn(2, 4, 128).to(torch.bfloat16)
    for idx in (_index(_shard(n=4)), _index(_shard(id_base=6))):
        with pytest.raises(ValueError, match="same documents"):
            r.search(q, prefilter=idx, n_candidates=3)
    with pytest.raises(ValueError, match="n_candidates"):
        r.search(q, prefilter=_index(shard))
    with pytest.raises(ValueError, match="prefilter must be a PackedCorpus, an FdeIndex, an Int8Index, a CentroidIndex or a BinaryIndex"):
        r.search(q, prefilter=torch.zeros(5, 16, dtype=torch.uint8), n_candidates=3)
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------ sharding
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_docs, k, m, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import colpali_amd
    from oracle import maxsim_oracle as mo
    from oracle import topk_oracle

    g = torch.Generator().manual_seed(11)
    lens = torch.randint(0, 40, (n_docs,), generator=g).tolist()
    docs = [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(torch.bfloat16) for n in lens]
    docs[4] = docs[2].clone()                 # exact ties across shards
    q = torch.nn.functional.normalize(torch.randn(4, 8, 128, generator=g), dim=-1).to(torch.bfloat16)

    def score_fn(queries, corpus):
        return torch.from_numpy(mo.maxsim_f32(queries.float().numpy(), corpus.blob.float().numpy(), corpus.offsets.numpy(), None))

    def rerank_fn(queries, corpus, candidates):
        full = score_fn(queries, corpus)
        n = full.shape[1]
        d = candidates - corpus.id_base
        ok = (candidates >= 0) & (d >= 0) & (d < n)
        got = torch.gather(full, 1, d.clamp(0, max(n - 1, 0))) if n else torch.zeros(candidates.shape)
        return torch.where(ok, got, torch.full_like(got, -float("inf"))), torch.where(ok, candidates, torch.full_like(candidates, -1))

    lo, hi = colpali_amd.shard_range(n_docs, world, rank)
    shard = colpali_amd.pack_passages(docs[lo:hi], torch.device("cpu"), batch_size=None, id_base=lo)
    r = colpali_amd.ShardedRetriever(shard, world=world, rank=rank, dist=dist, score_fn=score_fn, select=topk_oracle.torch_select,
                                     rerank_fn=rerank_fn, binary_score_fn=_truth_fn)
    ps, pi = r.search(q, k=k, prefilter=_index(shard), n_candidates=m)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), ps=ps.numpy(), pi=pi.numpy())

    if rank == 0:                             # unsharded truth
        full = colpali_amd.pack_passages(docs, torch.device("cpu"), batch_size=None)
        _, coarse_ids = topk_oracle.topk(_truth_fn(q, _index(full)).numpy(), m)
        s, i = rerank_fn(q, full, torch.from_numpy(coarse_ids))
        tps, tpi = topk_oracle.topk(s.numpy(), k, 0, i.numpy())
        np.savez(os.path.join(out_dir, "truth.npz"), ps=tps, pi=tpi)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n_docs,k,m", [(2, 37, 5, 9), (3, 50, 7, 12), (3, 8, 10, 4)])
def test_sharded_binary_prefilter_equals_unsharded(tmp_path, world, n_docs, k, m):
    mp.spawn(_worker, args=(world, _free_port(), n_docs, k, m, str(tmp_path)), nprocs=world, join=True)
    truth = np.load(tmp_path / "truth.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        for key in ("pi", "ps"):
            np.testing.assert_array_equal(got[key], truth[key], err_msg=f"rank {r}: {key}")
