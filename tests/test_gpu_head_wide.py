"""The embedding head at width 320 (ColQwen3: embed_head_wide.hip behind msim_embed_head_wide*, colpali_amd/embed.py) on the GPU,
against the comparison rule of tests/head_wide_truth.py (candidates of the reference's own lines on the CPU, shares calibrated by the
exactly-accumulated chain on the same input; tests/test_head_wide_host.py shows that the rule is meaningful for every case here).

Row tile of the kernel: 128 rows; K chunk 64; weight ring 2 deep, hidden-state ring 3 deep -- the forward cases walk those edges."""
import numpy as np
import pytest
import torch

from tests import head_wide_truth as wt
from tests.head_truth import _grad_close, _truth_grads

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W = 320


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).view(torch.int16), b.reshape(-1).view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name,seed,B,S,H,dtype,pad", wt.FORWARD_CASES, ids=[c[0] for c in wt.FORWARD_CASES])
def test_forward_against_the_reference_rule(amd, name, seed, B, S, H, dtype, pad):
    hidden, weight, bias, mask, cands, ref = wt.reference(seed, B, S, H, dtype, pad)
    got = amd.embedding_head(hidden.to(DEV), weight.to(DEV), bias.to(DEV), mask.to(DEV))
    wt.check_wide(got, hidden, weight, bias, mask, cands=cands, ref=ref, label=name)


# ------------------------------------------------------------------------------------------------------------------ 2. image mask
def test_image_mask_and_missing_bias(amd):
    hidden, weight, _, mask, extra = wt.image_mask_case()
    got = amd.embedding_head(hidden.to(DEV), weight.to(DEV), None, mask.to(DEV), extra.to(DEV))
    wt.check_wide(got, hidden, weight, None, mask, extra, label="image mask, no bias")
    as_int = amd.embedding_head(hidden.to(DEV), weight.to(DEV), None, mask.to(DEV), extra.to(torch.int64).to(DEV))
    assert _same_bits(got, as_int)
    as_bool_attention = amd.embedding_head(hidden.to(DEV), weight.to(DEV), None, (mask != 0).to(DEV), extra.to(DEV))
    assert _same_bits(got, as_bool_attention)


# ------------------------------------------------------------------------------------------------------------------ 3. row map
def test_row_map_forms_through_the_raw_abi(amd):
    """Kept rows to scattered, descending destinations; dropped rows (-1); zero rows (-2 - v); ld_out = 328 with a canary."""
    L = amd._lib.lib()
    seed, B, S, H, dtype, pad = wt.FORWARD_CASES[4][1:]                      # (2, 60, 256) bf16
    hidden, weight, bias, mask = wt.case(seed, B, S, H, dtype, pad)
    M, ld, n_dst = B * S, 328, 2 * B * S + 7
    x, w, b = hidden.to(DEV).reshape(M, H), weight.to(DEV), bias.to(DEV)
    dense = amd.embedding_head(hidden.to(DEV), w, b, torch.ones(B, S, dtype=torch.long, device=DEV)).reshape(M, W)
    g = torch.Generator().manual_seed(5)
    kind = torch.randint(0, 4, (M,), generator=g)                            # 0, 1: kept; 2: dropped; 3: zero row
    kind[:3] = torch.tensor([0, 2, 3])
    dest = (n_dst - 1 - 2 * torch.arange(M)) - torch.randint(0, 2, (M,), generator=g)   # descending, with gaps, all distinct
    row_map = torch.full(((M + 255) // 256 * 256,), -1, dtype=torch.int32)
    row_map[:M] = torch.where(kind <= 1, dest, torch.where(kind == 2, torch.full_like(dest, -1), -2 - dest)).to(torch.int32)
    canary = 0x5A5A
    buf = torch.full((n_dst, ld), canary, dtype=torch.int16, device=DEV).view(dtype)
    rc = L.msim_embed_head_wide(amd._lib.dtype_code(dtype), x.data_ptr(), M, H, w.data_ptr(), b.data_ptr(), W,
                                row_map.to(DEV).data_ptr(), buf.data_ptr(), ld, _stream())
    assert rc == 0, L.msim_last_error()
    torch.cuda.synchronize()
    out = buf.cpu().view(torch.int16)
    want = torch.full((n_dst, ld), canary, dtype=torch.int16)
    kept, zero = kind <= 1, kind == 3
    want[dest[kept], :W] = dense.cpu().view(torch.int16)[kept]
    want[dest[zero], :W] = 0
    assert int(kept.sum()) > 20 and int(zero.sum()) > 10 and int((kind == 2).sum()) > 10
    assert torch.equal(out[dest[kept], :W], want[dest[kept], :W])           # the dense result's rows, bit for bit
    assert torch.count_nonzero(out[dest[zero], :W] & 0x7FFF) == 0            # zero rows (of either sign)
    out_abs = out.clone()
    out_abs[dest[zero], :W] &= 0x7FFF
    assert torch.equal(out_abs, want)                                        # everything else still holds the canary


# ------------------------------------------------------------------------------------------------------------------ 4. degenerate
def test_degenerate_calls(amd):
    w = torch.randn(W, 64).to(torch.bfloat16).to(DEV)
    empty = amd.embedding_head(torch.zeros(0, 5, 64, dtype=torch.bfloat16, device=DEV), w, None,
                               torch.ones(0, 5, dtype=torch.long, device=DEV))
    assert empty.shape == (0, 5, W)
    hidden, weight, bias, mask = wt.single_row_case()
    got = amd.embedding_head(hidden.to(DEV), weight.to(DEV), bias.to(DEV), torch.zeros_like(mask).to(DEV))
    assert got.shape == (2, 9, W) and torch.count_nonzero(got) == 0          # an all-masked batch
    got = amd.embedding_head(hidden.to(DEV), weight.to(DEV), bias.to(DEV), mask.to(DEV))
    wt.check_wide(got, hidden, weight, bias, mask, label="single kept row")
    assert abs(float(got[1, 4].float().norm()) - 1.0) < 2.0**-6


# ------------------------------------------------------------------------------------------------------------------ 5. CorpusWriter
def test_corpus_writer_equals_the_reference_road_to_the_scorer(amd):
    """tests/test_gpu_head.py's test of the same name at width 320, H = 2048: the writer drops the masked rows and flags the page;
    scores must be identical bit for bit to the reference user's road (unbind the dense output, score_multi_vector)."""
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(78)
    H = 2048
    weight = (torch.randn(W, H, generator=g) / H**0.5).to(torch.bfloat16).to(dev)
    bias = (torch.randn(W, generator=g) * 0.1).to(torch.bfloat16).to(dev)
    writer = amd.CorpusWriter(capacity_rows=5 * 300 + 4 * 210 + 3 * 64, device=dev, width=W)
    pages, dense_all, masks = [], [], []
    for B, S, pad in ((5, 300, "left"), (4, 210, "right"), (3, 64, "right")):
        hidden, _, _, mask = wt.case(B + S, B, S, H, torch.bfloat16, pad)
        if S == 64:
            mask[:] = 1                                    # a batch without any padding
        hidden, mask = hidden.to(dev), mask.to(dev)
        assert writer.append(hidden, weight, bias, mask) == B
        dense = amd.embedding_head(hidden, weight, bias, mask)
        pages.extend(list(torch.unbind(dense)))
        dense_all.append(dense)
        masks.append(mask)
    corpus = writer.finish()
    assert len(corpus) == 12 and corpus.blob.shape[1] == W
    want_rows = torch.cat([d[m != 0] for d, m in zip(dense_all, masks)])
    assert _same_bits(corpus.blob, want_rows)
    assert corpus.lengths.tolist() == [int((m[b] != 0).sum()) for m in masks for b in range(m.shape[0])]
    qs = [torch.nn.functional.normalize(torch.randn(n, W, generator=g), dim=-1).to(torch.bfloat16) for n in (20, 32, 11)]
    via_reference_road = amd.score_multi_vector(qs, [p.cpu() for p in pages], device=dev)
    direct = amd.maxsim_scores(amd.pack_queries(qs, dev), corpus).cpu()
    assert torch.equal(via_reference_road, direct)
    from oracle import maxsim_oracle as mo

    want = mo.score_multi_vector([q.float().numpy() for q in qs], [p.float().cpu().numpy() for p in pages], batch_size=128, mode="f32")
    assert np.max(np.abs(direct.numpy() - want) / np.maximum(np.abs(want), 1.0)) <= 1e-5
    # the rest of the 320-wide line takes the written corpus as it takes pack_passages of the same pages
    packed_dense = amd.pack_passages([p.cpu() for p in pages], dev)                        # zero rows kept, as the reference user has them
    all_ids = torch.arange(12, device=dev).expand(3, 12).contiguous()
    assert torch.equal(amd.rerank(qs, corpus, all_ids), amd.rerank(qs, packed_dense, all_ids))
    assert torch.equal(amd.rerank(qs, corpus, all_ids).cpu(), direct)
    packed_kept = amd.pack_passages([d[m != 0].cpu() for dd, mm in zip(dense_all, masks) for d, m in zip(dd, mm)], dev)
    fp4, fp4_want = amd.Fp4WideIndex.build(corpus), amd.Fp4WideIndex.build(packed_kept)
    assert torch.equal(fp4.codes, fp4_want.codes) and torch.equal(fp4.scales, fp4_want.scales)
    # a two-stage search over the written corpus with every page a candidate is the full scan
    retriever = amd.ShardedRetriever(corpus)
    s2, i2 = retriever.search(qs, k=5, prefilter=fp4, n_candidates=12)
    s1, i1 = retriever.search(qs, k=5)
    assert torch.equal(s1, s2) and torch.equal(i1, i2)


def test_corpus_writer_rejections_leave_the_writer_usable(amd):
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(2)
    H = 256
    w = (torch.randn(W, H, generator=g) / H**0.5).to(torch.bfloat16).to(dev)
    writer = amd.CorpusWriter(capacity_rows=100, device=dev, width=W)
    h = torch.randn(2, 40, H, generator=g).to(torch.bfloat16).to(dev)
    mask = torch.ones(2, 40, dtype=torch.long, device=dev)
    mask[:, 10:] = 0                                       # 20 real rows out of 80 positions
    assert writer.append(h, w, None, mask) == 2
    big = torch.randn(3, 40, H, generator=g).to(torch.bfloat16).to(dev)
    with pytest.raises(RuntimeError, match="capacity"):
        writer.append(big, w, None, torch.ones(3, 40, dtype=torch.long, device=dev))      # 20 + 120 > 100
    assert writer.rows_written() == 20
    before = writer.blob.clone()
    with pytest.raises(ValueError, match="320.*128|128.*320"):                              # a weight of the other width
        writer.append(h, w[:128].contiguous(), None, mask)
    assert writer.rows_written() == 20 and torch.equal(writer.blob.view(torch.int16)[:20], before.view(torch.int16)[:20])
    narrow = amd.CorpusWriter(capacity_rows=100, device=dev)
    with pytest.raises(ValueError, match="320.*128|128.*320"):
        narrow.append(h, w, None, mask)
    assert narrow.rows_written() == 0
    assert writer.append(h, w, None, torch.ones(2, 40, dtype=torch.long, device=dev)) == 2   # 20 + 80 fits
    corpus = writer.finish()
    assert len(corpus) == 4 and corpus.blob.shape == (100, W)


# ------------------------------------------------------------------------------------------------------------------ 6. backward
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("with_bias", [True, False])
def test_backward_against_float64_autograd(amd, dtype, with_bias):
    B, S, H = 3, 45, 512
    hidden, weight, bias, mask = wt.case(41 + int(with_bias), B, S, H, dtype, bias=with_bias)
    G = torch.randn(B, S, W, generator=torch.Generator().manual_seed(S)).to(dtype)
    hx, wx = hidden.to(DEV).requires_grad_(True), weight.to(DEV).requires_grad_(True)
    bx = None if bias is None else bias.to(DEV).requires_grad_(True)
    out = amd.embedding_head(hx, wx, bx, mask.to(DEV))
    assert out.requires_grad and out.grad_fn is not None and out.shape == (B, S, W)
    (out.float() * G.to(DEV).float()).sum().backward()
    (want_h, want_w, want_b), (bd_h, bd_w, bd_b) = _truth_grads(hidden, weight, bias, mask, G)
    assert hx.grad.dtype == dtype and wx.grad.shape == (W, H)
    assert _grad_close(hx.grad, want_h, bd_h, dtype) and _grad_close(wx.grad, want_w, bd_w, dtype)
    if bx is not None:
        assert _grad_close(bx.grad, want_b, bd_b, dtype)
    assert torch.count_nonzero(hx.grad.cpu()[mask == 0]) == 0
    # masked rows' dproj is exactly zero: the raw entry
    L = amd._lib.lib()
    M = B * S
    proj = torch.nn.functional.linear(hidden.to(DEV).reshape(M, H), weight.to(DEV), None if bias is None else bias.to(DEV))
    row_map = torch.where(mask.reshape(-1) != 0, torch.arange(M), -2 - torch.arange(M)).to(torch.int32).to(DEV)
    dproj = torch.full((M, W), float("nan"), dtype=dtype, device=DEV)
    rc = L.msim_embed_head_wide_bwd(amd._lib.dtype_code(dtype), proj.data_ptr(), G.to(DEV).reshape(M, W).contiguous().data_ptr(),
                                    row_map.data_ptr(), M, W, dproj.data_ptr(), _stream())
    assert rc == 0, L.msim_last_error()
    dproj = dproj.cpu()
    keep = mask.reshape(-1) != 0
    assert torch.count_nonzero(dproj[~keep].view(torch.int16)) == 0
    assert bool(torch.isfinite(dproj[keep].float()).all()) and float(dproj[keep].float().abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------------ 7. patched model
def test_patched_colqwen3_forward(amd):
    """A ColQwen3 test class on transformers' Qwen3-VL backbone (tests/model_classes_wide.py), projection to 320 columns, text batch
    padded on the left: with the models patch the fused head runs exactly once (colpali_amd/models.py admits width 320: the fused
    head measured faster than the lines it replaces, profiles/head_wide_summary.md) and the output is within one ulp of the
    unpatched forward on the same GPU, more than 90 % bit-equal (tests/test_gpu_models.py's tolerances for the same comparison)."""
    from colpali_amd import models as M
    from tests.model_classes_wide import tiny_colqwen3
    from tests.model_fixtures import text_batch
    from tests.test_gpu_models import one_ulp_close

    for dtype in (torch.bfloat16, torch.float16):
        model, cls = tiny_colqwen3()
        model = model.to(DEV, dtype)
        assert model.custom_text_proj.out_features == W
        batch = text_batch(left_pad=True, device=DEV)
        with torch.no_grad():
            want = model(**batch)
        assert want.shape == (5, 37, W)
        amd.patch_colpali_engine(scorer=False, losses=False, models=True)
        try:
            assert cls in M.installed()
            calls = []
            real = M.embedding_head
            M.embedding_head = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
            try:
                with torch.no_grad():
                    got = model(**batch)
            finally:
                M.embedding_head = real
        finally:
            amd.unpatch_colpali_engine()
        pad = batch["attention_mask"] == 0
        assert got.dtype == want.dtype and got.shape == want.shape
        assert bool((got[pad] == 0).all()) and bool((want[pad] == 0).all())
        assert calls == [1], "the fused head did not run exactly once"
        ok, same = one_ulp_close(got, want, dtype)
        assert ok and same > 0.9, same
        with torch.no_grad():
            assert torch.equal(model(**batch), want)                         # unpatched again: the original, bit for bit


# ------------------------------------------------------------------------------------------------------------------ 8. capture
def test_head_under_graph_capture(amd):
    seed, B, S, H, dtype, pad = wt.FORWARD_CASES[3][1:]
    hidden, weight, bias, mask = (t.to(DEV) for t in wt.case(seed, B, S, H, dtype, pad))
    eager = amd.embedding_head(hidden, weight, bias, mask)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        amd.embedding_head(hidden, weight, bias, mask)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = amd.embedding_head(hidden, weight, bias, mask)
    for _ in range(2):
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(captured, eager)
