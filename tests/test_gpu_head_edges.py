"""The embedding head (K3: embed_head.hip behind msim_embed_head*, colpali_amd/embed.py) at the launch forms and edges that
tests/test_gpu_head.py does not reach: the 2-byte-store instantiation and output strides other than 128, 1-3 K chunks per tile with
several tiles per workgroup, the widest hidden sizes the ABI takes, every mask dtype, writer row maps with interior holes / many pages /
empty pages, non-finite rows, subnormal fp16 operands, a second grid-stride pass of the backward, and argument validation.

The reference is always oracle/head_oracle.py (`head_literal` on the CPU in the tensor dtype, `head_truth` in float64); layouts are plain
torch indexing of the dense kernel output.

Tolerances.  bf16: tests/head_truth.py's `check`, unchanged (the reference's own bf16 output stays >= 99.98 % bit-equal to the exactly
accumulated chain -- a float64 Linear with the same three roundings -- for every hidden size from 64 to 16384).  fp16: the truth tier
(2^-9 relative on |value| >= 1e-3) and the 2-ulp maximum stay; the share of elements more than one ulp off is NOT something the reference
alone keeps under 1e-4 in fp16 (its CPU literal is more than one ulp from the exact chain on 0.5e-4 .. 4e-4 of the elements, growing with
the hidden size), so `check_f16` measures the literal against the exact chain on the same inputs and allows the kernel, against the same
chain, max(1e-4, 2 x the literal's share) and a bit-equal share of at least 1 - 2 x (1 - the literal's); the factor 2 covers the scatter
between two independent fp32 accumulation orders at these element counts.
"""
import pytest
import torch

from oracle import head_oracle as ho
from tests.head_truth import _case, _grad_close, _truth_grads, check, grid_distance

pytestmark = pytest.mark.gpu

BF16, F16 = torch.bfloat16, torch.float16
SENTINEL = 0x7B9D          # a finite 16-bit pattern (fp16 62368, bf16 4.1e36) that no unit-norm output can take


@pytest.fixture(scope="module")
def amd():
    import colpali_amd

    colpali_amd._lib.lib()
    return colpali_amd


@pytest.fixture(scope="module")
def CUS():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _keep(mask, extra=None):
    return (mask != 0) if extra is None else ((mask != 0) & (extra.reshape(mask.shape) != 0))


def exact_chain(hidden, weight, bias, mask, extra=None):
    """The reference's rounding chain with an exactly accumulated Linear: float64 products and sums, the Linear output, the norm and
    the quotient each rounded once to the tensor dtype, then the mask multiply."""
    dt = hidden.dtype
    y = torch.nn.functional.linear(hidden.double(), weight.double(), None if bias is None else bias.double()).to(dt)
    n = y.double().square().sum(-1, keepdim=True).sqrt().to(dt)
    o = (y.double() / n.double()).to(dt)
    return o * _keep(mask, extra).unsqueeze(-1).to(dt)


def check_f16(got, hidden, weight, bias, mask, extra=None):
    """fp16 comparison of the new cases (module docstring): kernel against the exact chain, bounded by what the CPU literal itself
    shows against that chain on the same inputs; then the float64 truth tier and the exact zeros of `check`."""
    assert got.dtype == F16
    chain = exact_chain(hidden, weight, bias, mask, extra)
    d_lit, same_lit = grid_distance(ho.head_literal(hidden, weight, bias, mask, extra), chain)
    d, same = grid_distance(got, chain)
    far_lit, far = float((d_lit > 1).float().mean()), float((d > 1).float().mean())
    msg = (f"kernel vs exact chain: bit-equal {same:.6f}, > 1 ulp {far:.3e}, max {float(d.max()):.2f} ulp; "
           f"CPU literal vs exact chain: bit-equal {same_lit:.6f}, > 1 ulp {far_lit:.3e}, max {float(d_lit.max()):.2f} ulp")
    print(msg)
    assert same >= 1.0 - 2.0 * (1.0 - same_lit), msg
    assert far <= max(1e-4, 2.0 * far_lit), msg
    assert float(d.max()) <= 2.0, msg
    truth = ho.head_truth(hidden, weight, bias, mask, extra)
    big = truth.abs() >= 1e-3
    assert torch.all(((got.cpu().double() - truth).abs() <= 2.0**-9 * truth.abs())[big])
    assert torch.count_nonzero(got.cpu()[~_keep(mask, extra)]) == 0


def check_any(got, hidden, weight, bias, mask, extra=None):
    (check if got.dtype == BF16 else check_f16)(got, hidden, weight, bias, mask, extra)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _stream(amd):
    return amd._lib.current_stream_handle(torch.device("cuda:0"))


# ---------------------------------------------------------------------------------------------------------------------------
# A. output layouts through the C ABI

_LAYOUTS = {                     # name: (ld_out, offset of `out` inside the sentinel buffer in elements)
    "ld136_aligned": (136, 8),
    "ld132": (132, 0),
    "ld128_out_8_byte_aligned": (128, 4),
    "ld129": (129, 3),
}


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_output_layouts_through_the_c_abi(amd, dtype):
    """msim_embed_head ships two instantiations of the kernel, picked by `ld_out % 8 == 0 && out 16-byte aligned`:
      ld_out 136, out 16 bytes into the buffer   -> the whole-row form (rows staged through LDS, 16-byte stores) at a stride != 128
      ld_out 132                                 -> the 2-byte-store form (rows are 8-byte aligned only)
      ld_out 128, out 4 elements into the buffer -> the 2-byte-store form (rows 8-byte aligned only)
      ld_out 129, out 3 elements into the buffer -> the 2-byte-store form (odd rows 2-byte aligned only)
    Same arithmetic and accumulation order in both, only the store path differs: every layout holds the bits of the contiguous
    ld_out = 128 call (the whole-row form, what embed.py launches), and nothing else in the buffer is touched."""
    L, dev = amd._lib.lib(), torch.device("cuda:0")
    M, H = 3 * 256 + 77, 192
    hidden, weight, bias, mask = _case(41, 1, M, H, dtype)
    mask[0, 5::11] = 0                                    # zero rows among the kept ones; the map's tail (rows M .. 1023) is -1
    mask[0, 300:340] = 0
    x, w, b = hidden.to(dev), weight.to(dev), bias.to(dev)
    m_dev = mask.reshape(-1).to(dev)
    row_map = torch.full((4 * 256,), 12345, dtype=torch.int32, device=dev)
    assert L.msim_embed_head_row_map(m_dev.data_ptr(), 3, None, 0, M, row_map.data_ptr(), _stream(amd)) == 0, L.msim_last_error()
    want_map = torch.where(mask.reshape(-1) != 0, torch.arange(M), -2 - torch.arange(M)).to(torch.int32)
    assert torch.equal(row_map.cpu(), torch.cat([want_map, torch.full((1024 - M,), -1, dtype=torch.int32)]))

    def launch(out_ptr, ld):
        rc = L.msim_embed_head(amd._lib.dtype_code(dtype), x.data_ptr(), M, H, w.data_ptr(), b.data_ptr(), 128, row_map.data_ptr(),
                               out_ptr, ld, _stream(amd))
        assert rc == 0, L.msim_last_error()

    ref = torch.empty((M, 128), dtype=dtype, device=dev)
    assert ref.data_ptr() % 16 == 0
    launch(ref.data_ptr(), 128)
    check_any(ref.view(1, M, 128), hidden, weight, bias, mask)
    ref_bits = _bits(ref).cpu()
    for name, (ld, off) in _LAYOUTS.items():
        n = off + (M + 3) * ld + 16                       # elements in front of `out`, behind column 127 of every row, 3 rows behind the last
        buf = torch.full((n,), SENTINEL, dtype=torch.int16, device=dev)
        assert buf.data_ptr() % 16 == 0
        launch(buf.data_ptr() + 2 * off, ld)
        got = buf.cpu()
        rows = got[off: off + M * ld].view(M, ld)
        assert torch.equal(rows[:, :128], ref_bits), f"{name}: written columns differ from the contiguous call"
        want = torch.full((n,), SENTINEL, dtype=torch.int16)
        want[off: off + M * ld].view(M, ld)[:, :128] = ref_bits
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} elements outside the 128 columns of the {M} rows were written"


# ---------------------------------------------------------------------------------------------------------------------------
# B. few K chunks across many tiles; the widest hidden sizes

@pytest.mark.parametrize("H,dtype", [(64, BF16), (128, BF16), (192, BF16), (128, F16)], ids=["H64", "H128", "H192", "H128_f16"])
def test_one_to_three_k_chunks_with_several_tiles_per_workgroup(amd, CUS, H, dtype):
    """(2 CUS + 3) full tiles and a partial one: every workgroup walks two tiles, some three.  With 1, 2 or 3 chunks per tile (3 = the
    ring depth) the next tiles' chunks are in flight during an epilogue, which stages its rows in the slot just consumed."""
    M = (2 * CUS + 3) * 256 + 77
    hidden, weight, bias, mask = _case(H + 7, 1, M, H, dtype)
    mask[0, ::7] = 0
    got = amd.embedding_head(hidden.cuda(), weight.cuda(), bias.cuda(), mask.cuda())
    check_any(got, hidden, weight, bias, mask)


def test_prologue_asks_for_fewer_chunks_than_the_ring_holds(amd):
    hidden, weight, bias, mask = _case(100, 1, 100, 192, BF16)            # one partial tile of three chunks
    mask[0, ::7] = 0
    got = amd.embedding_head(hidden.cuda(), weight.cuda(), bias.cuda(), mask.cuda())
    check(got, hidden, weight, bias, mask)
    hidden, weight, bias, mask = _case(101, 1, 100, 64, BF16)             # ... and of one chunk
    got = amd.embedding_head(hidden.cuda(), weight.cuda(), bias.cuda(), mask.cuda())
    check(got, hidden, weight, bias, mask)


@pytest.mark.parametrize("H", [8192, 16384])
def test_widest_hidden_sizes_the_abi_takes(amd, H):
    """Above H = 4096 msim_embed_head launches the WIDE forms of the kernel (embed_head.hip), which fold the fp32 accumulator into a
    second one every 1024 K.  This test found why they are needed: with ONE accumulator taking all 1024 MFMA results of H = 16384 in
    K order, 4 of the 38 400 elements (1.04e-4) were two ulps from the CPU literal where `check` allows 1e-4 -- the accumulation error
    grows with the number of steps and flips the bf16 rounding of the Linear output, which moves the quotient by up to two ulps (a CPU
    emulation of that order gave 2 such elements on these inputs, the CPU GEMM's blocked sums none).  300 rows: a full tile and a
    partial one."""
    hidden, weight, bias, mask = _case(H, 2, 150, H, BF16, "left")
    x, w, b = hidden.cuda(), weight.cuda(), bias.cuda()
    got = amd.embedding_head(x, w, b, mask.cuda())
    check(got, hidden, weight, bias, mask)
    # the 2-byte-store form of the same width (ld_out = 132): the same bits, nothing else written
    from colpali_amd import embed

    L, M, ld = amd._lib.lib(), 300, 132
    row_map = embed._dense_row_map(mask.cuda(), None, M, x.device)
    buf = torch.full(((M + 2) * ld,), SENTINEL, dtype=torch.int16, device=x.device)
    rc = L.msim_embed_head(0, x.data_ptr(), M, H, w.data_ptr(), b.data_ptr(), 128, row_map.data_ptr(), buf.data_ptr(), ld, _stream(amd))
    assert rc == 0, L.msim_last_error()
    want = torch.full(((M + 2), ld), SENTINEL, dtype=torch.int16)
    want[:M, :128] = _bits(got).cpu().view(M, 128)
    assert torch.equal(buf.cpu().view(M + 2, ld), want)


# ---------------------------------------------------------------------------------------------------------------------------
# C. mask dtypes

def _mask_case(dtype):
    B, S, H = 3, 90, 128
    hidden, weight, bias, mask = _case(17, B, S, H, dtype, "left")
    mask[0, :4] = 0                                       # left padding on every page, plus interior holes
    mask[:, 40:43] = 0
    mask[1, 77] = 0
    mask[2, S - 1] = 0
    extra = (torch.arange(S)[None, :] % 3 != 0).expand(B, S).contiguous()
    return hidden, weight, bias, mask, extra


@pytest.fixture(scope="module")
def mask_base(amd):
    out = {}
    for dtype in (BF16, F16):
        hidden, weight, bias, mask, extra = _mask_case(dtype)
        dev = (hidden.cuda(), weight.cuda(), bias.cuda())
        got = amd.embedding_head(*dev, mask.cuda(), extra.cuda())
        check_any(got, hidden, weight, bias, mask, extra)
        only_att = amd.embedding_head(*dev, mask.cuda())
        check_any(only_att, hidden, weight, bias, mask)
        out[dtype] = (dev, mask, extra, _bits(got).cpu(), _bits(only_att).cpu())
    return out


def _as_mask(keep, dt, masked_value):
    if dt.is_floating_point:
        return torch.where(keep, torch.tensor(1.0, dtype=dt), torch.tensor(masked_value, dtype=dt))
    return keep.to(dt)


_MASK_DTYPES = [torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32, BF16, F16, torch.float64]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("mdt", _MASK_DTYPES, ids=lambda d: str(d).replace("torch.", ""))
def test_every_mask_dtype_gives_the_bits_of_the_int64_and_bool_call(amd, mask_base, dtype, mdt):
    """mask_nonzero has one branch per dtype of embed._MASK_KINDS (floating zeros of either sign are "masked"); float64 is outside the
    table and goes through _prep_mask's `!= 0`.  Under autocast models hand masks over in the model dtype."""
    from colpali_amd import embed

    assert set(_MASK_DTYPES) - {torch.float64} == set(embed._MASK_KINDS)
    dev, mask, extra, want, want_att = mask_base[dtype]
    for masked_value in ((0.0, -0.0) if mdt.is_floating_point else (0,)):
        m = _as_mask(mask != 0, mdt, masked_value).cuda()
        e = _as_mask(extra, mdt, masked_value).cuda()
        if str(masked_value) == "-0.0":
            assert bool(torch.signbit(m[mask.cuda() == 0]).all())        # the masked entries really are -0.0
        assert torch.equal(_bits(amd.embedding_head(*dev, m)).cpu(), want_att), f"{mdt} attention mask, masked value {masked_value!r}"
        assert torch.equal(_bits(amd.embedding_head(*dev, m, e)).cpu(), want), f"{mdt} for both masks, masked value {masked_value!r}"
        assert torch.equal(_bits(amd.embedding_head(*dev, mask.cuda(), e)).cpu(), want), f"{mdt} extra mask, masked value {masked_value!r}"
        assert torch.equal(_bits(amd.embedding_head(*dev, m, extra.cuda())).cpu(), want), f"{mdt} attention mask, bool extra mask"


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_non_contiguous_masks(amd, mask_base, dtype):
    dev, mask, extra, want, _ = mask_base[dtype]
    B, S = mask.shape
    wide = torch.empty(B, 2 * S, dtype=torch.long)
    wide[:, ::2], wide[:, 1::2] = mask, 1 - mask          # the skipped entries say the opposite
    wide_e = torch.empty(B, 2 * S, 1, dtype=torch.bool)
    wide_e[:, ::2, 0], wide_e[:, 1::2, 0] = extra, ~extra
    m, e = wide.cuda()[:, ::2], wide_e.cuda()[:, ::2]
    assert not m.is_contiguous() and not e.is_contiguous()
    assert torch.equal(_bits(amd.embedding_head(*dev, m, e)).cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------------
# D. the writer's row map

def _head_params(H, dtype, seed=3):
    g = torch.Generator().manual_seed(seed)
    weight = (torch.randn(128, H, generator=g) / H**0.5).to(dtype).cuda()
    bias = (torch.randn(128, generator=g) * 0.1).to(dtype).cuda()
    return weight, bias


def _queries(dtype, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.functional.normalize(torch.randn(n, 128, generator=g), dim=-1).to(dtype) for n in (20, 32, 11)]


def _write_and_compare(amd, batches, dtype=BF16, H=64, scores=False):
    """`batches`: (hidden [B, S, H] on the CPU, attention mask, extra mask or None) per append to ONE writer.  The finished corpus
    must hold torch.cat([dense[b][keep[b]] ...]) of the dense kernel output bit for bit, `lengths` the keep counts per page; with
    `scores`, the packed corpus must score exactly as the reference road does on the dense pages."""
    dev = torch.device("cuda:0")
    weight, bias = _head_params(H, dtype)
    writer = amd.CorpusWriter(capacity_rows=sum(h.shape[0] * h.shape[1] for h, _, _ in batches), device=dev, dtype=dtype)
    want_rows, want_len, pages = [], [], []
    for hidden, mask, extra in batches:
        B = hidden.shape[0]
        args = (hidden.to(dev), weight, bias, mask.to(dev), None if extra is None else extra.to(dev))
        assert writer.append(*args) == B
        dense = amd.embedding_head(*args)
        keep = _keep(mask, extra).to(dev)
        want_rows.extend(dense[b][keep[b]] for b in range(B))
        want_len.extend(int(keep[b].sum()) for b in range(B))
        pages.extend(torch.unbind(dense))
    total = sum(want_len)
    assert writer.rows_written() == total
    corpus = writer.finish()
    assert len(corpus) == len(want_len)
    assert corpus.lengths.tolist() == want_len
    assert corpus.offsets.cpu().tolist() == [0] + torch.tensor(want_len).cumsum(0).tolist()
    assert torch.equal(_bits(corpus.blob[:total]), _bits(torch.cat(want_rows)))
    if scores:
        qs = _queries(dtype)
        via_reference_road = amd.score_multi_vector(qs, [p.cpu() for p in pages], device=dev)
        direct = amd.maxsim_scores(amd.pack_queries(qs, dev), corpus).cpu()
        assert torch.equal(via_reference_road, direct)
        return corpus, direct
    return corpus, None


def _hidden(B, S, H, dtype, seed):
    return (torch.randn(B, S, H, generator=torch.Generator().manual_seed(seed)) * 2.0).to(dtype)


@pytest.mark.parametrize("S", [64, 256, 257, 513])
def test_writer_map_with_interior_holes(amd, S):
    """Ranks that are neither `s` nor `s - pad`: ballots inside a wave, the 4-entry carry across the waves of a 256-position round
    and the running base across rounds (S = 257, 513: a second and third round, the last with one live lane)."""
    g = torch.Generator().manual_seed(S)
    keep = torch.rand(4, S, generator=g) < 0.5
    coin = torch.rand(4, S, generator=g) < 0.5
    hidden = _hidden(4, S, 64, BF16, S + 1)
    _write_and_compare(amd, [(hidden, keep.long(), None),                                     # the attention mask alone
                             (hidden, (keep | coin).long(), (keep | ~coin).unsqueeze(-1))])   # split between the two masks


def test_writer_map_over_many_pages_in_two_appends(amd):
    """300 and 513 pages: the sum over the pages in front takes two and three strides of 256 threads, and the second append starts
    from a non-zero row count that only the device knows."""
    g = torch.Generator().manual_seed(8)
    batches = []
    for B in (300, 513):
        keep = torch.rand(B, 5, generator=g) < 0.6
        batches.append((_hidden(B, 5, 64, BF16, B), keep.long(), None))
    corpus, _ = _write_and_compare(amd, batches)
    assert len(corpus) == 813


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_writer_with_fully_masked_pages_scores_as_the_reference_road(amd, dtype):
    """Fully masked pages first, in the middle and last, among pages with holes; the reference road scores such a page 0.
    The fp16 case is the writer's other dtype."""
    g = torch.Generator().manual_seed(21)
    B, S = 7, 70
    keep = torch.rand(B, S, generator=g) < 0.5
    keep[[0, 3, 6]] = False
    keep[1] = True                                        # and a page without any masked position
    corpus, scores = _write_and_compare(amd, [(_hidden(B, S, 64, dtype, 5), keep.long(), None)], dtype=dtype, scores=True)
    assert [corpus.lengths.tolist()[i] for i in (0, 3, 6)] == [0, 0, 0]
    assert torch.count_nonzero(scores[:, [0, 3, 6]]) == 0 and bool((scores[:, [1, 2, 4, 5]] > 0).all())


def test_writer_with_everything_masked(amd):
    hidden = _hidden(3, 40, 64, BF16, 6)
    att = torch.ones(3, 40, dtype=torch.long)
    corpus, scores = _write_and_compare(amd, [(hidden, torch.zeros(3, 40, dtype=torch.long), None),
                                              (hidden, att, torch.zeros(3, 40, 1, dtype=torch.bool))], scores=True)
    assert corpus.lengths.tolist() == [0] * 6 and torch.count_nonzero(scores) == 0


def test_writer_empty_appends(amd):
    dev = torch.device("cuda:0")
    weight, bias = _head_params(64, BF16)
    writer = amd.CorpusWriter(capacity_rows=64, device=dev)
    hidden = _hidden(2, 10, 64, BF16, 1).to(dev)
    mask = torch.ones(2, 10, dtype=torch.long, device=dev)
    mask[1, 3:6] = 0
    assert writer.append(hidden, weight, bias, mask) == 2
    assert writer.rows_written() == 17
    assert writer.append(hidden[:0], weight, bias, mask[:0]) == 0                    # B == 0
    assert writer.rows_written() == 17
    assert writer.append(hidden[:, :0], weight, bias, mask[:, :0]) == 2              # S == 0, B > 0: two pages without rows
    assert writer.append(hidden[:0, :0], weight, bias, mask[:0, :0]) == 0
    assert writer.rows_written() == 17
    assert writer.append(hidden[:1], weight, bias, mask[:1]) == 1                    # the writer goes on where it was
    assert writer.rows_written() == 27
    corpus = writer.finish()
    assert len(corpus) == 5 and corpus.lengths.tolist() == [10, 7, 0, 0, 10]
    dense = amd.embedding_head(hidden, weight, bias, mask)
    want = torch.cat([dense[0], dense[1][mask[1] != 0], dense[0]])
    assert torch.equal(_bits(corpus.blob[:27]), _bits(want))


# ---------------------------------------------------------------------------------------------------------------------------
# E. non-finite parity with the literal reference

def _nonfinite_case(dtype):
    """[1, 8, 64], no bias.  Row 2: all-zero hidden states, unmasked (0 / 0).  Row 5: all-zero and masked (NaN * 0).  Row 6: an ordinary
    masked row.  fp16 only -- row 1: scaled so that several Linear outputs overflow fp16 (inf / inf, finite / inf); row 3: every Linear
    output finite, but the norm is not (finite / inf)."""
    hidden, weight, _, mask = _case(64, 1, 8, 64, dtype)
    hidden[0, 2] = 0
    hidden[0, 5] = 0
    mask[0, 5] = 0
    mask[0, 6] = 0
    normal = [0, 4, 6, 7]
    if dtype == F16:
        # the `_case` scales (hidden 2 x randn, weight randn / 8) times 30000, with the row's entries held to |x| <= 2 so that the scaled
        # hidden states themselves stay finite
        hidden[0, 1] = (hidden[0, 1].float().clamp(-2.0, 2.0) * 30000.0).to(dtype)
        g = torch.Generator().manual_seed(65)
        hidden[0, 3] = (torch.randn(64, generator=g) * 7000.0).to(dtype)         # unit variance x 7000: norm ~ 70 000 > 65 504
    else:
        normal += [1, 3]
    return hidden, weight, mask, sorted(normal)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_non_finite_rows_match_the_literal_reference(amd, dtype):
    """"NaN stays NaN -- what torch's multiply yields" (embed_head.hip): the NaN positions and the exactly-zero positions are the
    literal's, the other rows pass the normal comparison, and the writer drops masked rows whatever they hold."""
    hidden, weight, mask, normal = _nonfinite_case(dtype)
    lit = ho.head_literal(hidden, weight, None, mask)
    proj = torch.nn.functional.linear(hidden, weight)
    assert bool(torch.isfinite(hidden.float()).all())
    assert bool(lit[0, 2].isnan().all()) and bool(lit[0, 5].isnan().all())          # what the reference does with a zero row
    if dtype == F16:
        y64 = torch.nn.functional.linear(hidden.double(), weight.double())[0, 1].abs()
        assert int(proj[0, 1].isinf().sum()) >= 4 and int(proj[0, 1].isfinite().sum()) >= 4
        assert not bool(((y64 > 65504 * 0.99) & (y64 < 65520 * 1.01)).any())         # no output so close to the overflow threshold that the accumulation order decides
        assert bool(proj[0, 3].isfinite().all()) and bool(proj[0, 3].norm().isinf())
        assert bool(lit[0, 1].isnan().any()) and bool((lit[0, 1] == 0).any()) and bool((lit[0, 3] == 0).all())
    dev = torch.device("cuda:0")
    x, w, m = hidden.to(dev), weight.to(dev), mask.to(dev)
    got = amd.embedding_head(x, w, None, m).cpu()
    assert torch.equal(got.isnan(), lit.isnan()), (got.isnan().nonzero().tolist(), lit.isnan().nonzero().tolist())
    assert torch.equal(got == 0, lit == 0)
    assert not bool(got.isinf().any())
    check_any(got[:, normal], hidden[:, normal], weight, None, mask[:, normal])
    writer = amd.CorpusWriter(capacity_rows=8, device=dev, dtype=dtype)
    assert writer.append(x, w, None, m) == 1
    corpus = writer.finish()
    assert corpus.lengths.tolist() == [6]
    assert torch.equal(_bits(corpus.blob[:6]).cpu(), _bits(amd.embedding_head(x, w, None, m)[0][m[0] != 0]).cpu())


# ---------------------------------------------------------------------------------------------------------------------------
# F. subnormal fp16 operands

def _subnormal_case():
    g = torch.Generator().manual_seed(5)
    hidden = (torch.randn(1, 64, 256, generator=g) * 2.0**-15).to(F16)          # 95 % of the elements are subnormal fp16 numbers
    weight = (torch.randn(128, 256, generator=g) * 8.0).to(F16)                 # ... and the Linear outputs normal ones
    return hidden, weight, torch.ones(1, 64, dtype=torch.long)


def _within_truth_tier(got, truth):
    big = truth.abs() >= 1e-3
    return bool(torch.all(((got.cpu().double() - truth).abs() <= 2.0**-9 * truth.abs())[big]))


def test_subnormal_fp16_hidden_states_are_multiplied_not_flushed(amd):
    """DESIGN.md 3.6 records that the matrix cores flush subnormal fp16 operands in the dense backward; the head feeds raw fp16 hidden
    states and weights to v_mfma_f32_32x32x16_f16.  Two float64 truths that lie far apart on these inputs (median 0.06 absolute, on
    unit-norm rows): the real one, and the one with every subnormal hidden element replaced by zero.  The kernel has to be within the
    fp16 truth tier (2^-9 relative on |value| >= 1e-3, whole tensor) of exactly one of them.
    Outcome on an MI355X: the REAL one -- the head multiplies subnormal fp16 operands like the reference does (its largest relative
    error, 1.15e-3, is the CPU literal's own); against the flushed truth it is off by a median of 0.06.  No limit to document."""
    hidden, weight, mask = _subnormal_case()
    tiny = hidden.float().abs() < 2.0**-14
    assert 0.9 < float((tiny & (hidden != 0)).float().mean()) < 0.99
    assert float(torch.nn.functional.linear(hidden.double(), weight.double()).abs().median()) > 2.0**-14     # normal Linear outputs
    truth = ho.head_truth(hidden, weight, None, mask)
    truth_flushed = ho.head_truth(torch.where(tiny, torch.zeros_like(hidden), hidden), weight, None, mask)
    assert float((truth - truth_flushed).abs().median()) > 0.05
    assert _within_truth_tier(ho.head_literal(hidden, weight, None, mask), truth)          # the reference itself does not flush
    got = amd.embedding_head(hidden.cuda(), weight.cuda(), None, mask.cuda())
    near_real, near_flushed = _within_truth_tier(got, truth), _within_truth_tier(got, truth_flushed)
    assert near_real != near_flushed, (near_real, near_flushed)
    assert near_real and not near_flushed


# ---------------------------------------------------------------------------------------------------------------------------
# G. the backward's second grid-stride pass

@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_backward_takes_a_second_grid_stride_pass(amd, CUS, dtype):
    """embed_head_bwd_rows_kernel: at most CUS x 16 workgroups of 16 rows.  CUS x 256 + 1000 rows: a second, partial pass whose last
    workgroup has 8 live rows."""
    M = CUS * 256 + 1000
    assert M % 2 == 0 and M % 16 != 0
    hidden, weight, bias, _ = _case(M, 2, M // 2, 64, dtype)
    mask = torch.ones(2, M // 2, dtype=torch.long)
    mask.view(-1)[::5] = 0
    G = torch.randn(2, M // 2, 128, generator=torch.Generator().manual_seed(3)).to(dtype)
    hx, wx, bx = (t.cuda().requires_grad_(True) for t in (hidden, weight, bias))
    out = amd.embedding_head(hx, wx, bx, mask.cuda())
    (out.float() * G.cuda().float()).sum().backward()
    (want_h, want_w, want_b), (bd_h, bd_w, bd_b) = _truth_grads(hidden, weight, bias, mask, G)
    assert _grad_close(hx.grad, want_h, bd_h, dtype) and _grad_close(wx.grad, want_w, bd_w, dtype)
    assert _grad_close(bx.grad, want_b, bd_b, dtype)
    assert torch.count_nonzero(hx.grad.cpu()[mask == 0]) == 0
    assert torch.count_nonzero(hx.grad.cpu()[mask != 0]) > 0.99 * 64 * int(mask.sum())


def test_non_contiguous_hidden_states_and_weight_forward_and_backward(amd):
    B, S, H = 2, 51, 64
    hidden_w, weight, bias, _ = _case(12, B, S + 1, H, BF16)
    # the oracle gets the same values in a contiguous tensor: torch's CPU bf16 Linear WITH bias rounds twice on a strided input (matmul,
    # then the bias add: 73 % of its outputs equal the exactly accumulated ones, against 99.99 % on the contiguous copy), which is a
    # property of that CPU path, not of the reference lines
    hidden = hidden_w[:, 1:, :].contiguous()
    mask = torch.ones(B, S, dtype=torch.long)
    mask[1, 30:] = 0
    mask[0, ::9] = 0
    G = torch.randn(B, S, 128, generator=torch.Generator().manual_seed(4)).to(BF16)
    hx = hidden_w.cuda()[:, 1:, :].requires_grad_(True)
    wx = weight.t().contiguous().cuda().t().requires_grad_(True)           # [128, H] view of an [H, 128] tensor
    bx = bias.cuda().requires_grad_(True)
    assert not hx.is_contiguous() and not wx.is_contiguous() and hx.is_leaf and wx.is_leaf
    with torch.no_grad():
        check(amd.embedding_head(hx, wx, bx, mask.cuda()), hidden, weight, bias, mask)
    out = amd.embedding_head(hx, wx, bx, mask.cuda())
    check(out.detach(), hidden, weight, bias, mask)
    (out.float() * G.cuda().float()).sum().backward()
    (want_h, want_w, want_b), (bd_h, bd_w, bd_b) = _truth_grads(hidden, weight, bias, mask, G)
    assert hx.grad.shape == hx.shape and wx.grad.shape == wx.shape
    assert _grad_close(hx.grad, want_h, bd_h, BF16) and _grad_close(wx.grad, want_w, bd_w, BF16)
    assert _grad_close(bx.grad, want_b, bd_b, BF16)
    assert torch.count_nonzero(hx.grad.cpu()[mask == 0]) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# H. argument validation of the four entry points

EINVAL, EUNSUPPORTED = -1, -2          # what _lib.check maps to ValueError / NotImplementedError


def test_entry_points_validate_their_arguments_before_any_launch(amd):
    L, dev = amd._lib.lib(), torch.device("cuda:0")
    st = _stream(amd)
    M, H = 4, 64
    x = torch.ones((M + 1, H), dtype=BF16, device=dev)
    w = torch.ones((129, H), dtype=BF16, device=dev)
    bias = torch.zeros((128,), dtype=BF16, device=dev)
    proj = torch.ones((M + 1, 128), dtype=BF16, device=dev)
    gout = torch.ones((M + 1, 128), dtype=BF16, device=dev)
    mask = torch.ones((M,), dtype=torch.long, device=dev)
    extra = torch.ones((M,), dtype=torch.bool, device=dev)
    rows_before = torch.zeros((), dtype=torch.int64, device=dev)
    written = {                                           # everything an entry point could write: filled with a pattern, compared at the end
        "row_map": torch.full((256,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
        "out": torch.full((M, 128), SENTINEL, dtype=torch.int16, device=dev),
        "dproj": torch.full((M + 1, 128), SENTINEL, dtype=torch.int16, device=dev),
        "counts": torch.full((2,), 0x5A5A5A5A, dtype=torch.int64, device=dev),
        "rows_after": torch.full((), 0x5A5A5A5A, dtype=torch.int64, device=dev),
    }
    before = {k: v.clone() for k, v in written.items()}
    p = {k: v.data_ptr() for k, v in written.items()}

    def expect(rc, code, what):
        assert rc == code, f"{what}: returned {rc}, expected {code} ({L.msim_last_error()!r})"
        if code != 0:
            assert L.msim_last_error(), what

    def head(dtype=0, X=x.data_ptr(), M=M, H=H, W=w.data_ptr(), b=bias.data_ptr(), n_out=128, rm=p["row_map"], out=p["out"], ld=128):
        return L.msim_embed_head(dtype, X, M, H, W, b, n_out, rm, out, ld, st)

    for name in ("X", "W", "rm", "out"):
        expect(head(**{name: None}), EINVAL, f"msim_embed_head, null {name}")
    expect(head(dtype=2), EUNSUPPORTED, "msim_embed_head, fp32")
    expect(head(dtype=3), EUNSUPPORTED, "msim_embed_head, unknown dtype code")
    expect(head(n_out=64), EUNSUPPORTED, "msim_embed_head, n_out = 64")
    expect(head(H=96), EUNSUPPORTED, "msim_embed_head, H = 96")
    expect(head(H=16448), EUNSUPPORTED, "msim_embed_head, H = 16448")
    expect(head(H=0), EINVAL, "msim_embed_head, H = 0")
    expect(head(H=-64), EINVAL, "msim_embed_head, H = -64")
    expect(head(ld=127), EINVAL, "msim_embed_head, ld_out = 127")
    expect(head(X=x.data_ptr() + 2), EINVAL, "msim_embed_head, X one element off")
    expect(head(W=w.data_ptr() + 2), EINVAL, "msim_embed_head, W one element off")
    expect(head(M=-1), EINVAL, "msim_embed_head, M = -1")
    expect(head(M=0), 0, "msim_embed_head, M = 0")
    expect(head(M=0, X=None, W=None, rm=None, out=None), 0, "msim_embed_head, M = 0 without buffers")

    def bwd(dtype=0, pr=proj.data_ptr(), g=gout.data_ptr(), rm=p["row_map"], M=M, n_out=128, dp=p["dproj"]):
        return L.msim_embed_head_bwd(dtype, pr, g, rm, M, n_out, dp, st)

    for name in ("pr", "g", "rm", "dp"):
        expect(bwd(**{name: None}), EINVAL, f"msim_embed_head_bwd, null {name}")
    expect(bwd(dtype=2), EUNSUPPORTED, "msim_embed_head_bwd, fp32")
    expect(bwd(n_out=64), EUNSUPPORTED, "msim_embed_head_bwd, n_out = 64")
    expect(bwd(pr=proj.data_ptr() + 2), EINVAL, "msim_embed_head_bwd, proj one element off")
    expect(bwd(g=gout.data_ptr() + 2), EINVAL, "msim_embed_head_bwd, grad_out one element off")
    expect(bwd(dp=p["dproj"] + 2), EINVAL, "msim_embed_head_bwd, dproj one element off")
    expect(bwd(M=-1), EINVAL, "msim_embed_head_bwd, M = -1")
    expect(bwd(M=0), 0, "msim_embed_head_bwd, M = 0")

    def rmap(m=mask.data_ptr(), kind=3, e=None, ekind=0, M=M, rm=p["row_map"]):
        return L.msim_embed_head_row_map(m, kind, e, ekind, M, rm, st)

    expect(rmap(m=None), EINVAL, "msim_embed_head_row_map, null mask")
    expect(rmap(rm=None), EINVAL, "msim_embed_head_row_map, null row map")
    for kind in (-1, 7):
        expect(rmap(kind=kind), EINVAL, f"msim_embed_head_row_map, mask kind {kind}")
        expect(rmap(e=extra.data_ptr(), ekind=kind), EINVAL, f"msim_embed_head_row_map, extra kind {kind}")
    expect(rmap(M=-1), EINVAL, "msim_embed_head_row_map, M = -1")
    expect(rmap(M=0), 0, "msim_embed_head_row_map, M = 0")
    expect(rmap(M=0x7FFFFFFE), EUNSUPPORTED, "msim_embed_head_row_map, M = 0x7ffffffe")

    def wmap(m=mask.data_ptr(), kind=3, e=None, ekind=0, B=2, S=2, rb=rows_before.data_ptr(), c=p["counts"], rm=p["row_map"], ra=p["rows_after"]):
        return L.msim_embed_head_writer_map(m, kind, e, ekind, B, S, rb, c, rm, ra, st)

    for name in ("m", "rb", "c", "rm", "ra"):
        expect(wmap(**{name: None}), EINVAL, f"msim_embed_head_writer_map, null {name}")
    for kind in (-1, 7):
        expect(wmap(kind=kind), EINVAL, f"msim_embed_head_writer_map, mask kind {kind}")
        expect(wmap(e=extra.data_ptr(), ekind=kind), EINVAL, f"msim_embed_head_writer_map, extra kind {kind}")
    expect(wmap(S=0), EINVAL, "msim_embed_head_writer_map, S = 0")
    expect(wmap(S=-1), EINVAL, "msim_embed_head_writer_map, S = -1")
    expect(wmap(B=-1), EINVAL, "msim_embed_head_writer_map, B = -1")
    expect(wmap(B=0), 0, "msim_embed_head_writer_map, B = 0")

    torch.cuda.synchronize()
    for k, v in written.items():
        assert torch.equal(v, before[k]), f"a refused or empty call wrote to {k}"
    # the same arguments, valid: the calls above were refused for the one thing each of them changed
    expect(rmap(), 0, "msim_embed_head_row_map")
    expect(head(), 0, "msim_embed_head")
    expect(bwd(), 0, "msim_embed_head_bwd")
    expect(wmap(), 0, "msim_embed_head_writer_map")
    torch.cuda.synchronize()
    assert written["row_map"][:4].tolist() == [0, 1, 2, 3] and written["counts"].tolist() == [2, 2] and int(written["rows_after"]) == 4
    assert not torch.equal(written["out"], before["out"]) and not torch.equal(written["dproj"], before["dproj"])
