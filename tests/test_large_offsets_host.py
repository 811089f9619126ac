"""The large-offset fixtures of tests/helpers.py are wrap-proof (no GPU): what keeps a truncated offset from hiding.

tests/test_gpu_large_offsets.py scans shards that are one block of pages repeated T times and expects the block's truth, tiled.
An offset that lost bit 31 or 32 -- as a byte count or as an element count -- moves an address by a fixed distance.  If that distance
were a multiple of the block, the kernel would read an equal copy and the test would pass over a real bug.  For the exact parameters
the GPU module uses, this module asserts that every such distance, modulo the block, lies at least one longest page away from both
ends of the block: every ROW of every page then lands in another page, whose rows are other random rows.
"""
import numpy as np
import pytest

from tests import helpers as h

KINDS = sorted(h.LARGE_SHARDS)


@pytest.mark.parametrize("kind", KINDS)
def test_shard_is_tiled_and_crosses_its_boundaries(kind):
    s = h.large_shard_spec(kind)
    lens = s["lens"]
    assert s["P"] == h.LARGE_PAGES and set(h.LARGE_EDGE_LENS) <= set(lens) and lens.count(0) == 1
    assert s["R0"] == sum(lens) and s["R0"] % 2 == 1 and s["R0"] > 1
    assert s["rows"] == s["T"] * s["R0"] < 2**31 and s["n"] == s["T"] * s["P"]
    assert s["rows"] > h.LARGE_SHARDS[kind][3]
    assert s["rows"] * s["row_bytes"] <= 8.7e9                                   # the module's memory budget counts on it
    want = {"bf16_128": ["byte 2^31", "byte 2^32", "element 2^31", "element 2^32"], "bf16_320": ["byte 2^31", "byte 2^32", "element 2^31"],
            "f32_128": ["byte 2^31", "byte 2^32", "element 2^31"]}[kind]
    assert sorted(s["bounds"]) == sorted(want)
    for row in s["bounds"].values():                                             # a whole tile lies past every boundary
        assert row + s["R0"] <= s["rows"]
    tiles = h.large_tiles_of_interest(s)
    assert tiles[0] == 0 and tiles[-1] == s["T"] - 1
    for row in s["bounds"].values():
        assert {row // s["R0"] - 1, row // s["R0"], row // s["R0"] + 1} <= set(tiles)


@pytest.mark.parametrize("kind", KINDS)
def test_no_wrap_distance_lands_on_an_equal_copy(kind):
    s = h.large_shard_spec(kind)
    R0, rb, off, lens = s["R0"], s["row_bytes"], s["offsets"], s["lens"]
    longest = max(lens)
    for name, dist in h.large_wrap_bytes(s["elem_bytes"]).items():
        if dist % rb == 0:
            assert (dist // rb) % R0 != 0, (kind, name)                          # the distance in rows is no multiple of the block
        d = dist % (R0 * rb)
        assert longest * rb <= d <= (R0 - longest) * rb, (kind, name, d / rb)    # ... and a longest page away from both of its ends
        for t in (0, s["T"] // 2, s["T"] - 1):
            for p in range(s["P"]):
                if lens[p] == 0:
                    continue
                for j in {0, lens[p] - 1}:                                       # first and last row: both land in another page
                    addr = (t * R0 + int(off[p]) + j) * rb
                    for wrapped in (addr - dist, addr + dist):
                        assert h.large_page_at(s, wrapped) != p, (kind, name, t, p, j)
    # a ROW INDEX that lost a high bit: the same argument in rows
    for bit in range(16, 31):
        d = (1 << bit) % R0
        if (1 << bit) < s["rows"]:
            assert d != 0, (kind, bit)


def test_block_rows_differ_between_pages():
    """another page means other rows: no two rows of the block are equal"""
    s = h.large_shard_spec("bf16_128")
    rows = h.large_block_rows(s)
    assert rows.shape == (s["R0"], 128)
    import torch

    assert len(torch.unique(rows.view(torch.int16), dim=0)) == s["R0"]
    # ... and every value is one the 13-bit image holds (pack13_format.hpp: biased exponent 96 .. 127), so no page of the block is flagged
    e = (rows.view(torch.int16).numpy().view(np.uint16) >> 7) & 0xFF
    assert ((e >= 96) & (e <= 127)).all()


@pytest.mark.parametrize("form", sorted(h.LARGE_MATRIX_LD))
def test_score_matrix_is_wrap_proof(form):
    ld, n_q, b = h.LARGE_MATRIX_LD[form], h.LARGE_MATRIX_ROWS, h.LARGE_MATRIX_BLOCK
    assert n_q * ld > 2**31 and n_q * ld * 4 <= 8.7e9
    assert (ld % 4 == 0 and (ld // 4) % 2 == 1) if form == "vec" else ld % 2 == 1
    for e in (30, 31, 32):
        assert 2**e % ld != 0
        # the row an entry lands in after the wrap repeats another row of the 7-row block, or the same row at another column
        rows, cols = divmod(2**e, ld)
        assert rows % b != 0 or cols != 0
    probes = h.large_matrix_probe_rows(ld)
    assert probes[0] == 0 and probes[-1] == n_q - 1 and any(r * ld >= 2**30 for r in probes) and any(r * ld >= 2**31 for r in probes)
    blk = h.large_matrix_block(ld)
    assert blk.shape == (b, ld) and blk.dtype == np.float32
    assert np.isneginf(blk).any() and (np.signbit(blk) & (blk == 0)).any() and ((blk == 0) & ~np.signbit(blk)).any()
    for r in range(b):                                                           # ties at the top, at both ends of the row
        assert blk[r].max() == blk[r, 0] == blk[r, ld - 1] and (blk[r] == blk[r].max()).sum() == 3
    assert len({blk[r].tobytes() for r in range(b)}) == b


def test_fast_group_truth_is_the_group_truth():
    """the vectorised document reduction the large matrices are checked against equals tests/group_truth.py on a small matrix with
    ties, signed zeros, -inf rows and a document whose pages all score -inf"""
    from tests import group_truth as gt

    rng = np.random.default_rng(3)
    n = 400
    s = rng.integers(-3, 4, (5, n)).astype(np.float32)
    s[rng.random(s.shape) < 0.2] = -np.inf
    s[rng.random(s.shape) < 0.1] = -0.0
    labels = h.large_matrix_group_labels(n)
    labels[:37] = 10**12 + 5                                     # a document with pages in both halves
    s[:, labels == 10 * 2] = -np.inf
    want = gt.reduce_truth(s, labels, id_base=70)
    got = h.group_reduce_truth_fast(s, labels, id_base=70)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1].view(np.int32), want[1].view(np.int32))
    np.testing.assert_array_equal(got[2], want[2])
    lab = h.large_matrix_group_labels(h.LARGE_MATRIX_LD["vec"])
    assert np.unique(lab).size > 10000 and lab.min() >= 0
