"""The numpy truth of the int8 token-level index (tests/int8_truth.py) on its own edge cases: ties, zero pages and tokens, clamp0,
the int32 extreme, the documented summation order, and the agreement of its fast form with the plain one.  These check the
yardstick the GPU tests compare against, not the library, so they pass without it."""
import numpy as np

from tests import int8_truth as it


def test_ties_round_half_to_even():
    x = np.zeros((1, 128), np.float32)
    x[0, :8] = [127, 0.5, 1.5, 2.5, -2.5, -0.5, 3.5, -126.5]
    c, s = it.quantize(x)
    assert s == np.float32(1.0)
    assert c[0, :8].tolist() == [127, 0, 2, 2, -2, 0, 4, -126]


def test_zero_pages_and_tokens():
    c, s = it.quantize(np.zeros((3, 128), np.float32))
    assert s == 0 and (c == 0).all()
    c, s = it.quantize(np.zeros((0, 128), np.float32))
    assert s == 0 and c.shape == (0, 128)
    q = [np.ones((2, 128), np.float32), np.zeros((0, 128), np.float32)]
    p = [np.ones((3, 128), np.float32), np.zeros((0, 128), np.float32), np.zeros((2, 128), np.float32)]
    S = it.score_blocks(q, p)
    assert S[1, 0] == 0 and S[1, 2] == 0 and np.isneginf(S[:, 1]).all()
    assert S[0, 2] == 0
    assert S[0, 0] == np.float32(np.float32(1 / 127) * np.float32(2 * 127 * 127 * 128 / 127))


def test_clamp0_and_the_int32_extreme():
    q = [np.full((1, 128), 1.0, np.float32), np.full((1, 128), -1.0, np.float32)]
    p = [np.full((4, 128), 2.0, np.float32), np.full((4, 128), 2.0, np.float32)]
    S = it.score_blocks(q, p, clamp0=np.array([0, 1], np.uint8))
    M = it.maxima(np.array([[-127] * 128], np.int8), np.full((4, 128), 127, np.int8), [0, 4])
    assert M[0, 0] == -(127 ** 2) * 128 == -2064512
    assert S[1, 0] < 0 and S[1, 1] == 0 and S[0, 0] == S[0, 1] > 0


def test_score_is_the_sequential_sum_in_token_order():
    rng = np.random.default_rng(0)
    q = rng.standard_normal((37, 128)).astype(np.float32)
    p = rng.standard_normal((50, 128)).astype(np.float32)
    q8, sq = it.quantize_tokens(q)
    d8, sd = it.quantize_pages(p, [0, 50])
    M = (q8.astype(np.int64) @ d8.astype(np.int64).T).max(axis=1)
    T = np.float32(0)
    for i in range(37):
        T = np.float32(T + np.float32(np.float32(M[i]) * sq[i]))
    got = it.scores(q8, sq, [0, 37], d8, sd, [0, 50])
    assert got[0, 0] == np.float32(sd[0] * T)
    assert abs(got[0, 0] - (q @ p.T).max(axis=1).sum()) < 0.05 * abs((q @ p.T).max(axis=1).sum()) + 1


def test_fast_form_equals_the_plain_one():
    rng = np.random.default_rng(3)
    lens = [0, 1, 3, 0, 16, 17, 2, 0, 40, 5]
    off = np.cumsum([0] + lens)
    rows = rng.standard_normal((off[-1], 128)).astype(np.float32)
    rows[off[4]:off[5]] = 0
    d8, sd = it.quantize_pages(rows, off)
    q8, sq = it.quantize_tokens(rng.standard_normal((9, 128)).astype(np.float32))
    q_off = [0, 4, 4, 9]
    c0 = np.array([i % 3 == 0 for i in range(len(lens))], np.uint8)
    want = it.scores(q8, sq, q_off, d8, sd, off, c0)
    got = it.scores_fast(q8, sq, q_off, d8, sd, off, c0, token_block=4)
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
