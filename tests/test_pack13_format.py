"""The 13-bit code of the corpus image (csrc/pack13.hip), restated in numpy: it must round-trip every bf16 pattern it calls
representable and call exactly the patterns with an exponent field outside [96, 127] unrepresentable."""
import numpy as np


def representable(u):
    e = (u >> 7) & 0xFF
    return (e >= 96) & (e <= 127)


def encode(u):
    return u & 0xFF, (u >> 8) & 0xF, u >> 15


def decode(low, nibble, sign):
    return (((sign << 7) | 0x30 | nibble) << 8) | low


def test_every_bf16_pattern_round_trips_or_is_unrepresentable():
    u = np.arange(65536, dtype=np.uint32)
    low, nibble, sign = encode(u)
    assert low.max() == 0xFF and nibble.max() == 0xF and sign.max() == 1          # 8 + 4 + 1 = 13 bits
    back = decode(low, nibble, sign)
    ok = representable(u)
    assert np.array_equal(back[ok], u[ok])
    assert not np.any(back[~ok] == u[~ok])                    # and nothing else survives: the classification is exact
    assert int(ok.sum()) == 2 * 32 * 128                       # two signs x 32 exponents x 128 mantissas


def test_classification_in_values():
    u = np.arange(65536, dtype=np.uint32)
    with np.errstate(invalid="ignore"):
        x = (u << 16).astype(np.uint32).view(np.float32).astype(np.float64)
        in_range = np.isfinite(x) & (np.abs(x) >= 2.0 ** -31) & (np.abs(x) < 2.0)
    assert np.array_equal(representable(u), in_range)
    for bits in (0x0000, 0x8000, 0x0001, 0x2F80, 0x4000, 0x7F80, 0x7FC0):       # +0, -0, a denormal, 2^-32, 2.0, inf, NaN
        assert not representable(np.uint32(bits))
    for bits in (0x3000, 0x3F80, 0xBF80, 0x3FFF):                               # 2^-31, 1.0, -1.0, the largest value below 2
        assert representable(np.uint32(bits))
