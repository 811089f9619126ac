"""The contract of msim_digest / msim_digest_host (include/maxsim.h, "PERSISTENCE") restated in numpy uint64.

Not a test module: the persistence tests import `digest` from here and compare the library against it bit for bit."""
import numpy as np

C0 = np.uint64(0x9E3779B97F4A7C15)
C1 = np.uint64(0xC2B2AE3D27D4EB4F)
K = np.uint64(0xD6E8FEB86659FD93)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def mix(x: np.ndarray) -> np.ndarray:
    """the splitmix64 finaliser, element-wise on uint64 (numpy array arithmetic wraps mod 2^64)"""
    x = x ^ (x >> np.uint64(30))
    x = x * _M1
    x = x ^ (x >> np.uint64(27))
    x = x * _M2
    return x ^ (x >> np.uint64(31))


def digest(data: bytes, pos: int = 0, acc=(0, 0)):
    """(acc0, acc1) after adding the digest of `data`, a part that starts at byte `pos` (a multiple of 8) of some object."""
    assert pos % 8 == 0
    n = (len(data) + 7) // 8
    w = np.frombuffer(bytes(data) + b"\0" * (n * 8 - len(data)), dtype="<u8").astype(np.uint64)
    g1 = np.arange(n, dtype=np.uint64) + np.uint64(pos // 8 + 1)
    with np.errstate(over="ignore"):
        a0 = mix(w + g1 * C0).sum(dtype=np.uint64)
        a1 = mix((w ^ K) + g1 * C1).sum(dtype=np.uint64)
    return (int(a0) + acc[0]) % 2**64, (int(a1) + acc[1]) % 2**64
