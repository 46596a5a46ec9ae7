"""Host reference of the device sampler's random draw (sampling.hip): Philox4x32-10 and
the Gumbel variate built from it, in numpy.  Shared by test_philox_cpu (known-answer
vectors) and test_sampling_ref_gpu (device draws compared value by value)."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_M0 = np.uint64(0xD2511F53)
_M1 = np.uint64(0xCD9E8D57)
_W0 = np.uint64(0x9E3779B9)
_W1 = np.uint64(0xBB67AE85)
_S32 = np.uint64(32)

N_MAX = (1 << 24) - 1  # largest 24-bit variate n = word0 >> 8


def _u64(x):
    return np.asarray(x).astype(np.uint64) & M32


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., Random123): counter (c0..c3), key (k0, k1) -> the four
    output words.  Vectorised over broadcastable inputs; uint64 arithmetic masked to 32 bits."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(x) for x in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0 = _M0 * c0  # 32 x 32 -> 64 bit, no overflow in uint64
        p1 = _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32)
        k0 = (k0 + _W0) & M32
        k1 = (k1 + _W1) & M32
    return c0, c1, c2, c3


def draw_n(index, step, seed):
    """The sampler's 24-bit variate: word 0 of Philox(counter (index, step, 0, 0), key
    (seed low word, seed high word)), shifted right by 8."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w0 = philox4x32_10(index, step, 0, 0, seed & 0xFFFFFFFF, seed >> 32)[0]
    return (w0 >> np.uint64(8)).astype(np.int64)


def uniform_from_n(n):
    """u in (0, 1) from n in [0, 2^24), in float32 exactly as the kernel forms it:
    n * 2^-24 + 2^-25 (n * 2^-24 is exact, so a fused multiply-add rounds the same), then
    clamped to the largest float32 below 1 — n = 2^24 - 1 would otherwise round to 1.0."""
    n = np.asarray(n)
    u = n.astype(np.float32) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    return np.minimum(u, np.float32(1.0 - 2.0 ** -24)).astype(np.float32)


def gumbel_ref(index, step, seed):
    """G = -log(-log(u)) in float64 for the device's draw at (index, step, seed)."""
    u = uniform_from_n(draw_n(index, step, seed)).astype(np.float64)
    return -np.log(-np.log(u))
