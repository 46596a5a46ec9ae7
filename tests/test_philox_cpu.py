"""The numpy reference of the device sampler's draw (tests/_philox.py): Philox4x32-10
against the Random123 known-answer vectors, the uniform mapping's open interval, and the
counters of the default seed whose 24-bit variate is the largest one (the draws that
rounded to u = 1.0, G = +inf before the clamp in sampling.hip's gumbel())."""
import numpy as np
import pytest

from _philox import N_MAX, draw_n, gumbel_ref, philox4x32_10, uniform_from_n

# Random123 kat_vectors, philox4x32 10 rounds: (counter, key) -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]

DEFAULT_SEED_HITS = [(165, 15064), (255, 84910), (478, 18028), (599, 56489)]  # (step, index)


@pytest.mark.parametrize("ctr,key,out", KAT)
def test_known_answer_vectors(ctr, key, out):
    assert tuple(int(w) for w in philox4x32_10(*ctr, *key)) == out


def test_vectorised_equals_scalar():
    """Broadcast evaluation (index vector x scalar step / key) is the scalar function."""
    idx = np.array([0, 1, 128255, 2 ** 31 - 2, 0xFFFFFFFF])
    vec = philox4x32_10(idx, 7, 0, 0, 0x1234, 0x9)
    for j, i in enumerate(idx):
        one = philox4x32_10(int(i), 7, 0, 0, 0x1234, 0x9)
        assert [int(w[j]) for w in vec] == [int(w) for w in one]
    # the third KAT vector inside a batch
    c, k, out = KAT[2]
    got = philox4x32_10(np.array([0, c[0]]), np.array([0, c[1]]), np.array([0, c[2]]),
                        np.array([0, c[3]]), np.array([0, k[0]]), np.array([0, k[1]]))
    assert tuple(int(w[1]) for w in got) == out and int(got[0][0]) == 0x6627E8D5


def test_uniform_strictly_inside_unit_interval():
    n = np.array([0, 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 24 - 2, 2 ** 24 - 1])
    u = uniform_from_n(n)
    assert u.dtype == np.float32
    assert (u > 0).all() and (u < 1).all()
    assert (np.diff(u.astype(np.float64)) >= 0).all()
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.float32(1 - 2.0 ** -24)
    # the unclamped float32 expression is exactly 1.0 for the largest n: the bug's origin
    raw = np.float32(N_MAX) * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    assert raw == np.float32(1.0)
    g = -np.log(-np.log(u.astype(np.float64)))
    assert np.isfinite(g).all() and g[-1] < 16.7


def test_default_seed_hits_have_largest_n():
    from cake_amd.models.sampling import SamplingConfig
    seed = SamplingConfig().seed
    assert seed == 299792458
    for step, index in DEFAULT_SEED_HITS:
        assert int(draw_n(index, step, seed)) == N_MAX, (step, index)
        assert np.isfinite(gumbel_ref(index, step, seed))
    # and a whole step's scan finds the hit where it is, nowhere else
    n = draw_n(np.arange(128256), 165, seed)
    assert np.nonzero(n == N_MAX)[0].tolist() == [15064]
