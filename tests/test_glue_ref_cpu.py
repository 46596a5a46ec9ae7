"""CPU checks of tests/_glue.py: the hash and Philox words against known answers, the
extreme draws the GPU tests rely on, the moments of both normal references, and the
timestep-embedding / scheduler-step references against independent formulations."""
import math

import numpy as np
import pytest
import torch

import _glue as G
from _philox import N_MAX, draw_n

N_STAT = 1 << 20


def test_mix64_is_the_splitmix64_finaliser():
    """splitmix64 seeded with 0 adds the golden ratio, then finalises: its first outputs
    (Vigna's reference values)."""
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    state = np.arange(1, 4, dtype=np.uint64) * np.uint64(G.GOLDEN)
    assert [int(v) for v in G.mix64(state)] == want
    assert int(G.mix64(np.uint64(G.GOLDEN))) == 0xE220A8397B1DCDAF
    assert int(G.fill_hash(0, 0)) == int(G.mix64(G.mix64(np.uint64(G.GOLDEN))))
    assert int(G.fill_hash(5, 7)) == int(G.mix64(np.uint64(5) ^ G.mix64(np.uint64(7 + G.GOLDEN))))


def test_uniform_edges():
    u1, u2 = G.sd_uniforms(np.array([0, 1, 2 ** 23, 2 ** 23 + 1, N_MAX - 1, N_MAX]),
                           np.array([0, 1, 2 ** 23, 2 ** 23 + 1, N_MAX - 1, N_MAX]))
    # above 2^23 the + 0.5f is a tie: to even
    assert u1.tolist() == [2.0 ** -25, 1.5 * 2.0 ** -24, 0.5, 0.5 + 2.0 ** -23,
                           1.0 - 2.0 ** -23, 1.0]
    assert u2.tolist() == [0.0, 2.0 ** -24, 0.5, 0.5 + 2.0 ** -24, 1 - 2.0 ** -23, 1 - 2.0 ** -24]
    assert u1.dtype == u2.dtype == np.float32
    r = np.array([0, (1 << 40) - 1, 1 << 40, (1 << 64) - 1], dtype=np.uint64)
    f1, f2 = G.fill_uniforms(r)
    assert f1.tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1.0]
    assert f2.tolist() == [0.0, 1 - 2.0 ** -24, 0.0, 1 - 2.0 ** -24]


def test_sd_words_are_philox_words_0_and_1():
    i = np.arange(64)
    n1, n2 = G.sd_words(i, 3, (7 << 32) | 5)
    assert np.array_equal(n1, draw_n(i, 3, (7 << 32) | 5))          # the sampler's word 0
    assert not np.array_equal(n1, n2)
    # counter (index, step): swapping the two words of the counter is another stream
    assert not np.array_equal(n1, G.sd_words(3, i, (7 << 32) | 5)[0])
    # the high word of the seed is key word 1
    assert not np.array_equal(n1, G.sd_words(i, 3, 5)[0])


def test_pinned_extremes():
    for (seed, step, index, n), z in zip(G.SD_EXTREMES, G.SD_EXTREME_Z):
        assert int(G.sd_words(index, step, seed)[0]) == n
        got = float(G.sd_normal_ref(index, step, seed))
        assert got == pytest.approx(z, abs=1e-5) and (n != N_MAX or got == 0.0)
        assert index < 1 << 16
    for (key, pair, hi), (ze, zo) in zip(G.FILL_EXTREMES, G.FILL_EXTREME_Z):
        assert int(G.fill_hash(key, pair) >> np.uint64(40)) == hi
        e, o = G.fill_normal_ref(key, np.array([2 * pair, 2 * pair + 1]))
        assert e == pytest.approx(ze, abs=1e-5) and o == pytest.approx(zo, abs=1e-5)
        if hi == N_MAX:
            assert e == 0.0 and o == 0.0
    # the radius at the smallest u1: sqrt(2 * 25 ln 2) (scheduler), sqrt(2 * 24 ln 2) (fill)
    n2 = int(G.sd_words(40858, 51, 12345)[1])
    ang = float(np.float32(6.283185307179586) * np.float32(n2 * 2.0 ** -24))
    assert G.SD_EXTREME_Z[0] == pytest.approx(math.sqrt(50 * math.log(2)) * math.cos(ang), abs=1e-5)
    assert math.hypot(*G.FILL_EXTREME_Z[0]) == pytest.approx(math.sqrt(48 * math.log(2)), abs=1e-5)


@pytest.mark.parametrize("which", ["sd", "fill", "fill odd key"])
def test_reference_moments(which):
    """Mean, std and P(z > 1.96) over 2^20 indices within five standard errors."""
    i = np.arange(N_STAT)
    z = {"sd": lambda: G.sd_normal_ref(i, 0, 12345), "fill": lambda: G.fill_normal_ref(1, i),
         "fill odd key": lambda: G.fill_normal_ref(G.GOLDEN, i)}[which]()
    n = float(N_STAT)
    p = 0.5 * math.erfc(1.96 / math.sqrt(2))                  # 0.0249979
    assert abs(p - 0.025) < 1e-5
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.std() - 1) <= 5 / math.sqrt(2 * n)
    assert abs((z > 1.96).mean() - 0.025) <= 5 * math.sqrt(0.025 * 0.975 / n)
    # even / odd elements of a pair are the two Box-Muller outputs: uncorrelated
    assert abs((z[0::2] * z[1::2]).mean()) <= 5 / math.sqrt(n / 2)


def test_f32_forms_follow_the_references():
    i = np.arange(4096)
    assert np.abs(G.sd_normal_f32(i, 2, 9) - G.sd_normal_ref(i, 2, 9)).max() < 2e-6
    assert np.abs(G.fill_normal_f32(3, i) - G.fill_normal_ref(3, i)).max() < 2e-6
    e, o = G.fill_normal_ref(3, np.array([10, 11]))
    u1, u2 = G.fill_uniforms(G.fill_hash(3, np.array([5])))
    assert e * e + o * o == pytest.approx(-2 * math.log(float(u1[0])), rel=1e-12)


def test_timestep_embed_ref():
    for dim in G.TE_DIMS:
        half = dim // 2
        for flip in (False, True):
            for shift in (0.0, 1.0):
                ref, A = G.timestep_embed_ref(761.0, 3, dim, flip, shift)
                k = np.arange(half, dtype=np.float64)
                ang = 761.0 * 10000.0 ** (-k / (half - shift))
                s, c = np.sin(ang), np.cos(ang)
                want = np.concatenate([c, s] if flip else [s, c])
                assert ref.shape == (3, dim) and torch.equal(ref[0], ref[2])
                np.testing.assert_allclose(ref[1].numpy(), want, rtol=0, atol=1e-11)
                np.testing.assert_allclose(A[0, :half].numpy(), ang, rtol=1e-12)
                assert torch.equal(A[:, :half], A[:, half:])
        z, A = G.timestep_embed_ref(0.0, 1, dim, False, 1.0)
        assert (z[0, :half] == 0).all() and (z[0, half:] == 1).all() and (A == 0).all()
    assert G.TE_TABLE == [999.0, 761.0, 500.5, 21.0, 1.0, 0.0]


@pytest.mark.parametrize("cfg", [False, True])
def test_sched_step_ref(cfg):
    n = 257
    x, pred, coef = G.sched_inputs(n, cfg, torch.bfloat16, 3)
    for step in range(coef.shape[0]):
        a, b, nz, _ = coef[step].double().tolist()
        ref, A = G.sched_step_ref(x, pred, cfg, 7.5, coef, step, 12345)
        u = pred[:n].double()
        e = u + 7.5 * (pred[n:].double() - u) if cfg else u
        z = torch.from_numpy(G.sd_normal_ref(np.arange(n), step, 12345))
        want = a * x.double() + b * e + (nz * z if nz else 0)
        torch.testing.assert_close(ref, want, rtol=1e-13, atol=1e-13)
        assert (A >= ref.abs() - 1e-12).all() and (A >= (nz * z).abs() - 1e-12).all()
    # coef (0, 0, 1, 1): the noise alone
    one = torch.tensor([[0.0, 0.0, 1.0, 1.0]] * 4)
    ref, A = G.sched_step_ref(x, pred, cfg, 7.5, one, 3, (7 << 32) | 5)
    assert np.array_equal(ref.numpy(), G.sd_normal_ref(np.arange(n), 3, (7 << 32) | 5))
    assert torch.equal(A, ref.abs())
