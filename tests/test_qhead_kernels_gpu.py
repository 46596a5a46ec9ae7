"""Quantised lm_head kernels (gemv_norm_f32_kernel of gemv_kernel.h over the W8 / W4 weight
formats; entry points gemv_w8_head.hip, gemv_w4_head.hip): the RMSNorm-prologue, f32-output
GEMV over fp8 / MXFP4 rows and its fused greedy tail, against f32 torch math on
the dequantised weights (ops/reference.py) and against the unfused launch chain."""
import math

import pytest
import torch

from _qhead import FORMATS, dequant, quant
from cake_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16]
# the smallest K reaching each path: prefetch fallback, one chunk per lane, past one
# permutation block (1024 floats for w8, 2048 values for w4), prefetch 4 exactly full, NX 8
KS = {"fp8": [64, 1024, 1040, 4096, 8192], "mxfp4": [64, 2048, 2080, 4096, 8192]}
NS = [1, 9, 2050]  # one row, an odd last pair, idle and clamped waves
NMAX = max(NS)
EPS = 1e-5


def _gemv_tol(K):
    """The f32-output GEMV tolerance of tests/test_fp8_kernels_gpu.py::_gemv_case."""
    return dict(atol=2e-3 * math.sqrt(K / 256), rtol=1e-3)


_cache = {}


def _problem(fmt, dt, K, cuda):
    """One drawn problem per (format, dtype, K), NMAX rows, shared and left unchanged: rows are
    independent in both formats, so the cases with fewer rows take the first N.  Weights
    N(0, 0.02^2) quantised by the oracle; the reference is f32 torch math on the dequantised
    weights."""
    key = (fmt, dt, K)
    if key not in _cache:
        g = torch.Generator().manual_seed(1000 * K + 7 * len(fmt) + (dt == torch.float16))
        w16 = (torch.randn(NMAX, K, generator=g) * 0.02).to(dt)
        codes, scales = quant(fmt, w16)
        resid = torch.randn(K, generator=g) * 3
        nw = (1 + 0.1 * torch.randn(K, generator=g)).to(dt)
        wd = dequant(fmt, codes, scales).to(cuda)
        resid, nw = resid.to(cuda), nw.to(cuda)
        ref = wd @ R.rms_norm(resid, nw, EPS)
        _cache[key] = dict(codes=codes.to(cuda), scales=scales.to(cuda), resid=resid, nw=nw,
                           ref=ref)
    return _cache[key]


def _gemv(K_, fmt):
    return K_.norm_gemv_f32_w8 if fmt == "fp8" else K_.norm_gemv_f32_w4


def _select(K_, fmt):
    return K_.head_select_w8 if fmt == "fp8" else K_.head_select_w4


def _logits_case(K_, fmt, dt, K, N, cuda):
    p = _problem(fmt, dt, K, cuda)
    codes, scales = p["codes"][:N].contiguous(), p["scales"][:N].contiguous()
    guard = torch.full((N + 8,), 7.0, device=cuda)  # rows past N stay untouched
    out = guard[:N]
    _gemv(K_, fmt)(p["resid"], p["nw"], EPS, codes, scales, out)
    diff = float((out - p["ref"][:N]).abs().max())
    print(f"{fmt} {dt} K={K} N={N}: max |diff| {diff:.3e}, atol {_gemv_tol(K)['atol']:.3e}")
    torch.testing.assert_close(out, p["ref"][:N], **_gemv_tol(K))
    assert bool((guard[N:] == 7.0).all())


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS["fp8"])
def test_norm_gemv_f32_w8(cuda, dt, K, N):
    from cake_amd.ops import hip as K_
    _logits_case(K_, "fp8", dt, K, N, cuda)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS["mxfp4"])
def test_norm_gemv_f32_w4(cuda, dt, K, N):
    from cake_amd.ops import hip as K_
    _logits_case(K_, "mxfp4", dt, K, N, cuda)


@pytest.fixture
def head_tuning(cuda):
    from cake_amd.ops import hip as K_
    prev = (K_.get_gemv_w8_tuning("head"), K_.get_gemv_w4_tuning("head"))
    yield K_
    K_.set_gemv_w8_tuning("head", U=prev[0][0], prefetch=prev[0][1], max_blocks=prev[0][2])
    K_.set_gemv_w4_tuning("head", U=prev[1][0], prefetch=prev[1][1], max_blocks=prev[1][2])


def test_head_tuning_defaults(cuda):
    from cake_amd.ops import hip as K_
    assert K_.get_gemv_w8_tuning("head") == (2, 4, 1024)
    assert K_.get_gemv_w4_tuning("head") == (2, 4, 1024)


@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_cap_of_3_loops_over_pairs(head_tuning, cuda, fmt):
    """max_blocks 3: 12 waves walk the 1025 pairs, so every wave's loop runs past its
    prefetched first pair."""
    K_ = head_tuning
    setter = K_.set_gemv_w8_tuning if fmt == "fp8" else K_.set_gemv_w4_tuning
    getter = K_.get_gemv_w8_tuning if fmt == "fp8" else K_.get_gemv_w4_tuning
    U, pf, _ = getter("head")
    setter("head", U=U, prefetch=pf, max_blocks=3)
    assert getter("head") == (U, pf, 3)
    for K in (KS[fmt][2], 4096):
        _logits_case(K_, fmt, torch.bfloat16, K, NMAX, cuda)
    _fused_case(K_, fmt, torch.bfloat16, 4096, NMAX - 1, 64, 1.3, cuda)


def _state(N, hist0, resid0, cuda):
    hist = torch.zeros(400, dtype=torch.int32, device=cuda)
    hist[:300] = hist0.to(cuda)
    return dict(hist=hist, hist_len=torch.tensor([300], dtype=torch.int32, device=cuda),
                tok=torch.zeros(1, dtype=torch.int32, device=cuda),
                pos=torch.tensor([299], dtype=torch.int32, device=cuda),
                slot=torch.zeros(1, dtype=torch.int64, device=cuda),
                ticket=torch.zeros(1, dtype=torch.int32, device=cuda),
                logits=torch.empty(N, device=cuda), resid=resid0.clone())


def _fused_case(K_, fmt, dt, K, N, last_n, penalty, cuda):
    """The quantised twin of test_kernels_gpu.py::test_head_select_matches_four_launches:
    three steps in a row, the embedding row (16-bit table) given for the first two."""
    p = _problem(fmt, dt, K, cuda)
    codes, scales = p["codes"][:N].contiguous(), p["scales"][:N].contiguous()
    nw = p["nw"]
    g = torch.Generator().manual_seed(11 + N + last_n)
    table = (torch.randn(N, K, generator=g) * 2.0).to(dt).to(cuda)
    hist0 = torch.randint(0, N, (300,), generator=g, dtype=torch.int32)
    hist0[:20] = hist0[0]  # repeated tokens: penalised once
    a, b = _state(N, hist0, p["resid"], cuda), _state(N, hist0, p["resid"], cuda)
    ref = p["ref"][:N].clone()
    for step in range(3):
        _select(K_, fmt)(a["resid"], nw, EPS, codes, scales, a["logits"], a["hist"],
                         a["hist_len"], last_n, penalty, a["slot"], a["ticket"], a["tok"],
                         a["pos"], embed=table if step < 2 else None)
        _gemv(K_, fmt)(b["resid"], nw, EPS, codes, scales, b["logits"])
        if penalty != 1.0:
            K_.repeat_penalty(b["logits"], b["hist"], b["hist_len"], last_n, penalty)
        K_.argmax(b["logits"], b["slot"])
        K_.finalize_token(b["slot"], b["tok"], b["hist"], b["hist_len"], b["pos"])
        if step < 2:
            K_.embed(table, b["tok"], b["resid"])
        torch.cuda.synchronize()
        torch.testing.assert_close(a["logits"], b["logits"])
        for k in ("tok", "pos", "hist_len", "hist", "resid"):
            assert torch.equal(a[k], b[k]), (step, k)
        assert int(a["slot"]) == 0 and int(a["ticket"]) == 0
        assert int(a["hist_len"]) == 301 + step and int(a["pos"]) == 300 + step
        if step == 0:  # the first choice against f32 torch math
            if penalty != 1.0 and last_n:
                ref = R.apply_repeat_penalty(ref, penalty, hist0[300 - last_n:].tolist())
            tol = _gemv_tol(K)
            gap = float(ref.max()) - float(ref[int(a["tok"])])
            print(f"{fmt} first choice {int(a['tok'])}: reference gap to its maximum {gap:.3e}")
            assert 0 <= gap <= tol["atol"] + tol["rtol"] * abs(float(ref.max()))
    # without embed the input row is left alone
    assert torch.equal(a["resid"], b["resid"])


# penalty x last_n in full, N alternating odd / even
FUSED = [(2049, 0, 1.0), (2050, 64, 1.3), (2049, 256, 1.3), (2050, 256, 1.0), (2049, 64, 1.0),
         (2050, 0, 1.3)]


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("N,last_n,penalty", FUSED)
@pytest.mark.parametrize("fmt", FORMATS)
def test_head_select_q_matches_four_launches(cuda, fmt, dt, N, last_n, penalty):
    from cake_amd.ops import hip as K_
    _fused_case(K_, fmt, dt, KS[fmt][1], N, last_n, penalty, cuda)


@pytest.mark.parametrize("fmt", FORMATS)
def test_ties_go_to_the_smallest_index(cuda, fmt):
    """The maximal row duplicated (same codes, same scales) at i < j in different pairs and
    different workgroups: the token is i."""
    from cake_amd.ops import hip as K_
    dt, K, N = torch.bfloat16, KS[fmt][1], NMAX
    p = _problem(fmt, dt, K, cuda)
    codes, scales = p["codes"].clone(), p["scales"].clone()
    m = int(p["ref"].argmax())
    i, j = 5, 1500  # pairs 2 and 750: workgroups 0 and 187 of 257
    for r in (i, j):
        codes[r], scales[r] = p["codes"][m], p["scales"][m]
    if m not in (i, j):
        codes[m] = 0  # every code 0 is the value +0: logit 0, below the (positive) maximum
    assert float(p["ref"][m]) > 0
    s = _state(N, torch.zeros(300, dtype=torch.int32), p["resid"], cuda)
    _select(K_, fmt)(s["resid"], p["nw"], EPS, codes, scales, s["logits"], s["hist"],
                     s["hist_len"], 0, 1.0, s["slot"], s["ticket"], s["tok"], s["pos"])
    torch.cuda.synchronize()
    assert float(s["logits"][i]) == float(s["logits"][j]) == float(s["logits"].max())
    assert int((s["logits"] == s["logits"].max()).sum()) == 2
    assert int(s["tok"]) == i


def _fp8_codes(vals):
    return torch.tensor(vals, dtype=torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


@pytest.mark.parametrize("dt", DTYPES)
def test_w8_scaled_logits_decide(cuda, dt):
    """Rows A, B: the same codes (sign(x), sum S > 0) with scales 1 and 4; C: codes 8 sign(x)
    with scale 0.25, so its unscaled sum 8 S is the largest and its logit 2 S is not; D: A's
    codes with scale -1.  Every factor is a power of two, so the expected logits are exact.
    Without a window the token is B (4 S).  With B and D in the window and penalty 4 the
    penalty divides B's scaled 4 S to S and multiplies D's scaled -S to -4 S (a penalty on
    the unscaled sums would take the other branch for D), and the token is C.  Mirrors
    test_fp8_kernels_gpu.py::test_gemv_w8_scale_is_applied_per_row."""
    from cake_amd.ops import hip as K_
    K, N = 64, 4
    g = torch.Generator().manual_seed(31)
    resid = (torch.randn(K, generator=g) * 3).to(cuda)
    nw = (1 + 0.1 * torch.randn(K, generator=g)).to(dt).to(cuda)
    sgn = torch.sign(R.rms_norm(resid, nw, EPS)).cpu()
    assert bool((sgn != 0).all())
    one, eight = _fp8_codes(sgn.tolist()), _fp8_codes((8 * sgn).tolist())
    codes = torch.stack([one, one, eight, one]).to(cuda)
    scale = torch.tensor([1.0, 4.0, 0.25, -1.0], device=cuda)
    plain = torch.empty(N, device=cuda)
    K_.norm_gemv_f32_w8(resid, nw, EPS, codes, scale, plain)
    S = float(plain[0])
    assert S > 0 and plain.tolist() == [S, 4 * S, 2 * S, -S]
    for window, want_tok, want in (([], 1, [S, 4 * S, 2 * S, -S]),
                                   ([1, 3, 3], 2, [S, S, 2 * S, -4 * S])):
        hist = torch.zeros(16, dtype=torch.int32, device=cuda)
        hist[:len(window)] = torch.tensor(window, dtype=torch.int32)
        s = dict(hist=hist, hist_len=torch.tensor([len(window)], dtype=torch.int32, device=cuda),
                 tok=torch.full((1,), -1, dtype=torch.int32, device=cuda),
                 pos=torch.zeros(1, dtype=torch.int32, device=cuda),
                 slot=torch.zeros(1, dtype=torch.int64, device=cuda),
                 ticket=torch.zeros(1, dtype=torch.int32, device=cuda),
                 logits=torch.empty(N, device=cuda))
        K_.head_select_w8(resid, nw, EPS, codes, scale, s["logits"], s["hist"], s["hist_len"], 8,
                          4.0, s["slot"], s["ticket"], s["tok"], s["pos"])
        torch.cuda.synchronize()
        assert s["logits"].tolist() == want
        assert int(s["tok"]) == want_tok
        assert int(s["hist"][len(window)]) == want_tok and int(s["hist_len"]) == len(window) + 1


def test_refusals(cuda):
    """K % 16 (w8), K % 32 (w4), last_n = 257, penalty = 0, a tuning kind out of range: an
    error and nothing written."""
    from cake_amd.ops import hip as K_
    from cake_amd.ops._lib import KernelError, kernels
    dt, N = torch.bfloat16, 8
    for fmt, K in (("fp8", 24), ("mxfp4", 48)):
        resid = torch.randn(K, device=cuda)
        nw = torch.ones(K, dtype=dt, device=cuda)
        codes = torch.zeros((N, K if fmt == "fp8" else K // 2), dtype=torch.uint8, device=cuda)
        scales = (torch.ones(N, device=cuda) if fmt == "fp8"
                  else torch.full((N, K // 32), 127, dtype=torch.uint8, device=cuda))
        out = torch.full((N,), 3.0, device=cuda)
        with pytest.raises(KernelError):
            _gemv(K_, fmt)(resid, nw, 1e-5, codes, scales, out)
        s = _state(N, torch.zeros(300, dtype=torch.int32), resid, cuda)
        with pytest.raises(KernelError):
            _select(K_, fmt)(resid, nw, 1e-5, codes, scales, out, s["hist"], s["hist_len"], 0, 1.0,
                             s["slot"], s["ticket"], s["tok"], s["pos"])
        torch.cuda.synchronize()
        assert bool((out == 3.0).all())
    for fmt, K in (("fp8", 64), ("mxfp4", 64)):
        resid = torch.randn(K, device=cuda)
        nw = torch.ones(K, dtype=dt, device=cuda)
        codes = torch.zeros((N, K if fmt == "fp8" else K // 2), dtype=torch.uint8, device=cuda)
        scales = (torch.ones(N, device=cuda) if fmt == "fp8"
                  else torch.full((N, K // 32), 127, dtype=torch.uint8, device=cuda))
        out = torch.full((N,), 3.0, device=cuda)
        s = _state(N, torch.zeros(300, dtype=torch.int32), resid, cuda)
        args = (s["slot"], s["ticket"], s["tok"], s["pos"])
        with pytest.raises(ValueError):
            _select(K_, fmt)(resid, nw, 1e-5, codes, scales, out, s["hist"], s["hist_len"], 257,
                             1.1, *args)
        with pytest.raises(KernelError):
            _select(K_, fmt)(resid, nw, 1e-5, codes, scales, out, s["hist"], s["hist_len"], 8,
                             0.0, *args)
        torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and int(s["tok"]) == 0 and int(s["hist_len"]) == 300
    L = kernels()
    import ctypes as C
    out3 = (C.c_int * 3)()
    for name in ("w8", "w4"):
        assert getattr(L, f"cake_gemv_{name}_set_tuning")(4, 2, 4, 1024) != 0
        assert getattr(L, f"cake_gemv_{name}_set_tuning")(-1, 2, 4, 1024) != 0
        assert getattr(L, f"cake_gemv_{name}_get_tuning")(4, out3) != 0
        assert getattr(L, f"cake_gemv_{name}_get_tuning")(3, out3) == 0
    with pytest.raises(KeyError):
        K_.set_gemv_w8_tuning("tail", U=2, prefetch=4)
