"""FP8 MFMA prefill on the CPU: the float64 GEMM oracle against an explicit dequantise-and-
matmul, the exact-input generators' own conditions, the engine struct's new field and the
refusals of --prefill-dtype on every path that has no fp8 prefill."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _w8a8 as W
from _qhead import write_grid_head_checkpoint
from cake_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("epi", W.EPIS)
def test_ref_equals_explicit_dequantise_and_matmul(epi):
    c = W.random_case(17, 48, 384)
    a = R.dequant_rows_fp8(c["a8"], torch.ones(17)).double() * c["sa"].double()[:, None]
    w = R.dequant_rows_fp8(c["w8"], torch.ones(48)).double() * c["sw"].double()[:, None]
    y = a @ w.T
    if epi == "swiglu":
        g, u = y[:, :24], y[:, 24:]
        y = g * torch.sigmoid(g) * u
    got = R.gemm_w8a8_ref(c["a8"], c["sa"], c["w8"], c["sw"], epi)
    assert got.dtype == torch.float64 and got.shape == y.shape
    # the scales multiply the sum once here and every term there: equal to float64 rounding
    assert torch.allclose(got, y, rtol=1e-12, atol=0)


def test_ref_on_one_element():
    a8 = W.codes_of(torch.tensor([[1.5] + [0.0] * 127]))
    w8 = W.codes_of(torch.tensor([[-448.0] + [0.0] * 127, [2.0 ** -9] + [0.0] * 127]))
    y = R.gemm_w8a8_ref(a8, torch.tensor([0.5]), w8, torch.tensor([2.0, 4.0]))
    assert y.tolist() == [[-672.0, 1.5 * 2.0 ** -9 * 2.0]]
    with pytest.raises(ValueError):
        R.gemm_w8a8_ref(a8, torch.tensor([0.5]), w8, torch.tensor([2.0, 4.0]), "geglu")


def test_random_codes_cover_the_format():
    c = W.random_codes((64, 1152), torch.Generator().manual_seed(0))
    assert len(set(c.reshape(-1).tolist())) == 254
    assert not ((c & 0x7F) == 0x7F).any()
    assert float(W.values_of(c).abs().max()) == 448.0


# ---------------------------------------------------------------------------
# the exact generators
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(1, 16, 128), (257, 272, 1152), (129, 144, 384)])
def test_exact_case_products_and_partial_sums_are_exact(M, N, K):
    """Every product is an integer, the sum of the magnitudes stays below 2^24 grains (so any
    partial sum in any order does), and the f32 evaluation in a scrambled k order equals the
    float64 one."""
    c = W.exact_case(M, N, K)
    a, w = W.values_of(c["a8"]), W.values_of(c["w8"])
    assert float(a.abs().max()) <= 8 and float(w.abs().max()) <= 8
    prod_mag = a.abs() @ w.abs().T                      # sum_k |a||w|: bounds every partial sum
    assert float(prod_mag.max()) < 2 ** 24
    grain = W.check_exact(c["a8"], c["w8"], c["sa"], c["sw"], c["r32"])
    s = c["sa"].double()[:, None] * c["sw"].double()[None, :]
    assert float((prod_mag * s + c["r32"].abs().double()).max()) / grain < 2 ** 24
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(K))
    y32 = (a[:, perm].float() @ w[:, perm].float().T) * s.float()
    assert torch.equal(y32.double(), c["want"])
    assert torch.equal((c["r32"] + y32).double(), c["want_r"])


def test_exact_check_rejects_bad_inputs():
    c = W.exact_case(15, 16, 128)
    with pytest.raises(AssertionError, match="power of two"):
        W.check_exact(c["a8"], c["w8"], c["sa"] * 1.5, c["sw"])
    half = W.codes_of(torch.full((15, 128), 0.5))
    with pytest.raises(AssertionError, match="non-integer"):
        W.check_exact(half, c["w8"], c["sa"], c["sw"])
    with pytest.raises(AssertionError, match="24 bits"):
        W.check_exact(c["a8"], c["w8"], torch.cat([c["sa"][:-1], torch.tensor([2.0 ** -30])]),
                      c["sw"])
    with pytest.raises(AssertionError):
        W.codes_of(torch.tensor([17.0]))


def test_gated_case_is_exact_and_bounded():
    c = W.gated_case(129, 48, 1152)
    assert float(c["pre"].abs().max()) <= 16 and float((c["pre"] != 0).float().mean()) > 0.5
    assert c["want"].shape == (129, 48) and c["want"].dtype == torch.float64


def test_one_hot_case():
    c = W.one_hot_case()
    assert c["a8"].shape == c["w8"].shape == (256, 256)
    assert int((c["a8"] == W.E4M3_ONE).sum()) == 256 and int((c["a8"] != 0).sum()) == 256
    want = R.gemm_w8a8_ref(c["a8"], c["sa"], c["w8"], c["sw"])
    assert torch.equal(want, c["want"].double())
    assert not torch.equal(c["want"], c["want"].T)


# ---------------------------------------------------------------------------
# the option's surfaces
# ---------------------------------------------------------------------------

def test_native_llama_rejects_an_unknown_prefill_before_opening():
    from cake_amd.engine import NativeLlama
    with pytest.raises(ValueError, match="prefill"):
        NativeLlama("/nonexistent", prefill="int4")


def test_engine_opts_carry_prefill_fmt_in_the_weight_fmt_word():
    """The struct keeps its 40 bytes and every offset (its layout is pinned by the earlier
    formats' tests): prefill_fmt travels in bits 8 and up of weight_fmt, 0 for every caller
    that passes a plain weight format."""
    from cake_amd.engine import PREFILL_FMT_SHIFT, PREFILL_FORMATS, WEIGHT_FORMATS, EngineOpts
    assert C.sizeof(EngineOpts) == 40 and EngineOpts.kv_fmt.offset == 36
    assert EngineOpts.weight_fmt.offset == 20 and EngineOpts.weight_fmt.size == 4
    assert not hasattr(EngineOpts, "prefill_fmt")
    assert PREFILL_FORMATS == {"model": 0, "fp8": 1} and PREFILL_FMT_SHIFT == 8
    assert max(WEIGHT_FORMATS.values()) < 1 << PREFILL_FMT_SHIFT
    src = open(os.path.join(ROOT, "cake_amd", "csrc", "engine", "llama_engine.h")).read()
    assert "#define CAKE_PREFILL_FMT_SHIFT 8" in src


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return write_grid_head_checkpoint(tmp_path_factory.mktemp("w8a8_ckpt"), "fp8")


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_prefill_dtype_and_rejects_int4(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and "--prefill-dtype" in r.stdout
    assert "fp8" in r.stdout[r.stdout.index("--prefill-dtype"):][:600]
    r = _run([*_entry(entry), "--prefill-dtype", "int4"])
    assert r.returncode == 2 and "--prefill-dtype" in r.stderr, r.stderr


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("how", ["CAKE_NATIVE=0", "--cpu", "--no-graph", "f32"])
def test_prefill_dtype_refused_on_the_python_engines(ckpt, tmp_path, entry, how):
    """Every Python engine path refuses with the --weight-dtype wording and status 2, and
    never runs the 16-bit prefill instead."""
    extra, env = [], {}
    if how == "CAKE_NATIVE=0":
        env["CAKE_NATIVE"] = "0"
    elif how == "f32":
        extra = ["--dtype", "f32"]
    else:
        extra = [how]
    r = _run([*_entry(entry), "--model", str(ckpt), "--topology", str(tmp_path / "none.yml"),
              "--prefill-dtype", "fp8", "--temperature", "0", "-n", "2", "--prompt", "hi",
              *extra], **env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--prefill-dtype fp8" in r.stderr and "native Llama engine" in r.stderr
    assert "refusing rather than running 16-bit" in r.stderr
    assert r.stdout.strip() == ""  # nothing was generated


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_prefill_dtype_refused_for_image_models(ckpt, tmp_path, entry):
    r = _run([*_entry(entry), "--model", str(ckpt), "--topology", str(tmp_path / "none.yml"),
              "--model-type", "image-model", "--prefill-dtype", "fp8"])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--prefill-dtype fp8" in r.stderr and "text model only" in r.stderr
