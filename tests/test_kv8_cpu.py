"""FP8 (e4m3) KV cache on the CPU: the format oracle against an exhaustive float64 search,
the refusals of --kv-dtype on every path that has no fp8 cache, and the exact conversion of
the block-code attention caches of tests/_exact.py to codes."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

import _exact as X
import _kv8 as KV
from _qhead import write_grid_head_checkpoint
from cake_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------

def _probe_values() -> torch.Tensor:
    """Every finite code's value, every midpoint of two neighbouring codes (the ties), their
    f32 neighbours on both sides, values beyond +-448, tiny values and a Gaussian sample."""
    v = KV.code_values_f64()[:127]
    mids = (v[:-1] + v[1:]) / 2
    base = torch.cat([v, mids]).float()
    assert torch.equal(base.double(), torch.cat([v, mids]))  # all exact in f32
    inf = torch.full_like(base, float("inf"))
    pts = torch.cat([base, torch.nextafter(base, inf), torch.nextafter(base, -inf),
                     torch.tensor([448.0, 449.0, 464.0, 480.0, 1e4, 3e38, 2.0 ** -10, 2.0 ** -11,
                                   1e-30, 0.0]),
                     torch.randn(4096, generator=torch.Generator().manual_seed(0)) * 4])
    return torch.cat([pts, -pts])


def test_oracle_matches_float64_nearest_code_search():
    x = _probe_values()
    got = R.quant_kv_fp8(x)
    want = KV.nearest_code_f64(x)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, [(float(x[i]), int(got[i]), int(want[i])) for i in bad[:5, 0]]
    assert got.dtype == torch.uint8 and got.shape == x.shape


def test_oracle_ties_go_to_the_even_code():
    v = KV.code_values_f64()[:127]
    mids = ((v[:-1] + v[1:]) / 2).float()
    codes = R.quant_kv_fp8(mids)
    assert bool((codes % 2 == 0).all())
    lo = torch.arange(126)
    assert torch.equal(codes.long(), torch.where(lo % 2 == 0, lo, lo + 1))
    assert torch.equal(R.quant_kv_fp8(-mids).long(), codes.long() | 0x80)


def test_oracle_saturates_and_never_gives_the_nan_code():
    big = torch.tensor([448.0, 448.0001, 464.0, 500.0, 1e9, 3.4e38])
    assert R.quant_kv_fp8(big).tolist() == [0x7E] * 6
    assert R.quant_kv_fp8(-big).tolist() == [0xFE] * 6
    x = _probe_values()
    codes = R.quant_kv_fp8(x)
    assert not bool(((codes & 0x7F) == 0x7F).any())


def test_oracle_round_trips_every_finite_code():
    vals = R.dequant_kv_fp8(KV.FINITE_CODES)
    assert vals.dtype == torch.float32 and bool(torch.isfinite(vals).all())
    assert torch.equal(vals.double(), KV.code_values_f64()[KV.FINITE_CODES.long()])
    assert torch.equal(R.quant_kv_fp8(vals), KV.FINITE_CODES)
    nan = R.dequant_kv_fp8(torch.tensor(KV.NAN_CODES, dtype=torch.uint8))
    assert bool(torch.isnan(nan).all())


@pytest.mark.parametrize("dt", KV.DTYPES)
def test_every_e4m3_value_is_exact_in_16_bits(dt):
    vals = R.dequant_kv_fp8(KV.FINITE_CODES)
    assert torch.equal(vals.to(dt).float(), vals)


def test_near_boundary_and_code_steps_helpers():
    v = KV.code_values_f64()[:127]
    mids = ((v[:-1] + v[1:]) / 2).float()
    assert bool(KV.near_boundary(mids).all())
    assert not bool(KV.near_boundary(v[1:].float()).any())
    a = torch.tensor([0x00, 0x01, 0x81, 0x7E], dtype=torch.uint8)
    b = torch.tensor([0x80, 0x02, 0x01, 0x7D], dtype=torch.uint8)
    assert KV.code_steps(a, b).tolist() == [0, 1, 2, 1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_rope_reference_is_rarely_within_an_ulp_of_a_boundary(seed):
    """The share of f32 rope-reference elements that may legitimately land one code step off
    stays far under the 0.1 % the GPU test tolerates (same seeds, same shapes)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(130, 8, 128, generator=g).to(torch.bfloat16)
    k = torch.randn(130, 2, 128, generator=g).to(torch.bfloat16)
    inv = R.inv_freq(128, 500000.0)
    _, kr = KV.rope_reference_f32(q, k, inv, 33)
    share = float(KV.near_boundary(kr).float().mean())
    assert share < 1e-3 / 10, share


# ---------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------

def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    return write_grid_head_checkpoint(tmp_path_factory.mktemp("kv8_ckpt"), "fp8")


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_kv_dtype_and_rejects_int4(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and "--kv-dtype" in r.stdout
    assert "fp8" in r.stdout[r.stdout.index("--kv-dtype"):][:600]
    r = _run([*_entry(entry), "--kv-dtype", "int4"])
    assert r.returncode == 2 and "--kv-dtype" in r.stderr, r.stderr
    # the test-oracle format has no CLI value
    r = _run([*_entry(entry), "--kv-dtype", "fp8-emulated"])
    assert r.returncode == 2 and "--kv-dtype" in r.stderr, r.stderr


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
@pytest.mark.parametrize("how", ["CAKE_NATIVE=0", "--cpu", "--no-graph", "f32"])
def test_kv_dtype_refused_on_the_python_engines(ckpt, tmp_path, entry, how):
    """Every Python engine path refuses with the --weight-dtype wording and status 2, and
    never runs a 16-bit cache instead."""
    extra, env = [], {}
    if how == "CAKE_NATIVE=0":
        env["CAKE_NATIVE"] = "0"
    elif how == "f32":
        extra = ["--dtype", "f32"]
    else:
        extra = [how]
    r = _run([*_entry(entry), "--model", str(ckpt), "--topology", str(tmp_path / "none.yml"),
              "--kv-dtype", "fp8", "--temperature", "0", "-n", "2", "--prompt", "hi", *extra],
             **env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--kv-dtype fp8" in r.stderr and "native Llama engine" in r.stderr
    assert "KV cache" in r.stderr
    assert r.stdout.strip() == ""  # nothing was generated


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_kv_dtype_refused_for_image_models(ckpt, tmp_path, entry):
    r = _run([*_entry(entry), "--model", str(ckpt), "--topology", str(tmp_path / "none.yml"),
              "--model-type", "image-model", "--kv-dtype", "fp8"])
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--kv-dtype fp8" in r.stderr and "text model only" in r.stderr


def test_native_llama_rejects_an_unknown_kv_before_opening():
    from cake_amd.engine import NativeLlama
    with pytest.raises(ValueError, match="kv"):
        NativeLlama("/nonexistent", kv="int4")


def test_engine_opts_layout_with_kv_fmt():
    """kv_fmt is the trailing field: at 36, inside the former tail padding (40 bytes)."""
    from cake_amd.engine import KV_FORMATS, EngineOpts
    assert C.sizeof(EngineOpts) == 40
    assert EngineOpts.kv_fmt.offset == 36 and EngineOpts.kv_fmt.size == 4
    assert EngineOpts.head_fmt.offset == 32
    o = EngineOpts(256, 0, 0, 1, 0, 2, 7, 1)  # callers that stop at head_fmt: kv_fmt 0
    assert o.kv_fmt == 0 and o.head_fmt == 1
    assert KV_FORMATS == {"model": 0, "fp8": 1, "fp8-emulated": 2}


# ---------------------------------------------------------------------------
# block-code caches as codes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dt", KV.DTYPES)
@pytest.mark.parametrize("phase", [0, 8])
@pytest.mark.parametrize("Tk", [1, 17, 321])
def test_block_code_cache_converts_exactly(dt, phase, Tk):
    bc = X.decode_case(2, 64, Tk, 512, phase, dt)
    k8, v8 = KV.block_code_codes(bc)
    assert k8.dtype == torch.uint8 and tuple(k8.shape) == (2, 512, 64) == tuple(v8.shape)
    assert set(k8.unique().tolist()) <= {0x38, 0xB8}            # +-1
    assert set(v8[:, :Tk].unique().tolist()) <= {0x00, 0x38}     # one-hot
    assert bool((v8[:, Tk:] == 0x7F).all())
    assert int((v8[:, :Tk] == 0x38).sum()) == 2 * Tk
