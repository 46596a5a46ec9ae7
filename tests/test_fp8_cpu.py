"""FP8 (e4m3) weight-only format on the CPU: the plain-torch oracle
(ops/reference.py quant_rows_fp8 / dequant_rows_fp8), the lossless grid checkpoint of
tests/_fp8.py, and the --weight-dtype flag of both entry points."""
import os
import subprocess
import sys

import pytest
import torch

from _fp8 import half_spacing, projection_tensors, write_grid_checkpoint
from cake_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


def _codes_f32(codes):
    return codes.view(torch.float8_e4m3fn).float()


def test_quant_rows_half_spacing_bound():
    torch.manual_seed(0)
    w = (torch.randn(96, 2064) * 0.02).to(torch.bfloat16)
    codes, scale = R.quant_rows_fp8(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (96,)
    assert torch.equal(scale, w.float().abs().amax(dim=1) / 448.0)
    assert int(((codes & 0x7F) == 0x7F).sum()) == 0  # never the NaN code
    v = w.float() / scale[:, None]
    err = (v - _codes_f32(codes)).abs()
    assert bool((err <= half_spacing(v)).all()), float((err / half_spacing(v)).max())
    # every row holds a +-448 code: its amax maps onto the format's maximum
    assert bool((_codes_f32(codes).abs().amax(dim=1) == 448.0).all())


def test_quant_rows_zero_row_and_single_nonzero():
    w = torch.zeros(3, 32, dtype=torch.bfloat16)
    w[1, 7] = -0.37
    w[2] = (torch.arange(32) - 16).to(torch.bfloat16) * 0.01
    codes, scale = R.quant_rows_fp8(w)
    assert float(scale[0]) == 1.0 and int(codes[0].abs().sum()) == 0
    assert int(codes[1, 7]) == 0xFE and int((codes[1] != 0).sum()) == 1  # -448
    assert int(((codes & 0x7F) == 0x7F).sum()) == 0
    d = R.dequant_rows_fp8(codes, scale)
    assert d.dtype == torch.float32 and float(d[1, 7]) == float(w[1, 7])


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("fp8_grid"))


def test_grid_checkpoint_is_lossless(grid):
    scales = set()
    ts = projection_tensors(grid)
    assert len(ts) == 3 * 7
    for name, w in ts.items():
        assert w.dtype == torch.bfloat16
        codes, scale = R.quant_rows_fp8(w)
        assert int(((codes & 0x7F) == 0x7F).sum()) == 0, name
        assert torch.equal(R.dequant_rows_fp8(codes, scale).to(torch.bfloat16), w), name
        m, _ = torch.frexp(scale)
        assert bool((m == 0.5).all()), name  # powers of two
        scales |= set(scale.tolist())
    assert len(scales) >= 3
    std = torch.cat([w.float().reshape(-1) for w in ts.values()]).std()
    assert 0.01 < float(std) < 0.03  # near the 0.02 of the synthetic checkpoints


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def test_cake_cli_rejects_bogus_weight_dtype():
    r = _run([CLI, "--weight-dtype", "bogus"])
    assert r.returncode == 2 and "--weight-dtype" in r.stderr, r.stderr
    r = _run([CLI, "--help"])
    assert r.returncode == 0 and "--weight-dtype" in r.stdout


def test_python_cli_rejects_bogus_weight_dtype():
    r = _run([sys.executable, "-m", "cake_amd.cli", "--weight-dtype", "bogus"])
    assert r.returncode == 2 and "--weight-dtype" in r.stderr, r.stderr


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_fp8_refused_on_the_python_path(grid, tmp_path, entry):
    """CAKE_NATIVE=0 keeps the Python generator, which has no fp8 weights: it refuses
    with a message and never runs 16-bit instead."""
    head = [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]
    r = _run([*head, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--weight-dtype", "fp8", "--temperature", "0", "-n", "2", "--prompt", "hi"],
             CAKE_NATIVE="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--weight-dtype fp8" in r.stderr and "native Llama engine" in r.stderr
    assert r.stdout.strip() == ""  # nothing was generated
