"""MXFP4 weight-only format on the CPU: the plain-torch oracle (ops/reference.py
quant_rows_mxfp4 / dequant_rows_mxfp4), the lossless grid checkpoint of tests/_mxfp4.py, and
the --weight-dtype flag of both entry points."""
import os
import subprocess
import sys

import pytest
import torch

from _mxfp4 import (grid_matrix, grid_spacing_half, projection_tensors,
                    write_grid_checkpoint)
from cake_amd.ops import reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


def _nibbles(codes):
    c = codes.to(torch.int64)
    return torch.stack((c & 15, c >> 4), dim=2).reshape(codes.shape[0], -1)


def test_tie_rule_saturation_and_sign():
    """Block exponent 0 (amax 4): the seven midpoints go to the even code, on both signs."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0, 2, 2, 4, 4, 6, 6]  # values 0, 1, 1, 2, 2, 4, 4
    w = torch.zeros(2, 32, dtype=torch.bfloat16)
    w[0, :7] = torch.tensor(ties)
    w[0, 7] = 4.0
    w[1, 8:15] = -torch.tensor(ties)
    w[1, 20] = -4.0
    codes, e8 = R.quant_rows_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == (2, 16)
    assert e8.dtype == torch.uint8 and e8.shape == (2, 1) and e8.tolist() == [[127], [127]]
    n = _nibbles(codes)
    assert n[0, :8].tolist() == want + [6]
    assert n[1, 8:15].tolist() == [c | 8 for c in want]  # -0.25 -> -0, code 8
    assert int(n[1, 20]) == 14
    d = R.dequant_rows_mxfp4(codes, e8)
    assert d.dtype == torch.float32
    assert d[0, :8].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]
    # 7 under the scale 2^0 saturates to 6 (code 7); 6 < 7 < 8 keeps e = 0
    w = torch.zeros(1, 32, dtype=torch.bfloat16)
    w[0, 3], w[0, 4] = 7.0, -7.0
    codes, e8 = R.quant_rows_mxfp4(w)
    assert int(e8[0, 0]) == 127
    assert _nibbles(codes)[0, 3:5].tolist() == [7, 15]


def test_zero_block_and_scale_range():
    w = torch.zeros(3, 64, dtype=torch.bfloat16)
    w[1, 40] = -0.37  # one non-zero: its block gets e = floor(log2 .37) - 2 = -4
    w[2, :32] = 3.0e38  # near the bf16 maximum
    w[2, 32:] = 1e-40  # a subnormal block: the exponent clamps at -126
    codes, e8 = R.quant_rows_mxfp4(w)
    assert e8[0].tolist() == [127, 127] and int(codes[0].sum()) == 0
    assert e8[1].tolist() == [127, 123]
    assert int((codes[1] != 0).sum()) == 1 and int(_nibbles(codes)[1, 40]) == 8 | 7  # -5.92 -> -6
    assert e8[2].tolist() == [127 + 125, 1]
    assert int((e8 == 0xFF).sum()) == 0 and int((e8 == 0).sum()) == 0
    with pytest.raises(ValueError):
        R.quant_rows_mxfp4(torch.zeros(2, 48, dtype=torch.bfloat16))


def test_rounding_error_is_within_half_a_grid_step():
    torch.manual_seed(0)
    w = (torch.randn(96, 2080) * 0.02).to(torch.bfloat16)
    codes, e8 = R.quant_rows_mxfp4(w)
    assert codes.shape == (96, 1040) and e8.shape == (96, 65)
    assert int((e8 == 0xFF).sum()) == 0
    scale = torch.exp2(e8.float() - 127).repeat_interleave(32, dim=1)
    v = w.float() / scale
    q = R.dequant_rows_mxfp4(codes, e8) / scale
    unsat = v.abs() <= 6
    err = (v - q).abs()
    assert bool((err[unsat] <= grid_spacing_half(v.abs())[unsat]).all())
    assert bool((q[~unsat].abs() == 6).all()) and bool((q.sign() * v.sign() >= 0).all())
    # every block's amax lands in [4, 8): its code is magnitude 4 or 6
    top = q.abs().reshape(96, 65, 32).amax(dim=2)
    assert bool(((top == 4) | (top == 6)).all())
    rel = float(((R.dequant_rows_mxfp4(codes, e8) - w.float()).pow(2).mean()
                 / w.float().pow(2).mean()).sqrt())
    sat = float((~unsat).float().mean())
    print(f"mxfp4 N(0, 0.02^2): relative rms error {rel:.4f}, saturated {sat:.4f}")
    assert 0.08 < rel < 0.15


def test_grid_matrix_round_trip_is_bit_equal():
    w, codes, e8 = grid_matrix(33, 2080, torch.Generator().manual_seed(5))
    c2, s2 = R.quant_rows_mxfp4(w)
    assert torch.equal(c2, codes) and torch.equal(s2, e8)
    assert int(((_nibbles(codes) == 8).sum())) > 0  # -0 codes survive
    assert torch.equal(R.dequant_rows_mxfp4(c2, s2).to(torch.bfloat16).view(torch.int16),
                       w.view(torch.int16))


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    return write_grid_checkpoint(tmp_path_factory.mktemp("mxfp4_grid"))


def test_grid_checkpoint_is_lossless(grid):
    ts = projection_tensors(grid)
    assert len(ts) == 3 * 7
    scales = set()
    for name, w in ts.items():
        assert w.dtype == torch.bfloat16 and w.shape[1] % 32 == 0
        codes, e8 = R.quant_rows_mxfp4(w)
        assert torch.equal(R.dequant_rows_mxfp4(codes, e8).to(torch.bfloat16), w), name
        scales |= set(e8.reshape(-1).tolist())
    assert scales == {119, 120, 121}
    std = torch.cat([w.float().reshape(-1) for w in ts.values()]).std()
    # uniform codes have rms 2.9, the three exponents an rms scale of 0.0103: 0.030, the
    # order of the synthetic checkpoints' 0.02
    assert 0.02 < float(std) < 0.04


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_mxfp4_and_rejects_bogus(entry):
    head = [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]
    r = _run([*head, "--help"])
    assert r.returncode == 0 and "--weight-dtype" in r.stdout and "mxfp4" in r.stdout
    r = _run([*head, "--weight-dtype", "bogus"])
    assert r.returncode == 2 and "--weight-dtype" in r.stderr, r.stderr


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_mxfp4_refused_on_the_python_path(grid, tmp_path, entry):
    """CAKE_NATIVE=0 keeps the Python generator, which has no mxfp4 weights: it refuses
    with a message and never runs 16-bit instead."""
    head = [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]
    r = _run([*head, "--model", str(grid), "--topology", str(tmp_path / "none.yml"),
              "--weight-dtype", "mxfp4", "--temperature", "0", "-n", "2", "--prompt", "hi"],
             CAKE_NATIVE="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--weight-dtype mxfp4" in r.stderr and "native Llama engine" in r.stderr
    assert r.stdout.strip() == ""  # nothing was generated
