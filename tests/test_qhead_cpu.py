"""Quantised lm_head (--head-dtype) on the CPU: the flag of both entry points, the layout of
CakeEngineOpts, and the lossless grid-head checkpoint of tests/_qhead.py."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

from _qhead import (FORMATS, UNIT_EXPONENTS, dequant, grid_matrix, head_tensor, quant,
                    write_grid_head_checkpoint)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "cake_amd", "lib", "cake-cli")


def _run(cmd, **env):
    e = dict(os.environ, CAKE_LOG="warning", **env)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=180, env=e, cwd=ROOT)


def _entry(entry):
    return [CLI] if entry == "cake-cli" else [sys.executable, "-m", "cake_amd.cli"]


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_cli_lists_head_dtype_and_rejects_bogus(entry):
    r = _run([*_entry(entry), "--help"])
    assert r.returncode == 0 and "--head-dtype" in r.stdout
    after = r.stdout[r.stdout.index("--head-dtype"):][:600]
    assert "fp8" in after and "mxfp4" in after
    r = _run([*_entry(entry), "--head-dtype", "bogus"])
    assert r.returncode == 2 and "--head-dtype" in r.stderr, r.stderr


@pytest.fixture(scope="module")
def grid_head(tmp_path_factory):
    return write_grid_head_checkpoint(tmp_path_factory.mktemp("qhead_grid"), "fp8")


@pytest.mark.parametrize("entry", ["cake-cli", "python"])
def test_head_dtype_refused_on_the_python_path(grid_head, tmp_path, entry):
    """CAKE_NATIVE=0 keeps the Python generator, which has no quantised head: it refuses with
    the --weight-dtype wording and never runs 16-bit instead."""
    r = _run([*_entry(entry), "--model", str(grid_head), "--topology", str(tmp_path / "none.yml"),
              "--head-dtype", "fp8", "--temperature", "0", "-n", "2", "--prompt", "hi"],
             CAKE_NATIVE="0")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert "--head-dtype fp8" in r.stderr and "native Llama engine" in r.stderr
    assert r.stdout.strip() == ""  # nothing was generated


def test_engine_opts_layout():
    """CakeEngineOpts: six int32, the 8-byte seed at 24, head_fmt appended at 32; 40 bytes."""
    from cake_amd.engine import EngineOpts
    assert C.sizeof(EngineOpts) == 40
    assert EngineOpts.head_fmt.offset == 32 and EngineOpts.head_fmt.size == 4
    assert EngineOpts.seed.offset == 24 and EngineOpts.weight_fmt.offset == 20
    o = EngineOpts(256, 0, 0, 1, 0, 2, 7)  # callers that stop at the seed: head_fmt 0
    assert o.head_fmt == 0 and o.weight_fmt == 2 and o.seed == 7


def test_native_llama_rejects_an_unknown_head_before_opening():
    from cake_amd.engine import NativeLlama
    with pytest.raises(ValueError, match="head"):
        NativeLlama("/nonexistent", head="int4")


@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_head_checkpoint_is_lossless(tmp_path, fmt):
    d = write_grid_head_checkpoint(tmp_path, fmt)
    w = head_tensor(d)
    assert w.dtype == torch.bfloat16 and tuple(w.shape) == (2048, 512)
    codes, scales = quant(fmt, w)
    back = dequant(fmt, codes, scales).to(torch.bfloat16)
    assert torch.equal(back.view(torch.int16), w.view(torch.int16))
    # the base checkpoint's head is not on the grid: quantisation changes it
    base = head_tensor(tmp_path / "base")
    assert int((dequant(fmt, *quant(fmt, base)).to(torch.bfloat16) != base).sum()) > 0
    # the order of the synthetic head's std of 0.02
    assert 0.01 < float(w.float().std()) < 0.05


@pytest.mark.parametrize("fmt", FORMATS)
def test_unit_scale_grid_is_exact_in_bf16(fmt):
    """The tied-embedding grid: exponents suited to N(0, 1) rows, still bit-exact."""
    w, codes, scales = grid_matrix(fmt, 64, 512, torch.Generator().manual_seed(9),
                                   UNIT_EXPONENTS[fmt])
    c2, s2 = quant(fmt, w)
    assert torch.equal(c2, codes) and torch.equal(s2.float(), scales.float())
    assert 0.3 < float(w.float().std()) < 3.0
