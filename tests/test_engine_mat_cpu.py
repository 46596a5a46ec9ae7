"""cake::Mat (csrc/engine/llama_weights.h), the engine's one weight-matrix type: the byte
offsets of a sub-matrix (q | k | v, gate | up) in every weight format and the byte totals,
checked by a stand-alone host program (csrc/tests/mat_selftest.cpp) against literal values.
Host code only: nothing is launched."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ROCM_INCLUDE = Path(os.environ.get("ROCM_PATH", "/opt/rocm")) / "include"


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
@pytest.mark.skipif(not (ROCM_INCLUDE / "hip" / "hip_runtime_api.h").exists(),
                    reason="ROCm include directory not found")
def test_mat_offsets_and_bytes(tmp_path):
    exe = tmp_path / "mat_selftest"
    src = ROOT / "cake_amd" / "csrc" / "tests" / "mat_selftest.cpp"
    c = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__",
                        f"-I{ROCM_INCLUDE}", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=120)
    assert c.returncode == 0, c.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    assert "mat selftest ok" in r.stdout
