"""The native engine with and without the packed (lossless 13-bit) copies of its bf16 weights
(CAKE_PACK16, docs/ENV.md): the same tokens and bit-equal logits, the copies reported by
packed_bytes() beside an unchanged weight_bytes().  Each engine runs in a fresh process: the
knob is read at open."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]

# "issue": of the kinds packed by default (gate | up, down_proj) down_proj alone has K a
# multiple of the 2048-value tile; "wide": both do, and with CAKE_PACK16_KINDS naming every
# kind (ALL_KINDS) so do q | k | v, o_proj and the lm_head
CONFIGS = {
    "issue": dict(hidden_size=1024, intermediate_size=2048, num_attention_heads=8,
                  num_key_value_heads=2, num_hidden_layers=2, vocab_size=512),
    "wide": dict(hidden_size=2048, intermediate_size=4096, num_attention_heads=16,
                 num_key_value_heads=4, num_hidden_layers=2, vocab_size=512),
}
ALL_KINDS = "qkv,o,gu,down,head"

CHILD = r"""
import json, sys
import numpy as np
from cake_amd.engine import NativeLlama, write_config
from cake_amd.models.llama3.config import preset
out, overrides, dtype, head = sys.argv[1], json.loads(sys.argv[2]), sys.argv[3], sys.argv[4]
d = write_config(out + "/model", preset("tiny", **overrides))
eng = NativeLlama(d, max_seq=256, dtype=dtype, random_init=True, seed=5, head=head)
prompt = [1, 5, 7, 9, 11, 13, 17, 19]
res = dict(packed=eng.packed_bytes(), weights=eng.weight_bytes())
res["greedy"] = eng.generate(prompt, 48, repeat_penalty=1.1).tokens
res["sampled"] = eng.generate(prompt, 24, temperature=0.8, top_k=40, top_p=0.95, seed=1234,
                              repeat_penalty=1.0).tokens
np.save(out + "/forced.npy", eng.forced_logits(prompt, res["greedy"][:6]))
eng.close()
print("RESULT " + json.dumps(res))
"""


def _run(tmp_path, name, cfg, pack, dtype="bf16", kinds=None, head="model"):
    out = tmp_path / name
    out.mkdir()
    env = {k: v for k, v in os.environ.items() if not k.startswith("CAKE_PACK16")}
    if pack is not None:
        env["CAKE_PACK16"] = pack
    if kinds is not None:
        env["CAKE_PACK16_KINDS"] = kinds
    env["PYTHONPATH"] = str(ROOT) + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, "-c", CHILD, str(out), json.dumps(CONFIGS[cfg]), dtype,
                        head],
                       capture_output=True, text=True, env=env, timeout=300)
    if r.returncode != 0:
        return None, r.stderr
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    res = json.loads(line[len("RESULT "):])
    res["forced"] = np.load(out / "forced.npy")
    return res, r.stderr


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_packed_engine_equals_the_16_bit_engine(tmp_path, cfg):
    off, _ = _run(tmp_path, "off", cfg, "0")
    on, log = _run(tmp_path, "on", cfg, None)
    assert off is not None and on is not None, log
    assert on["greedy"] == off["greedy"] and len(on["greedy"]) == 48
    assert on["sampled"] == off["sampled"] and len(on["sampled"]) == 24
    assert np.array_equal(on["forced"].view(np.int32), off["forced"].view(np.int32))
    assert np.isfinite(on["forced"]).all()
    assert off["packed"] == 0 and on["packed"] > 0
    assert on["weights"] == off["weights"]
    assert "packed to 13 bits" in log
    c = CONFIGS[cfg]
    H, I, L = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"]
    if cfg == "issue":  # down_proj [H, I] of both layers, and nothing else
        assert on["packed"] >= L * H * I * 13 // 8
        assert on["packed"] < L * H * I * 2


def test_every_kind_packed_equals_the_16_bit_engine(tmp_path):
    """The kinds the default leaves 16-bit (q | k | v, o_proj, the lm_head: forced_logits, the
    fused greedy selection and the sampled head) run packed when CAKE_PACK16_KINDS names them."""
    off, _ = _run(tmp_path, "off", "wide", "0")
    dflt, _ = _run(tmp_path, "dflt", "wide", None)
    every, log = _run(tmp_path, "all", "wide", "1", kinds=ALL_KINDS)
    assert off is not None and dflt is not None and every is not None, log
    assert every["greedy"] == off["greedy"] and len(every["greedy"]) == 48
    assert every["sampled"] == off["sampled"] and len(every["sampled"]) == 24
    assert np.array_equal(every["forced"].view(np.int32), off["forced"].view(np.int32))
    assert every["weights"] == off["weights"]
    c = CONFIGS["wide"]
    H, I, L, V = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"], c["vocab_size"]
    nq = c["num_attention_heads"] * 128
    nk = c["num_key_value_heads"] * 128
    values = L * ((nq + 2 * nk) * H + H * nq + 3 * H * I) + V * H
    assert values * 13 // 8 <= every["packed"] < values * 2
    assert every["packed"] > dflt["packed"] >= L * 3 * H * I * 13 // 8


@pytest.mark.parametrize("head", ["fp8", "mxfp4"])
def test_packed_projections_with_a_quantised_head(tmp_path, head):
    """Every projection packed beside a quantised lm_head: the head keeps its own format (it
    has no 16-bit rows to pack) and the packed projections change no token and no logit bit."""
    off, _ = _run(tmp_path, "off", "wide", "0", head=head)
    every, log = _run(tmp_path, "all", "wide", "1", kinds=ALL_KINDS, head=head)
    assert off is not None and every is not None, log
    assert every["greedy"] == off["greedy"] and len(every["greedy"]) == 48
    assert every["sampled"] == off["sampled"] and len(every["sampled"]) == 24
    assert np.array_equal(every["forced"].view(np.int32), off["forced"].view(np.int32))
    assert every["weights"] == off["weights"]
    c = CONFIGS["wide"]
    H, I, L = c["hidden_size"], c["intermediate_size"], c["num_hidden_layers"]
    nq = c["num_attention_heads"] * 128
    nk = c["num_key_value_heads"] * 128
    values = L * ((nq + 2 * nk) * H + H * nq + 3 * H * I)  # without the head's V * H
    assert values * 13 // 8 <= every["packed"] < values * 2
    assert off["packed"] == 0


def test_required_packing_refuses_f16(tmp_path):
    """CAKE_PACK16=1 asks for packed copies; an f16 engine has nothing to pack: open fails
    (docs/ENV.md).  Unset, the same engine opens and packs nothing."""
    res, log = _run(tmp_path, "req", "issue", "1", dtype="f16")
    assert res is None and "CAKE_PACK16=1" in log
    res, log = _run(tmp_path, "auto", "issue", None, dtype="f16")
    assert res is not None and res["packed"] == 0, log
    res, log = _run(tmp_path, "req16", "issue", "1")
    assert res is not None and res["packed"] > 0, log
