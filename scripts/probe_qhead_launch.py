"""The lm_head launches at the 8B shape (V 128256, H 4096), outside the engine: each timed
inside a captured graph of 20 back-to-back calls (no host launch gaps).  Per head format the
plain f32-logits launch and the fused greedy tail with the penalty on / off and with / without
the embedding row; then the quantised heads over grid caps.

    python scripts/probe_qhead_launch.py > profiles/qhead_head_launch_probe.jsonl
"""
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cake_amd.ops import hip as K_  # noqa: E402

V, H = 128256, 4096
dev = "cuda"
dt = torch.bfloat16
g = torch.Generator(device=dev).manual_seed(1)
resid = torch.randn(H, device=dev, generator=g) * 3
nw = torch.ones(H, device=dev, dtype=dt)
w16 = (torch.randn(V, H, device=dev, generator=g) * 0.02).to(dt)
w8 = torch.empty(V, H, dtype=torch.uint8, device=dev)
s8 = torch.empty(V, device=dev)
K_.quant_rows_fp8(w16, w8, s8)
w4 = torch.empty(V, H // 2, dtype=torch.uint8, device=dev)
e8 = torch.empty(V, H // 32, dtype=torch.uint8, device=dev)
K_.quant_rows_mxfp4(w16, w4, e8)
table = (torch.randn(V, H, device=dev, generator=g)).to(dt)
logits = torch.empty(V, device=dev)
hist = torch.randint(0, V, (8192,), dtype=torch.int32, device=dev)
REP = 20


def state():
    return dict(hist_len=torch.tensor([300], dtype=torch.int32, device=dev),
                tok=torch.zeros(1, dtype=torch.int32, device=dev),
                pos=torch.tensor([299], dtype=torch.int32, device=dev),
                slot=torch.zeros(1, dtype=torch.int64, device=dev),
                ticket=torch.zeros(1, dtype=torch.int32, device=dev))


def graph_time(fn):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            for _ in range(REP):
                fn()
        ts = []
        for _ in range(8):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            gr.replay()
            b.record(st)
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) * 1e3 / REP)
    ts.sort()
    return round(ts[len(ts) // 2], 1)


def sel(fmt, pen, emb):
    s = state()
    r = resid.clone()
    e = table if emb else None
    kw = dict(embed=e)
    if fmt == "fp8":
        return lambda: K_.head_select_w8(r, nw, 1e-5, w8, s8, logits, hist, s["hist_len"], 128, pen,
                                         s["slot"], s["ticket"], s["tok"], s["pos"], **kw)
    if fmt == "mxfp4":
        return lambda: K_.head_select_w4(r, nw, 1e-5, w4, e8, logits, hist, s["hist_len"], 128, pen,
                                         s["slot"], s["ticket"], s["tok"], s["pos"], **kw)
    return lambda: K_.head_select(r, nw, 1e-5, w16, logits, hist, s["hist_len"], 128, pen,
                                  s["slot"], s["ticket"], s["tok"], s["pos"], **kw)


def plain(fmt):
    if fmt == "fp8":
        return lambda: K_.norm_gemv_f32_w8(resid, nw, 1e-5, w8, s8, logits)
    if fmt == "mxfp4":
        return lambda: K_.norm_gemv_f32_w4(resid, nw, 1e-5, w4, e8, logits)
    return lambda: K_.norm_gemv_f32(resid, nw, 1e-5, w16, logits)


for fmt in ("model", "fp8", "mxfp4"):
    rec = {"head": fmt, "plain_us": graph_time(plain(fmt))}
    for pen in (1.0, 1.1):
        for emb in (False, True):
            rec[f"sel_pen{pen}_embed{int(emb)}_us"] = graph_time(sel(fmt, pen, emb))
    print(json.dumps(rec), flush=True)
base8, base4 = K_.get_gemv_w8_tuning("head"), K_.get_gemv_w4_tuning("head")
for mb in (128, 256, 512, 2048):
    K_.set_gemv_w8_tuning("head", U=2, prefetch=4, max_blocks=mb)
    K_.set_gemv_w4_tuning("head", U=2, prefetch=4, max_blocks=mb)
    print(json.dumps({"max_blocks": mb,
                      "fp8": {"plain_us": graph_time(plain("fp8")),
                              "sel_us": graph_time(sel("fp8", 1.1, True))},
                      "mxfp4": {"plain_us": graph_time(plain("mxfp4")),
                                "sel_us": graph_time(sel("mxfp4", 1.1, True))}}), flush=True)
K_.set_gemv_w8_tuning("head", U=base8[0], prefetch=base8[1], max_blocks=base8[2])
K_.set_gemv_w4_tuning("head", U=base4[0], prefetch=base4[1], max_blocks=base4[2])
