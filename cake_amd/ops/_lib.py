"""ctypes binding of ``libcake_kernels.so`` (the gfx950 HIP kernels).

The library exposes a plain C ABI; each entry point takes raw device pointers
plus the HIP stream to launch on.  We pass torch's *current* stream so that a
``torch.cuda.graph`` capture records our launches like any torch op.

On a machine with a GPU the library is mandatory: :func:`kernels` raises if it
is missing rather than silently falling back to PyTorch ops.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

_LIB_PATH = Path(__file__).resolve().parent.parent / "lib" / "libcake_kernels.so"
_lock = threading.Lock()
_lib = None

P = C.c_void_p
I = C.c_int
F = C.c_float
D = C.c_double
Z = C.c_size_t
L = C.c_longlong
U = C.c_ulonglong

# Every entry point of the kernel library: name -> (restype, argtypes), in the order of
# csrc/kernels/cake_kernels.h (None: void; I results are a hipError_t unless the header says
# otherwise; P: any pointer or the hipStream_t).  A literal mirror of the header, kept honest
# by tests/test_abi_cpu.py; adding an entry point: docs/ABI.md.
_SIGS = {
    # kernels/allreduce.hip
    "cake_ar_inbox_words": (L, [I, I]),
    "cake_ar_sum": (I, [P, P, I, I, P, P, P, P, I, I, D, P]),
    "cake_ar_max_key": (I, [P, P, P, P, P, I, I, D, P]),
    "cake_ar_gather": (I, [P, I, I, P, I, P, P, P, P, I, I, D, P]),
    # kernels/attention.hip
    "cake_attn_set_impl": (I, [I]),
    "cake_attn_set_stamps": (I, [P]),
    "cake_attn_set_split_cap": (I, [I]),
    "cake_attn_set_target_splits": (I, [I]),
    "cake_attn_set_prefetch": (I, [I]),
    "cake_attn_set_single_max": (I, [I]),
    "cake_attn_debug_drop_partials": (I, [I]),
    "cake_attn_splits": (I, [I]),
    "cake_attn_max_split": (I, [I]),
    "cake_attn_set_min_keys": (I, [I]),
    "cake_attn_decode": (I, [I, P, P, P, P, I, I, I, I, F, P, P, P, P]),
    "cake_attn_decode_kv8": (I, [I, P, P, P, P, I, I, I, I, F, P, P, P, P]),
    "cake_attn_set_head_prefetch": (I, [I]),
    "cake_attn_set_heads": (I, [I, I]),
    "cake_attn_heads_max": (I, []),
    "cake_attn_decode_heads": (I, [I, P, P, P, P, I, I, I, I, F, P, P]),
    # kernels/attn512.hip
    "cake_attn512": (I, [I, P, P, P, P, I, I, I, L, L, L, L, L, L, L, L, F, P, P]),
    # kernels/conv2d.hip
    "cake_conv1x1_small": (I, [I, P, P, P, P, I, I, I, I, I, P]),
    "cake_conv2d_workspace": (L, [I, I, I]),
    "cake_conv2d_nhwc2": (I, [I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I,
                              I, I, P]),
    "cake_conv2d_nhwc": (I, [I, P, P, P, P, P, P, P, P, I, I, I, I, I, I, I, I, I, I, I, I, I, I,
                             I, P]),
    # kernels/elementwise.hip
    "cake_sum_slices": (I, [P, P, I, L, L, I, P]),
    "cake_stream_read": (I, [P, Z, I, P, P]),
    "cake_cast16": (I, [I, I, P, P, Z, P]),
    "cake_fill_normal": (I, [I, P, Z, F, F, U, P]),
    "cake_embed": (I, [I, P, P, I, I, P, P]),
    "cake_rmsnorm_set_reg": (None, [I]),
    "cake_rmsnorm": (I, [I, P, P, F, I, I, P, P]),
    "cake_rope_kv": (I, [I, P, P, P, I, I, I, I, I, I, P, I, I, P, P, P]),
    "cake_rope_kv_kvf": (I, [I, P, P, P, I, I, I, I, I, I, P, I, I, P, P, P, I]),
    "cake_dequant_kv_fp8": (I, [I, P, P, I, I, I, I, P, P, P]),
    "cake_silu_mul": (I, [I, P, P, Z, P, P]),
    "cake_silu_mul_rows": (I, [I, P, Z, I, P, P]),
    "cake_add_resid": (I, [I, P, P, Z, P]),
    "cake_wave_reduce_probe": (I, [P, P, P]),
    # kernels/flash_attn.hip
    "cake_flash_set_impl": (None, [I]),
    "cake_flash_set_nw": (None, [I]),
    "cake_flash_set_pair_min": (None, [L]),
    "cake_flash_set_ksplit": (None, [I]),
    "cake_flash_attn_ws": (I, [I, P, P, P, P, I, I, I, I, I, I, P, F, I, I, P, L, P]),
    "cake_flash_attn": (I, [I, P, P, P, P, I, I, I, I, I, I, P, F, I, I, P]),
    # kernels/gemm.hip
    "cake_gemm_tile": (I, [I, P, P]),
    "cake_gemm_ws_floats": (L, [I, I, I, I, I, I]),
    "cake_gemm": (I, [I, I, I, I, P, L, P, L, P, L, P, P, L, P, P, I, I, I, P]),
    # kernels/gemm_w8a8.hip
    "cake_gemm_w8a8_num_cfgs": (I, []),
    "cake_gemm_w8a8_plan": (I, [I, I, I]),
    "cake_gemm_w8a8": (I, [I, I, I, P, L, P, P, L, P, P, L, P, L, I, I, I, P]),
    # kernels/gemv.hip
    "cake_gemv_set_tuning": (I, [I, I, I, I]),
    "cake_qkv_rope_kvf": (I, [I, P, P, F, P, P, P, I, I, I, I, P, P, P, P, P, I, P, I]),
    "cake_qkv_rope": (I, [I, P, P, F, P, P, P, I, I, I, I, P, P, P, P, P, I, P]),
    # kernels/gemv_head.hip
    "cake_gemv_norm_f32": (I, [I, P, P, F, P, I, I, P, P]),
    "cake_head_select": (I, [I, P, P, F, P, I, I, P, P, P, I, F, P, P, P, P, I, P, P, P]),
    # kernels/gemv_mlp.hip
    "cake_swiglu": (I, [I, P, P, F, P, P, I, I, P, P]),
    "cake_gemv_x16": (I, [I, P, P, I, I, P, I, P]),
    # kernels/gemv_p13.hip: lossless 13-bit bf16 projections (with pack13.hip
    "cake_gemv_p13_set_tuning": (I, [I, I, I, I]),
    "cake_gemv_p13_get_tuning": (I, [I, P]),
    "cake_qkv_rope_p13_kvf": (I, [I, P, P, F, P, P, P, P, P, P, P, P, P, I, I, I, I, P, P, P, P,
                                  P, I, P, I]),
    # kernels/gemv_p13_head.hip: the packed lm_head
    "cake_gemv_norm_f32_p13": (I, [I, P, P, F, P, P, P, I, I, P, P]),
    "cake_head_select_p13": (I, [I, P, P, F, P, P, P, I, I, P, P, P, I, F, P, P, P, P, I, P, P,
                                 P]),
    # kernels/gemv_p13_mlp.hip
    "cake_swiglu_p13": (I, [I, P, P, F, P, P, P, P, P, P, I, I, P, P]),
    "cake_gemv_x16_p13": (I, [I, P, P, P, P, I, I, P, I, P]),
    # kernels/gemv_rows.hip: the projections of a lock-step batched decode step
    "cake_gemv_rows_set_tuning": (I, [I, I, I, I]),
    "cake_gemv_rows_get_tuning": (I, [I, P]),
    "cake_gemv_rows": (I, [I, I, P, L, P, L, P, L, P, L, I, I, I, P]),
    "cake_rmsnorm_split_rows": (I, [I, P, P, F, I, I, P, P]),
    "cake_rope_kv_rows": (I, [I, P, L, I, P, P, I, I, I, I, P, P, P, L, P]),
    # kernels/gemv_w4.hip: MXFP4 weight-only projections (with quant_mxfp4.hip
    "cake_gemv_w4_set_tuning": (I, [I, I, I, I]),
    "cake_gemv_w4_get_tuning": (I, [I, P]),
    "cake_qkv_rope_w4_kvf": (I, [I, P, P, F, P, P, P, P, P, P, I, I, I, I, P, P, P, P, P, I, P,
                                 I]),
    "cake_qkv_rope_w4": (I, [I, P, P, F, P, P, P, P, P, P, I, I, I, I, P, P, P, P, P, I, P]),
    # kernels/gemv_w4_head.hip: quantised lm_head
    "cake_gemv_norm_f32_w4": (I, [I, P, P, F, P, P, I, I, P, P]),
    "cake_head_select_w4": (I, [I, P, P, F, P, P, I, I, P, P, P, I, F, P, P, P, P, I, P, P, P]),
    # kernels/gemv_w4_mlp.hip
    "cake_swiglu_w4": (I, [I, P, P, F, P, P, P, P, I, I, P, P]),
    # kernels/gemv_w4_x16.hip
    "cake_gemv_x16_w4": (I, [I, P, P, P, I, I, P, I, P]),
    # kernels/gemv_w8.hip: FP8 e4m3fn weight-only projections (with quant_fp8.hip
    "cake_gemv_w8_set_tuning": (I, [I, I, I, I]),
    "cake_gemv_w8_get_tuning": (I, [I, P]),
    "cake_qkv_rope_w8_kvf": (I, [I, P, P, F, P, P, P, P, P, P, I, I, I, I, P, P, P, P, P, I, P,
                                 I]),
    "cake_qkv_rope_w8": (I, [I, P, P, F, P, P, P, P, P, P, I, I, I, I, P, P, P, P, P, I, P]),
    # kernels/gemv_w8_head.hip: quantised lm_head
    "cake_gemv_norm_f32_w8": (I, [I, P, P, F, P, P, I, I, P, P]),
    "cake_head_select_w8": (I, [I, P, P, F, P, P, I, I, P, P, P, I, F, P, P, P, P, I, P, P, P]),
    # kernels/gemv_w8_mlp.hip
    "cake_swiglu_w8": (I, [I, P, P, F, P, P, P, P, I, I, P, P]),
    # kernels/gemv_w8_x16.hip
    "cake_gemv_x16_w8": (I, [I, P, P, P, I, I, P, I, P]),
    # kernels/hop.hip
    "cake_hop_alloc": (I, [Z, P]),
    "cake_hop_free": (I, [P]),
    "cake_ipc_handle": (I, [P, P]),
    "cake_ipc_handle_size": (I, []),
    "cake_ipc_open": (I, [P, P]),
    "cake_ipc_close": (I, [P]),
    "cake_hop_words": (I, [I, I, I]),
    "cake_hop_send": (I, [P, I, I, I, P, P, P]),
    "cake_hop_recv": (I, [P, I, I, I, P, P, P, D, P]),
    "cake_bulk_send": (I, [P, P, P, I, P, U, P, P, P]),
    "cake_bulk_recv": (I, [P, U, P, P, P, D, P]),
    # kernels/logit_controls.hip: count penalties, logit_bias and the min_p cut
    "cake_logit_controls": (I, [P, I, P, P, P, P, P, I, P]),
    "cake_logit_controls_merge_thr": (I, [P, P, P]),
    # kernels/logprob.hip: log-probs of a generated token
    "cake_logprob_ws_bytes": (L, [I]),
    "cake_logprob_topk": (I, [P, I, P, P, I, P, I, P, P, I, P]),
    # kernels/pack13.hip: bf16 rows <-> their lossless 13-bit form
    "cake_pack13_bytes": (L, [I, I, I]),
    "cake_pack13_rows": (I, [I, P, I, I, I, P, P, P, I, P]),
    "cake_unpack13_rows": (I, [P, P, P, I, I, P, P]),
    # kernels/quant_fp8.hip
    "cake_quant_rows_fp8": (I, [I, P, I, I, P, P, P]),
    "cake_dequant_rows_fp8": (I, [I, P, P, I, I, P, P]),
    # kernels/quant_mxfp4.hip
    "cake_quant_rows_mxfp4": (I, [I, P, I, I, P, P, P]),
    "cake_dequant_rows_mxfp4": (I, [I, P, P, I, I, P, P]),
    # kernels/sampling.hip
    "cake_sample_threshold": (I, [P, I, F, I, F, P, P]),
    "cake_select_dev": (I, [P, I, P, P, P, P, P]),
    "cake_gumbel_argmax": (I, [P, I, F, U, P, P, P, P]),
    "cake_repeat_penalty": (I, [P, P, P, I, F, P]),
    "cake_argmax": (I, [P, I, P, P]),
    "cake_select_shard": (I, [P, I, I, P, P, I, F, F, U, P, P]),
    "cake_finalize_token": (I, [P, P, P, P, P, I, P]),
    "cake_push_token": (I, [P, P, P, P, P, I, P]),
    # kernels/score.hip: sequence scoring
    "cake_lse_rows": (I, [P, L, I, I, I, I, P, P, P, P, P, P]),
    "cake_lse_finish": (I, [P, P, P, I, P, P, P, P]),
    # kernels/sd_norm.hip
    "cake_groupnorm": (I, [I, P, P, P, I, I, L, I, F, I, P, P, P]),
    "cake_layernorm": (I, [I, P, P, P, L, I, F, P, P]),
    "cake_geglu": (I, [I, P, L, I, P, P]),
    "cake_groupnorm_nhwc_splits": (I, [I]),
    "cake_groupnorm_nhwc2": (I, [I, P, P, I, P, P, P, I, I, I, I, F, I, P, P, P, P, P]),
    "cake_groupnorm_nhwc": (I, [I, P, P, P, I, I, I, I, F, I, P, P, P, P, P]),
    # kernels/sd_small.hip
    "cake_timestep_embed": (I, [I, P, P, I, I, I, F, I, P, P]),
    "cake_sched_step": (I, [I, P, P, L, I, F, P, P, P, P, P]),
    "cake_step_advance": (I, [P, P]),
    "cake_scale_copy": (I, [I, P, L, F, I, P, P]),
    "cake_to_rgb8": (I, [I, P, I, I, I, I, P, P]),
    "cake_clip_embed": (I, [I, P, P, P, I, I, I, I, P, P]),
    "cake_widen16": (I, [I, P, L, P, P]),
    # driver/blaslt.cpp
    "cake_blaslt_gemm": (I, [I, I, P, L, P, L, P, L, I, I, I, P, Z, P]),
    # driver/graph_loop.cpp (declared in driver/graph_loop.h: LoopSpec / LoopResult of
    # ops/graph_loop.py by reference)
    "cake_graph_decode": (I, [P, P]),
    # ==== experimental: only in CAKE_BUILD_EXPERIMENTAL=1 builds (_OPTIONAL)
    # experimental/attn_oproj.hip
    "cake_attn_oproj_supported": (I, [I, I, I, I]),
    "cake_attn_oproj_ws_floats": (L, [I, I]),
    "cake_attn_oproj_ticket_words": (L, [I, I]),
    "cake_attn_oproj": (I, [I, P, P, P, P, I, I, I, I, F, P, I, I, P, I, P, P, P, P]),
    # experimental/decode_mk.hip
    "cake_mk_gstride": (L, [I, I, I, I, I]),
    "cake_mk_grid": (I, []),
    "cake_mk_set_stamps": (I, [P]),
    "cake_mk_set_tuning": (I, [I, I, I, I]),
    "cake_mk_supported": (I, [I, I, I, I, I]),
    "cake_mk_decode": (I, [I, P, I, I, I, I, I, I, I, F, F, P, P, P, P, P, D, P]),
}
# entry points of csrc/experimental (not in the default build): the fused decode attention +
# o_proj (measured slower: profiles/r5_attn_oproj_ab.md) and the persistent decode engine
_OPTIONAL = {"cake_attn_oproj_supported", "cake_attn_oproj_ws_floats",
             "cake_attn_oproj_ticket_words", "cake_attn_oproj",
             "cake_mk_gstride", "cake_mk_grid", "cake_mk_set_stamps", "cake_mk_set_tuning",
             "cake_mk_supported", "cake_mk_decode"}


class KernelError(RuntimeError):
    pass


def lib_path() -> Path:
    return Path(os.environ.get("CAKE_KERNEL_LIB", _LIB_PATH))


def kernels():
    """Load (once) and return the kernel library; raise if it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            import torch  # noqa: F401  (HIP runtime must be loaded by torch first)

            path = lib_path()
            if not path.exists():
                raise KernelError(
                    f"{path} not built; run `python -m cake_amd.build` (hipcc gfx950)")
            lib = C.CDLL(str(path), mode=C.RTLD_GLOBAL)
            for name, (restype, argtypes) in _SIGS.items():
                if name in _OPTIONAL and not hasattr(lib, name):
                    continue  # csrc/experimental, built with CAKE_BUILD_EXPERIMENTAL=1
                fn = getattr(lib, name)
                fn.argtypes = argtypes
                fn.restype = restype
            _lib = lib
    return _lib


def available() -> bool:
    try:
        kernels()
        return True
    except (KernelError, OSError):
        return False


def check(rc: int, name: str) -> None:
    if rc != 0:
        raise KernelError(f"{name} failed with hipError {rc}")
