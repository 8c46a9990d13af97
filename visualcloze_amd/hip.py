"""ctypes binding of libvcloze_hip.so (the C ABI in include/vcloze_hip.h).

torch is used here only for device memory and streams: every wrapper takes torch CUDA tensors, checks
dtype / contiguity on the host and hands raw device pointers to the library.  There is NO fallback:
a missing library or a missing GPU raises (`VclozeHipError`)."""
from __future__ import annotations

import ctypes as C
import functools
import os
import subprocess
from typing import Optional

import numpy as np
import torch  # noqa: F401  (must be imported first so the process shares torch's HIP runtime)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VC_HIP_LIB") or os.path.join(_HERE, "lib", "libvcloze_hip.so")   # VC_HIP_LIB: profiling build
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 11               # VC_ABI_VERSION of include/vcloze_hip.h
SOLVER_EULER, SOLVER_MIDPOINT, SOLVER_RK4 = 0, 1, 2     # VC_SOLVER_*: the fixed-grid methods of the fused sampling loop
SOLVERS = {"euler": SOLVER_EULER, "midpoint": SOLVER_MIDPOINT, "rk4": SOLVER_RK4}
SDE_EM, SDE_HEUN1, SDE_HEUN2, SDE_LAST, SDE_INJECT, SDE_ROW = 0, 1, 2, 3, 4, 5     # VC_SDE_*: the row modes of vc_sde_stage, values per row
MS_ROW, MS_HIST = 4, 3         # VC_MS_ROW / VC_MS_HIST: coefficients per row (= the highest order) and ring planes of vc_ms_stage
GEMM_MAX_PROBLEMS = 4          # VC_GEMM_MAX_PROBLEMS: grouped problems per vc_gemm launch
EPI_BIAS, EPI_GELU, EPI_GATE_RES, EPI_SILU, EPI_QKV = 0, 1, 2, 3, 4
GEMM_NO_SPLIT = 64             # VC_GEMM_NO_SPLIT: tile_cfg value that keeps an auto-tiled vc_gemm one launch
GEMM_PERSIST = 128             # VC_GEMM_PERSIST: opt into the persistent tile loop of the loader-wave GEMM (multi-round launches)
GEMM_NO_SPLITK = 1 << 20       # VC_GEMM_NO_SPLITK: an auto-tiled call keeps its remainder tiles whole even with a splitk_ws
GEMM_STREAMK = 1 << 21         # VC_GEMM_STREAMK: force the stream form of the split-K remainder (tests, A/B runs)
GEMM_PREFER_STREAMK = 1 << 22  # VC_GEMM_PREFER_STREAMK: auto-tiled calls take the stream form wherever eligible (A/B runs)
GEMM_STREAMK_ANY_K = 1 << 23   # VC_GEMM_STREAMK_ANY_K: ... at any K
GEMM_SPLITK_WS_BYTES = 2 * 256 * 256 * 192 * 4     # VC_GEMM_SPLITK_WS_BYTES


def GEMM_SPLITK(S: int) -> int:
    """VC_GEMM_SPLITK(S): force the 256x192 loader-wave tile with the remainder tiles cut S ways along K (tests, A/B runs)"""
    return int(S) << 16


class VclozeHipError(RuntimeError):
    pass


class GemmProblem(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("C", C.c_void_p),
        ("res", C.c_void_p), ("gate", C.c_void_p),
        ("lda", C.c_int64), ("ldw", C.c_int64), ("ldc", C.c_int64), ("ldres", C.c_int64), ("gate_bstride", C.c_int64),
        ("a_bstride", C.c_int64), ("c_bstride", C.c_int64),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("rows_per_batch", C.c_int32),
        ("a_rpb", C.c_int32), ("c_rpb", C.c_int32),
        ("tiles_m", C.c_int32), ("tiles_n", C.c_int32), ("tile_start", C.c_int32), ("m_begin", C.c_int32),
        ("vt", C.c_void_p), ("vt_bstride", C.c_int64),
        ("vt_col0", C.c_int32), ("vt_rpb", C.c_int32), ("vt_row0", C.c_int32), ("vt_lpad", C.c_int32),
        ("kn_scale", C.c_void_p), ("kn_rope", C.c_void_p), ("kn_rope_bstride", C.c_int64), ("kn_heads", C.c_int32), ("qn_prescale", C.c_int32),
        ("qn_scale", C.c_void_p),
        ("a_zstride", C.c_int64), ("w_zstride", C.c_int64), ("c_zstride", C.c_int64),
    ]


class GemmArgs(C.Structure):
    _fields_ = [
        ("p", GemmProblem * 4), ("nprob", C.c_int32), ("epi", C.c_int32),
        ("step_ptr", C.c_void_p), ("gate_step_stride", C.c_int64), ("debug_ts", C.c_void_p),
        ("splitk_ws", C.c_void_p), ("splitk_ws_bytes", C.c_int64),
        ("sk_full", C.c_int32), ("sk_rem", C.c_int32), ("sk_S", C.c_int32), ("batch", C.c_int32),
        ("sk_stream", C.c_int32), ("sk_pad_", C.c_int32),
    ]


class LnStream(C.Structure):
    """VcLnStream of include/vcloze_hip.h."""
    _fields_ = [("x", C.c_void_p), ("ldx", C.c_int64), ("y", C.c_void_p), ("ldy", C.c_int64), ("shift", C.c_void_p),
                ("scale", C.c_void_p), ("rows", C.c_int32), ("rows_per_batch", C.c_int32)]


class Attention(C.Structure):
    """VcAttention of include/vcloze_hip.h."""
    _fields_ = [("qkv", C.c_void_p), ("ld", C.c_int64), ("bstride", C.c_int64), ("vt", C.c_void_p), ("out", C.c_void_p),
                ("ldo", C.c_int64), ("out_bstride", C.c_int64), ("kv_len", C.c_void_p),
                ("B", C.c_int32), ("L", C.c_int32), ("Lpad", C.c_int32), ("H", C.c_int32), ("variant", C.c_int32), ("split", C.c_int32),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64),
                ("q_scale", C.c_void_p), ("q_scale2", C.c_void_p), ("rope", C.c_void_p), ("rope_bstride", C.c_int64),
                ("kv_gap", C.c_void_p), ("logit_bound", C.c_float), ("q_prescaled", C.c_int32)]


class FluxConfig(C.Structure):
    """VcFluxConfig of include/vcloze_hip.h."""
    _fields_ = [("in_channels", C.c_int32), ("out_channels", C.c_int32), ("vec_in_dim", C.c_int32), ("context_in_dim", C.c_int32),
                ("hidden_size", C.c_int32), ("num_heads", C.c_int32), ("depth", C.c_int32), ("depth_single_blocks", C.c_int32),
                ("mlp_hidden", C.c_int32), ("guidance_embed", C.c_int32), ("axes_dim", C.c_int32 * 3), ("theta", C.c_int32)]


class FluxInputs(C.Structure):
    """VcFluxInputs of include/vcloze_hip.h (txt / y device pointers, everything else host arrays)."""
    _fields_ = [("B", C.c_int32), ("T", C.c_int32), ("N", C.c_int32), ("max_steps", C.c_int32),
                ("txt", C.c_void_p), ("y", C.c_void_p), ("guidance", C.POINTER(C.c_float)), ("img_ids", C.POINTER(C.c_float)),
                ("txt_ids", C.POINTER(C.c_float)), ("kv_len", C.POINTER(C.c_int32)), ("kv_gap", C.POINTER(C.c_int32)),
                ("guidance_is_bf16", C.c_int32), ("_pad", C.c_int32)]


class VaeConfig(C.Structure):
    """VcVaeConfig of include/vcloze_hip.h."""
    _fields_ = [("in_channels", C.c_int32), ("ch", C.c_int32), ("out_ch", C.c_int32), ("ch_mult", C.c_int32 * 8), ("n_ch_mult", C.c_int32),
                ("num_res_blocks", C.c_int32), ("z_channels", C.c_int32), ("scale_factor", C.c_float), ("shift_factor", C.c_float)]


VAE_ENCODER, VAE_DECODER = 1, 2                             # VC_VAE_ENCODER / VC_VAE_DECODER (`which` of vc_vae_prepare)
VAE_LATENT_BF16, VAE_LATENT_F32, VAE_TOKENS = 0, 1, 2       # VC_VAE_LATENT_* / VC_VAE_TOKENS (latent_form)


class TextConfig(C.Structure):
    """VcTextConfig of include/vcloze_hip.h."""
    _fields_ = [("kind", C.c_int32), ("vocab_size", C.c_int32), ("d_model", C.c_int32), ("d_kv", C.c_int32), ("d_ff", C.c_int32),
                ("num_layers", C.c_int32), ("num_heads", C.c_int32), ("num_buckets", C.c_int32), ("max_distance", C.c_int32),
                ("max_positions", C.c_int32), ("eos_token_id", C.c_int32), ("eps", C.c_float)]


TEXT_T5, TEXT_CLIP = 1, 2                                   # VC_TEXT_T5 / VC_TEXT_CLIP (VcTextConfig.kind)

GRID_MAX_ROWS, GRID_SDEDIT_CHUNK = 16, 4                    # VC_GRID_MAX_ROWS / VC_GRID_SDEDIT_CHUNK
PIXELS_F32, PIXELS_U8 = 0, 1                                # VC_PIXELS_* (out_form of vc_pixels_out and of the grid jobs)


class GridConfig(C.Structure):
    """VcGridConfig of include/vcloze_hip.h: the four borrowed sub-handles."""
    _fields_ = [("flux", C.c_void_p), ("vae", C.c_void_p), ("t5", C.c_void_p), ("clip", C.c_void_p)]


class GridJob(C.Structure):
    """VcGridJob of include/vcloze_hip.h."""
    _fields_ = [("rows", C.c_int32), ("pixels_is_f32", C.c_int32), ("height", C.c_int32 * GRID_MAX_ROWS), ("width", C.c_int32 * GRID_MAX_ROWS),
                ("pixels", C.c_void_p * GRID_MAX_ROWS), ("masks", C.c_void_p * GRID_MAX_ROWS), ("decode", C.c_int32 * GRID_MAX_ROWS),
                ("t5_ids", C.POINTER(C.c_int32)), ("clip_ids", C.POINTER(C.c_int32)), ("t5_len", C.c_int32), ("clip_len", C.c_int32),
                ("seed", C.c_uint64), ("noise_offset", C.c_uint64), ("noise_offset_out", C.POINTER(C.c_uint64)),
                ("guidance", C.c_float), ("n_points", C.c_int32), ("method", C.c_int32), ("out_form", C.c_int32), ("max_evals", C.c_int32),
                ("_pad", C.c_int32), ("time_shifting_factor", C.c_double)]


class GridSdedit(C.Structure):
    """VcGridSdedit of include/vcloze_hip.h."""
    _fields_ = [("count", C.c_int32), ("pixels_is_f32", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("pixels", C.c_void_p * GRID_MAX_ROWS), ("t5_ids", C.POINTER(C.c_int32)), ("clip_ids", C.POINTER(C.c_int32)),
                ("t5_len", C.c_int32), ("clip_len", C.c_int32), ("seed", C.c_uint64), ("noise_offset", C.c_uint64),
                ("noise_offset_out", C.POINTER(C.c_uint64)), ("guidance", C.c_float), ("n_points", C.c_int32), ("method", C.c_int32),
                ("out_form", C.c_int32), ("max_evals", C.c_int32), ("_pad", C.c_int32), ("strength", C.c_double)]


FILTER_BICUBIC, FILTER_LANCZOS = 0, 1                       # VC_FILTER_* (vc_resample_u8)
FILTERS = {"bicubic": FILTER_BICUBIC, "lanczos": FILTER_LANCZOS}


class CellPlan(C.Structure):
    """VcCellPlan of include/vcloze_hip.h: what vc_grid_layout says about one cell."""
    _fields_ = [(n, C.c_int32) for n in ("present", "fit_w", "fit_h", "cover_w", "cover_h", "crop_left", "crop_top", "cell_w", "cell_h",
                                         "final_w", "final_h", "mask")]


class GridPhotos(C.Structure):
    """VcGridPhotos of include/vcloze_hip.h."""
    _fields_ = [("grid_h", C.c_int32), ("grid_w", C.c_int32), ("resolution", C.c_int32), ("out_form", C.c_int32),
                ("images", C.POINTER(C.c_void_p)), ("width", C.POINTER(C.c_int32)), ("height", C.POINTER(C.c_int32)),
                ("decode", C.c_int32 * GRID_MAX_ROWS), ("t5_ids", C.POINTER(C.c_int32)), ("clip_ids", C.POINTER(C.c_int32)),
                ("t5_len", C.c_int32), ("clip_len", C.c_int32), ("seed", C.c_uint64), ("noise_offset", C.c_uint64),
                ("noise_offset_out", C.POINTER(C.c_uint64)), ("guidance", C.c_float), ("n_points", C.c_int32), ("method", C.c_int32),
                ("max_evals", C.c_int32), ("time_shifting_factor", C.c_double)]


class GridSdeditU8(C.Structure):
    """VcGridSdeditU8 of include/vcloze_hip.h."""
    _fields_ = [("count", C.c_int32), ("cell_h", C.c_int32), ("cell_w", C.c_int32), ("height", C.c_int32), ("width", C.c_int32),
                ("out_form", C.c_int32), ("pixels", C.c_void_p * GRID_MAX_ROWS), ("t5_ids", C.POINTER(C.c_int32)),
                ("clip_ids", C.POINTER(C.c_int32)), ("t5_len", C.c_int32), ("clip_len", C.c_int32), ("seed", C.c_uint64),
                ("noise_offset", C.c_uint64), ("noise_offset_out", C.POINTER(C.c_uint64)), ("guidance", C.c_float), ("n_points", C.c_int32),
                ("method", C.c_int32), ("max_evals", C.c_int32), ("strength", C.c_double)]


# every symbol include/vcloze_hip.h declares: name -> (restype, argtypes)
_vp, _i32, _i64 = C.c_void_p, C.c_int32, C.c_int64
class FluxLaunchClass(C.Structure):          # VcFluxLaunchClass (vc_flux_profile)
    _fields_ = [("kind", C.c_int32), ("epi", C.c_int32), ("n", C.c_int32), ("k", C.c_int32), ("launches", C.c_int32), ("reserved", C.c_int32),
                ("flops", C.c_double), ("bytes", C.c_double), ("total_us", C.c_float), ("min_us", C.c_float), ("max_us", C.c_float),
                ("reserved2", C.c_float)]


LAUNCH_GEMM, LAUNCH_ATTENTION, LAUNCH_LN_MODULATE, LAUNCH_PASS, LAUNCH_TAP = 1, 2, 3, 4, 5


class Stat(C.Structure):                     # VcStat (vc_tensor_stats, vc_flux_set_monitor)
    _fields_ = [("max_abs", C.c_float), ("sum_sq", C.c_float), ("nonfinite", C.c_uint32), ("count", C.c_uint32)]


MONITOR_MAX_BLOCKS = 256                     # VC_MONITOR_MAX_BLOCKS


class ImageMetrics(C.Structure):             # VcImageMetrics (vc_image_compare)
    _fields_ = [("n", C.c_uint64), ("n_windows", C.c_uint64), ("sse_u64", C.c_uint64), ("n_diff", C.c_uint64), ("sse_f32", C.c_float),
                ("max_abs", C.c_float), ("ssim_mean", C.c_float), ("form", C.c_int32)]


IMG_U8_HWC, IMG_F32_CHW = 0, 1               # VC_IMG_*: the storage of both operands of vc_image_compare
IMG_TILE, IMG_RECORD_BYTES = 32, 32          # VC_IMG_TILE / VC_IMG_RECORD_BYTES

SYMBOLS = {
    "vc_abi_version": (C.c_int, []),
    "vc_last_error": (C.c_char_p, []),
    "vc_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_device_count": (C.c_int, []),
    "vc_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int64)]),
    "vc_gemm": (C.c_int, [C.POINTER(GemmArgs), C.c_int, _vp]),
    "vc_gemm_plan": (C.c_int, [C.POINTER(GemmArgs), C.c_int, C.POINTER(C.c_int32)]),
    "vc_ln_modulate": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "vc_ln_modulate2": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "vc_qknorm_rope_vt": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vc_attention": (C.c_int, [C.POINTER(Attention), _vp]),
    "vc_attention_scratch_bytes": (_i64, []),
    "vc_attention_plan": (C.c_int, [C.POINTER(Attention), _i32, C.POINTER(C.c_int32)]),
    "vc_timestep_embedding": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "vc_silu": (C.c_int, [_vp, _vp, _i64, _vp]),
    "vc_act2d": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp]),
    "vc_gate_residual": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _vp]),
    "vc_add3": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp]),
    "vc_copy": (C.c_int, [_vp, _vp, _i64, _vp]),
    "vc_concat_cols": (C.c_int, [_vp, _i32, _vp, _i32, _vp, _i64, _vp]),
    "vc_euler_step": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_euler_step_f32": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_step_advance": (C.c_int, [_vp, _vp]),
    "vc_solver_evals": (C.c_int, [C.c_int]),
    "vc_ode_stage": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_dopri5_stage": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_dopri5_error_ratio": (C.c_int, [_i32, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _i64, _vp]),
    "vc_dopri5_interp": (C.c_int, [_vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _i64, _vp]),
    "vc_rk_evals": (C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_rk_stage": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_rk_error_ratio": (C.c_int, [_i32, _i32, _vp, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp, _i64, _vp]),
    "vc_rk_interp": (C.c_int, [_i32, _vp, _vp, _vp, _vp, C.c_float, _vp, _i32, _i64, _vp]),
    "vc_sde_plan": (C.c_int, [C.c_char_p, C.c_char_p, C.c_double, C.c_char_p, C.c_double, C.POINTER(C.c_float), _i32, C.POINTER(C.c_float),
                              C.POINTER(C.c_float), _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_sde_stage": (C.c_int, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_ms_plan": (C.c_int, [_i32, C.POINTER(C.c_float), _i32, C.POINTER(C.c_float), C.POINTER(C.c_float), _i32, C.POINTER(_i32)]),
    "vc_ms_stage": (C.c_int, [_i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "vc_residual_change": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _vp]),
    "vc_residual_sub": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _vp]),
    "vc_residual_add": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _i64, _vp]),
    "vc_cfg_combine": (C.c_int, [_vp, _vp, _vp, _i64, C.c_float, _vp]),
    "vc_monitor_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_tensor_stats": (C.c_int, [_vp, _i32, _i64, _i64, _i32, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp]),
    "vc_fm_plan": (C.c_int, [_vp, _i32, _i64, _i64, _vp, _vp, C.c_uint64, C.c_uint64, _vp, _i64, _vp, _i32, _i64, _i32, _vp]),
    "vc_fm_loss": (C.c_int, [_vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _i64, _i32, _vp]),
    "vc_fm_times": (C.c_int, [C.c_char_p, C.POINTER(C.c_float), _i32, _i32, _i32, C.POINTER(C.c_float)]),
    "vc_sdedit_mix": (C.c_int, [_vp, _vp, C.c_double, _vp, _i64, _vp]),
    "vc_pack_latent": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i32, _vp]),
    "vc_pack_mask": (C.c_int, [_vp, _vp, _i32, _i32, _i64, _i32, _vp]),
    "vc_unpack_latent": (C.c_int, [_vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp]),
    "vc_im2col3x3": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "vc_conv3x3": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vc_groupnorm": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, C.c_float, _i32, _vp]),
    "vc_softmax_rows": (C.c_int, [_vp, _i64, _i32, _i32, C.c_float, _vp, _i64, _i32, _vp]),
    "vc_embedding": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp]),
    "vc_rmsnorm": (C.c_int, [_vp, _vp, _vp, _i32, _i32, C.c_float, _vp]),
    "vc_layernorm": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, C.c_float, _vp]),
    "vc_mul": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "vc_add": (C.c_int, [_vp, _vp, _vp, _i64, _vp]),
    "vc_quick_gelu": (C.c_int, [_vp, _vp, _i64, _vp]),
    "vc_t5_relative_buckets": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32)]),
    "vc_t5_position_bias": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vc_clip_embed": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _vp]),
    "vc_clip_pool": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp]),
    "vc_transpose": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "vc_nchw_to_nhwc": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i64, C.c_float, C.c_float, _vp]),
    "vc_nhwc_to_nchw": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _vp]),
    "vc_gaussian_sample": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i64, C.c_float, C.c_float, _vp]),
    "vc_randn": (C.c_int, [_vp, _i32, _i64, C.c_uint64, C.c_uint64, _vp]),
    "vc_randn_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i32, C.c_uint64, C.c_uint64, _vp]),
    "vc_torch_randn_policy": (C.c_int, [_i64, _i32, _i32, C.POINTER(_i32), C.POINTER(C.c_uint64)]),
    "vc_randn_torch": (C.c_int, [_vp, _i32, _i64, C.c_uint64, C.c_uint64, _i32, _i32, _vp]),
    "vc_randn_torch_tokens": (C.c_int, [_vp, _i32, _i32, _i32, _i64, _i32, C.c_uint64, C.c_uint64, _i32, _i32, _vp]),
    "vc_lora_merge": (C.c_int, [_vp, _i32, _i64, _vp, _i64, _vp, _i64, C.c_float, _vp, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp]),
    "vc_lora_merge_qkv": (C.c_int, [_vp, _i32, _i64, _vp, _i64, _vp, _i64, C.c_float, _vp, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32,
                                    _vp]),
    "vc_flux_create": (C.c_int, [C.POINTER(FluxConfig), C.POINTER(_vp)]),
    "vc_flux_destroy": (C.c_int, [_vp]),
    "vc_flux_bind_weight": (C.c_int, [_vp, C.c_char_p, _vp, _vp, _i32, _i32, _i64]),
    "vc_flux_bind_lora": (C.c_int, [_vp, C.c_char_p, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32]),
    "vc_flux_set_lora_scale": (C.c_int, [_vp, C.c_float]),
    "vc_flux_load_key": (C.c_int, [_vp, _i32, C.c_char_p, _i32, C.POINTER(_i64), C.POINTER(_i32)]),
    "vc_flux_load_tensor": (C.c_int, [_vp, C.c_char_p, _vp, _i32, C.POINTER(_i64), _i32]),
    "vc_flux_load_bytes": (_i64, [_vp]),
    "vc_flux_load_finish": (C.c_int, [_vp, C.c_float, _vp, _i64, _vp]),
    "vc_flux_bound": (C.c_int, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i64)]),
    "vc_flux_set_tap": (C.c_int, [_vp, C.c_char_p, _vp]),
    "vc_flux_tap_shape": (C.c_int, [_vp, C.c_char_p, C.POINTER(_i64), C.POINTER(_i32)]),
    "vc_flux_mod_offset": (_i64, [_vp, C.c_char_p]),
    "vc_flux_set_option": (C.c_int, [_vp, C.c_char_p, _i32]),
    "vc_flux_workspace_bytes": (_i64, [_vp, _i32, _i32, _i32, _i32]),
    "vc_flux_prepare": (C.c_int, [_vp, C.POINTER(FluxInputs), _vp, _i64, _vp]),
    "vc_flux_forward": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), _i32, _vp, _vp]),
    "vc_flux_eval_loss": (C.c_int, [_vp, _vp, _i32, _vp, C.POINTER(C.c_float), _vp, C.c_uint64, C.c_uint64, _vp, _vp]),
    "vc_flux_sample_euler": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, _vp, _vp]),
    "vc_flux_sample_begin": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, _vp]),
    "vc_flux_sample_steps": (C.c_int, [_vp, _i32, _vp, _vp]),
    "vc_flux_sample_end": (C.c_int, [_vp, _vp, _vp]),
    "vc_flux_sample_ode": (C.c_int, [_vp, _i32, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, _vp, _vp]),
    "vc_flux_sample_begin_ode": (C.c_int, [_vp, _i32, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, _vp]),
    "vc_flux_sample_dopri5": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, C.c_float, C.c_float, _i32, _vp, _vp]),
    "vc_flux_dopri5_log": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(_i32), _i32,
                                     C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_flux_sample_rk": (C.c_int, [_vp, _i32, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, C.c_float, C.c_float, _i32, _vp, _vp]),
    "vc_flux_rk_log": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(_i32), _i32,
                                 C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_flux_sample_sde": (C.c_int, [_vp, C.c_char_p, _vp, _vp, C.POINTER(C.c_float), _i32, C.c_char_p, C.c_double, C.c_char_p, C.c_double,
                                     C.c_uint64, C.c_uint64, _i32, _vp, _vp]),
    "vc_flux_sample_multistep": (C.c_int, [_vp, _i32, _vp, _vp, C.POINTER(C.c_float), _i32, _i32, _vp, _vp]),
    "vc_flux_plan_count": (C.c_int, [_vp]),
    "vc_flux_set_step_cache": (C.c_int, [_vp, C.c_float, _i32]),
    "vc_flux_set_cfg": (C.c_int, [_vp, _i32, C.c_float]),
    "vc_flux_step_cache_stats": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_float), _i32]),
    "vc_flux_profile": (C.c_int, [_vp, _i32, C.POINTER(FluxLaunchClass), _i32, C.POINTER(_i32), _vp]),
    "vc_flux_step_nodes": (C.c_int, [_vp, C.POINTER(_i32)]),
    "vc_flux_set_monitor": (C.c_int, [_vp, _i32, _vp, _i32, _vp]),
    "vc_flux_monitor_sites": (C.c_int, [_vp, _i32, C.c_char_p, _i32]),
    "vc_flux_monitor_bytes": (C.c_int, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "vc_flux_monitor_report": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _vp]),
    "vc_vae_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_vae_create": (C.c_int, [C.POINTER(VaeConfig), C.POINTER(_vp)]),
    "vc_vae_destroy": (C.c_int, [_vp]),
    "vc_vae_weight_name": (C.c_int, [_vp, _i32, C.c_char_p, _i32]),
    "vc_vae_bind_weight": (C.c_int, [_vp, C.c_char_p, _vp, _vp, _i32, C.POINTER(_i64), _i32, _vp]),
    "vc_vae_workspace_bytes": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_i64)]),
    "vc_vae_prepare": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    "vc_vae_decode": (C.c_int, [_vp, _vp, _i32, _i64, _i32, _vp, _i32, _vp]),
    "vc_vae_encode": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _i32, _i64, _i32, _vp]),
    "vc_vae_plan_count": (C.c_int, [_vp]),
    "vc_text_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_text_create": (C.c_int, [C.POINTER(TextConfig), C.POINTER(_vp)]),
    "vc_text_destroy": (C.c_int, [_vp]),
    "vc_text_weight_name": (C.c_int, [_vp, _i32, C.c_char_p, _i32]),
    "vc_text_bind_tensor": (C.c_int, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i32]),
    "vc_text_workspace_bytes": (C.c_int, [_vp, _i32, C.POINTER(_i64)]),
    "vc_text_prepare": (C.c_int, [_vp, _i32, _vp, _i64, _vp]),
    "vc_text_encode": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "vc_text_plan_count": (C.c_int, [_vp]),
    "vc_time_grid": (C.c_int, [_i32, _i32, C.c_double, C.c_double, _i32, C.c_double, C.POINTER(C.c_float)]),
    "vc_grid_tokens": (_i64, [_i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_grid_img_ids": (C.c_int, [_i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(C.c_float)]),
    "vc_pixels_out": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "vc_image_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_image_compare_scratch_bytes": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "vc_image_compare": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp]),
    "vc_image_psnr": (C.c_int, [C.POINTER(ImageMetrics), C.POINTER(C.c_double)]),
    "vc_grid_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_grid_create": (C.c_int, [C.POINTER(GridConfig), C.POINTER(_vp)]),
    "vc_grid_destroy": (C.c_int, [_vp]),
    "vc_grid_set_noise": (C.c_int, [_vp, _i32, _i32, _i32]),
    "vc_grid_workspace_bytes": (C.c_int, [_vp, C.POINTER(GridJob), C.POINTER(_i64)]),
    "vc_grid_sdedit_workspace_bytes": (C.c_int, [_vp, C.POINTER(GridSdedit), C.POINTER(_i64)]),
    "vc_grid_generate": (C.c_int, [_vp, C.POINTER(GridJob), _vp, _i64, C.POINTER(_vp), _vp]),
    "vc_grid_sdedit": (C.c_int, [_vp, C.POINTER(GridSdedit), _vp, _i64, C.POINTER(_vp), _vp]),
    "vc_resample_kmax": (C.c_int, [_i32, _i32, _i32]),
    "vc_resample_coeffs": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), _i32]),
    "vc_resample_tmp_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "vc_resample_u8": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _i64, _vp]),
    "vc_pixels_in": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vc_mask_fill": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "vc_fit_size": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_grid_layout": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32), _i32, C.POINTER(CellPlan)]),
    "vc_upsampling_size": (C.c_int, [_i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "vc_photo_struct_sizes": (None, [C.POINTER(C.c_int32)]),
    "vc_grid_photos_workspace_bytes": (C.c_int, [_vp, C.POINTER(GridPhotos), C.POINTER(_i64)]),
    "vc_grid_sdedit_u8_workspace_bytes": (C.c_int, [_vp, C.POINTER(GridSdeditU8), C.POINTER(_i64)]),
    "vc_grid_generate_photos": (C.c_int, [_vp, C.POINTER(GridPhotos), _vp, _i64, C.POINTER(_vp), _vp]),
    "vc_grid_sdedit_u8": (C.c_int, [_vp, C.POINTER(GridSdeditU8), _vp, _i64, C.POINTER(_vp), _vp]),
    "vc_stream_create": (C.c_int, [C.POINTER(_vp)]),
    "vc_stream_destroy": (C.c_int, [_vp]),
    "vc_stream_sync": (C.c_int, [_vp]),
    "vc_graph_begin": (C.c_int, [_vp]),
    "vc_graph_end": (C.c_int, [_vp, C.POINTER(_vp)]),
    "vc_graph_launch": (C.c_int, [_vp, _vp]),
    "vc_graph_destroy": (C.c_int, [_vp]),
    "vc_event_create": (C.c_int, [C.POINTER(_vp)]),
    "vc_event_record": (C.c_int, [_vp, _vp]),
    "vc_event_elapsed_ms": (C.c_int, [_vp, _vp, C.POINTER(C.c_float)]),
    "vc_event_destroy": (C.c_int, [_vp]),
}

_lib = None


def build(force: bool = False) -> str:
    """Compile csrc/*.hip for gfx950 into lib/libvcloze_hip.so (hipcc cross-compiles without a GPU).  `make` is
    incremental and knows every dependency (the ABI header include/vcloze_hip.h included), so it is simply run."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], capture_output=True, text=True)
    r = subprocess.run(["make", "-C", CSRC, "-j8"], capture_output=True, text=True)
    if r.returncode != 0:
        raise VclozeHipError("building libvcloze_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VclozeHipError(
                f"{LIB_PATH} is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(the HIP extension is mandatory; there is no CPU fallback)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(l, name)  # AttributeError if the ABI lost a symbol
            fn.restype, fn.argtypes = res, args
        if l.vc_abi_version() != ABI_VERSION:
            raise VclozeHipError(f"libvcloze_hip.so ABI version {l.vc_abi_version()} != {ABI_VERSION} expected by hip.py - rebuild")
        sizes = (C.c_int32 * 7)()
        l.vc_struct_sizes(sizes)          # a stale library whose structs disagree with these ctypes mirrors must not run
        if list(sizes) != [C.sizeof(GemmProblem), C.sizeof(GemmArgs), C.sizeof(LnStream), C.sizeof(Attention),
                           C.sizeof(FluxConfig), C.sizeof(FluxInputs), C.sizeof(FluxLaunchClass)]:
            raise VclozeHipError(f"libvcloze_hip.so struct sizes {list(sizes)} differ from the ctypes mirrors - rebuild")
        vsize = (C.c_int32 * 1)()
        l.vc_vae_struct_sizes(vsize)
        if vsize[0] != C.sizeof(VaeConfig):
            raise VclozeHipError(f"libvcloze_hip.so sizeof(VcVaeConfig) {vsize[0]} differs from the ctypes mirror - rebuild")
        l.vc_text_struct_sizes(vsize)
        if vsize[0] != C.sizeof(TextConfig):
            raise VclozeHipError(f"libvcloze_hip.so sizeof(VcTextConfig) {vsize[0]} differs from the ctypes mirror - rebuild")
        l.vc_monitor_struct_sizes(vsize)
        if vsize[0] != C.sizeof(Stat):
            raise VclozeHipError(f"libvcloze_hip.so sizeof(VcStat) {vsize[0]} differs from the ctypes mirror - rebuild")
        l.vc_image_struct_sizes(vsize)
        if vsize[0] != C.sizeof(ImageMetrics):
            raise VclozeHipError(f"libvcloze_hip.so sizeof(VcImageMetrics) {vsize[0]} differs from the ctypes mirror - rebuild")
        gsize = (C.c_int32 * 3)()
        l.vc_grid_struct_sizes(gsize)
        if list(gsize) != [C.sizeof(GridConfig), C.sizeof(GridJob), C.sizeof(GridSdedit)]:
            raise VclozeHipError(f"libvcloze_hip.so grid struct sizes {list(gsize)} differ from the ctypes mirrors - rebuild")
        l.vc_photo_struct_sizes(gsize)
        if list(gsize) != [C.sizeof(CellPlan), C.sizeof(GridPhotos), C.sizeof(GridSdeditU8)]:
            raise VclozeHipError(f"libvcloze_hip.so photo struct sizes {list(gsize)} differ from the ctypes mirrors - rebuild")
        _lib = l
    return _lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        raise VclozeHipError(f"{what} failed ({rc}): {lib().vc_last_error().decode()}")


def require_gpu() -> None:
    if lib().vc_device_count() < 1:
        raise VclozeHipError("no ROCm device visible: " + lib().vc_last_error().decode())


def device_cus(device=None) -> int:
    """compute units of the device (256 on MI355X)"""
    idx = torch.device(device).index if device is not None else torch.cuda.current_device()
    n = C.c_int()
    _check(lib().vc_device_info(idx or 0, None, 0, C.byref(n), None), "vc_device_info")
    return n.value


def cur_stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _bf16(t: torch.Tensor, name: str) -> None:
    if t.dtype != torch.bfloat16 or not t.is_cuda:
        raise VclozeHipError(f"{name}: expected a CUDA bf16 tensor, got {t.dtype} on {t.device}")


# ------------------------------------------------------------------------------------------------
# op wrappers (2-D row-major views; the last dim must be contiguous)
# ------------------------------------------------------------------------------------------------
def qkv_head_permutation(H: int) -> torch.Tensor:
    """Row order of a HEAD-PERMUTED qkv weight [3 * 128 * H, K] (VcGemmProblem.kn_heads): 2H blocks of 192 rows = [head t (128
    rows: query head t for t < H, key head t - H after) | V rows 64 t .. 64 t + 63] - every 192-column GEMM tile then holds one
    whole query or key head (QKNorm + RoPE in its epilogue) and half a value head.  perm[p] = the original row."""
    D = 128 * H
    idx = []
    for t in range(2 * H):
        idx += list(range(128 * t, 128 * t + 128)) + list(range(2 * D + 64 * t, 2 * D + 64 * t + 64))
    return torch.tensor(idx, dtype=torch.long)


def make_problem(a, w, bias, out, res=None, gate=None, rows_per_batch=None, gate_bstride=0, M=None,
                 a_rpb=0, a_bstride=0, c_rpb=0, c_bstride=0, vt=None, vt_col0=0, vt_rpb=0, vt_row0=0,
                 kn_heads=0, kn_scale=None, kn_rope=None, qn_scale=None, qn_prescale=False) -> GemmProblem:
    """`M` + (a_rpb, a_bstride) / (c_rpb, c_bstride) describe batch-strided rows: `a` / `out` are then views of the
    FIRST batch element's rows (row m of the problem lives at (m // rpb) * bstride + (m % rpb) * ld).
    EPI_QKV: `vt` [B, H, 128, Lpad] receives the columns >= vt_col0 transposed; this problem's rows are tokens
    vt_row0 .. vt_row0 + vt_rpb of each batch element's joint sequence."""
    for n, t in (("A", a), ("W", w), ("C", out)):
        _bf16(t, n)
        if t.dim() != 2 or t.stride(1) != 1:
            raise VclozeHipError(f"gemm {n}: need a 2-D tensor with contiguous last dim")
    K = a.shape[1]
    N = w.shape[0]
    if M is None:
        M = a.shape[0]
        if tuple(out.shape) != (M, N):
            raise VclozeHipError(f"gemm shape mismatch A{tuple(a.shape)} W{tuple(w.shape)} C{tuple(out.shape)}")
    if w.shape[1] != K or out.shape[1] != N:
        raise VclozeHipError(f"gemm shape mismatch A{tuple(a.shape)} W{tuple(w.shape)} C{tuple(out.shape)}")
    p = GemmProblem()
    p.A, p.W, p.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    p.bias = _p(bias)
    p.lda, p.ldw, p.ldc = a.stride(0), w.stride(0), out.stride(0)
    p.M, p.N, p.K = M, N, K
    p.rows_per_batch = rows_per_batch or M
    p.a_rpb, p.a_bstride, p.c_rpb, p.c_bstride = a_rpb, a_bstride, c_rpb, c_bstride
    if res is not None:
        _bf16(res, "res")
        p.res, p.ldres = res.data_ptr(), res.stride(0)
    if gate is not None:
        _bf16(gate, "gate")
        p.gate, p.gate_bstride = gate.data_ptr(), gate_bstride
    if vt is not None:
        _bf16(vt, "vt")
        if vt.dim() != 4 or not vt.is_contiguous():
            raise VclozeHipError("gemm vt: contiguous [B, H, 128, Lpad] expected")
        p.vt, p.vt_bstride, p.vt_lpad = vt.data_ptr(), vt.stride(0), vt.shape[-1]
        p.vt_col0, p.vt_rpb, p.vt_row0 = vt_col0, vt_rpb or M, vt_row0
    if kn_heads:
        p.kn_heads = kn_heads        # w / bias are head-permuted (qkv_head_permutation); C receives the logical columns
        if vt is None:
            p.vt_rpb, p.vt_row0 = vt_rpb or M, vt_row0
        if kn_scale is not None or qn_scale is not None:     # ... and QKNorm + RoPE of the key / query heads happen in the epilogue
            if kn_rope is None or kn_rope.dtype != torch.float32 or not kn_rope.is_contiguous():
                raise VclozeHipError("gemm kn_rope: contiguous f32 [B?, L, 64, 2] expected")
            p.kn_rope = kn_rope.data_ptr()
            p.kn_rope_bstride = kn_rope.shape[-3] * 128 if kn_rope.dim() == 4 else 0
            if kn_scale is not None:
                _bf16(kn_scale, "kn_scale")
                p.kn_scale = kn_scale.data_ptr()
            if qn_scale is not None:     # qn_prescale: the queries leave times 128^-0.5 * log2(e) (attention(q_prescaled=True))
                _bf16(qn_scale, "qn_scale")
                p.qn_scale, p.qn_prescale = qn_scale.data_ptr(), int(bool(qn_prescale))
    p._keep = (a, w, bias, out, res, gate, vt, kn_scale, kn_rope, qn_scale)   # the struct carries raw pointers: keep the operands alive with it
    return p


def splitk_workspace(device) -> torch.Tensor:
    """f32 scratch for the split-K remainder of vc_gemm (VcGemmArgs.splitk_ws): two 256x192 partial tiles per CU of one round"""
    return torch.empty(GEMM_SPLITK_WS_BYTES, dtype=torch.uint8, device=device)


def gemm(problems, epi=EPI_BIAS, tile_cfg=0, step_ptr=None, gate_step_stride=0, stream=None, debug_ts=None, splitk_ws=None,
         batch=0) -> None:
    """`batch` = Z > 1: Z independent GEMMs per problem in one launch; set the problem's a_zstride / w_zstride / c_zstride."""
    args = GemmArgs()
    args.batch = batch
    if splitk_ws is not None:
        args.splitk_ws, args.splitk_ws_bytes = splitk_ws.data_ptr(), splitk_ws.numel() * splitk_ws.element_size()
    if isinstance(problems, GemmProblem):
        problems = [problems]
    args.nprob = len(problems)
    for i, p in enumerate(problems):
        args.p[i] = p
    args.epi = epi
    args.step_ptr = _p(step_ptr)
    args.gate_step_stride = gate_step_stride
    args.debug_ts = _p(debug_ts)
    _check(lib().vc_gemm(C.byref(args), tile_cfg, stream if stream is not None else cur_stream()), "vc_gemm")


def linear(a, w, bias=None, out=None, epi=EPI_BIAS, res=None, gate=None, tile_cfg=0, stream=None):
    if out is None:
        out = torch.empty(a.shape[0], w.shape[0], dtype=torch.bfloat16, device=a.device)
    gemm(make_problem(a, w, bias, out, res=res, gate=gate), epi=epi, tile_cfg=tile_cfg, stream=stream)
    return out


def lora_merge(weight, lora_a, lora_b, scale, out=None, bias=None, lora_b_bias=None, stream=None, qkv_heads=0):
    """(W', b') = (bf16(W + scale * B @ A), bf16(b + scale * b_B)): LinearLora (models/modules/lora.py:92-98) folded into one
    weight by vc_lora_merge.  `weight` [out, in] and `bias` [out]: bf16 or f32; `lora_a` [r, in], `lora_b` [out, r],
    `lora_b_bias` [out]: bf16 (f32 factors are not bf16 values - the matrix cores would round them - and are refused); both
    factors None = rank 0, a conversion of `weight` / `bias`.  `out`: a [out, in] bf16 view with any row stride (rows of a
    stacked matrix), `weight` itself (bf16: merged in place) or None (a new tensor).  Returns (out, bias_out or None).
    `qkv_heads` H > 0 (vc_lora_merge_qkv): the rows [0, 3 * 128 * H) of the result and of the bias are stored head-permuted, i.e.
    `merged[:3 * 128 * H][qkv_head_permutation(H)]`; `out` must then not be `weight`."""
    if weight.dim() != 2 or not weight.is_cuda or weight.dtype not in (torch.bfloat16, torch.float32) or weight.stride(1) != 1:
        raise VclozeHipError(f"lora_merge weight: need a 2-D CUDA bf16 / f32 tensor with contiguous last dim, got {weight.dtype} "
                             f"{tuple(weight.shape)} on {weight.device}")
    O, I = weight.shape
    for n, t in (("lora_a", lora_a), ("lora_b", lora_b), ("out", out), ("bias", bias), ("lora_b_bias", lora_b_bias)):
        if t is not None and t.device != weight.device:
            raise VclozeHipError(f"lora_merge {n}: on device {t.device}, the weight is on {weight.device}")
    if stream is None and weight.device.index != torch.cuda.current_device():
        raise VclozeHipError(f"lora_merge: the tensors are on device {weight.device}, the current stream on cuda:{torch.cuda.current_device()}")
    if (lora_a is None) != (lora_b is None):
        raise VclozeHipError("lora_merge: lora_a and lora_b come together")
    R = 0
    if lora_a is not None:
        for n, t in (("lora_a", lora_a), ("lora_b", lora_b)):
            if t.dtype == torch.float32:
                raise VclozeHipError(f"lora_merge {n}: f32 LoRA factors are not merged on the bf16 matrix cores (they would be "
                                     "rounded); use the torch merge (lora_merge=\"torch\") or cast the factors to bf16")
            _bf16(t, "lora_merge " + n)
            if t.dim() != 2 or t.stride(1) != 1:
                raise VclozeHipError(f"lora_merge {n}: need a 2-D tensor with contiguous last dim")
        R = lora_a.shape[0]
        if lora_a.shape[1] != I or tuple(lora_b.shape) != (O, R):
            raise VclozeHipError(f"lora_merge shape mismatch W{tuple(weight.shape)} A{tuple(lora_a.shape)} B{tuple(lora_b.shape)}")
    if out is None:
        out = torch.empty(O, I, dtype=torch.bfloat16, device=weight.device)
    _bf16(out, "lora_merge out")
    if tuple(out.shape) != (O, I) or out.stride(1) != 1:
        raise VclozeHipError(f"lora_merge out: need a [{O}, {I}] view with contiguous last dim, got {tuple(out.shape)}")
    bias_out = None
    for n, t in (("bias", bias), ("lora_b_bias", lora_b_bias)):
        if t is None:
            continue
        ok = (torch.bfloat16, torch.float32) if n == "bias" else (torch.bfloat16,)
        if not t.is_cuda or t.dtype not in ok or tuple(t.shape) != (O,) or not t.is_contiguous():
            raise VclozeHipError(f"lora_merge {n}: need a contiguous CUDA [{O}] tensor of {ok}, got {t.dtype} {tuple(t.shape)}")
        bias_out = torch.empty(O, dtype=torch.bfloat16, device=weight.device) if bias_out is None else bias_out
    args = (weight.data_ptr(), int(weight.dtype == torch.float32), weight.stride(0),
            _p(lora_a), lora_a.stride(0) if R else 0, _p(lora_b), lora_b.stride(0) if R else 0, float(scale),
            out.data_ptr(), out.stride(0), _p(bias), int(bias is not None and bias.dtype == torch.float32),
            _p(lora_b_bias), _p(bias_out), O, I, R)
    if qkv_heads:
        _check(lib().vc_lora_merge_qkv(*args, int(qkv_heads), stream if stream is not None else cur_stream()), "vc_lora_merge_qkv")
    else:
        _check(lib().vc_lora_merge(*args, stream if stream is not None else cur_stream()), "vc_lora_merge")
    return out, bias_out


def ln_modulate(x, shift, scale, out=None, step_ptr=None, mod_step_stride=0, stream=None, rows_per_batch=None,
                mod_bstride=0):
    _bf16(x, "x")
    rows, D = x.shape
    if out is None:
        out = torch.empty(rows, D, dtype=torch.bfloat16, device=x.device)
    _check(lib().vc_ln_modulate(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), shift.data_ptr(),
                                scale.data_ptr(), mod_bstride, rows, D, rows_per_batch or rows, _p(step_ptr), mod_step_stride,
                                stream if stream is not None else cur_stream()), "vc_ln_modulate")
    return out


def ln_modulate2(streams, step_ptr=None, mod_step_stride=0, stream=None, mod_bstride=0) -> None:
    """LayerNorm + modulate over one or two row sets in one launch; streams: [(x, shift, scale, out, rows_per_batch), ...]
    (the img and txt streams of a DoubleStreamBlock)."""
    if not 1 <= len(streams) <= 2:
        raise VclozeHipError("ln_modulate2 takes one or two row sets")
    segs, D = [], streams[0][0].shape[1]
    for (x, shift, scale, out, rpb) in streams:
        _bf16(x, "x"); _bf16(out, "out")
        if x.shape[1] != D or out.shape != x.shape:
            raise VclozeHipError("ln_modulate2: row sets must share D, and out must match x")
        segs.append(LnStream(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), shift.data_ptr(), scale.data_ptr(),
                             x.shape[0], rpb or x.shape[0]))
    _check(lib().vc_ln_modulate2(C.byref(segs[0]), C.byref(segs[1]) if len(segs) > 1 else None, mod_bstride, D,
                                 _p(step_ptr), mod_step_stride, stream if stream is not None else cur_stream()), "vc_ln_modulate2")


QKN_Q, QKN_K, QKN_VT, QKN_QPRE = 1, 2, 4, 8


def qknorm_rope_vt(qkv, q_scale, k_scale, rope, vt, L, H, stream=None, q_scale2=None, k_scale2=None, split=0, B=1,
                   parts=QKN_Q | QKN_K | QKN_VT):
    """qkv: [L, >=3*H*128] rows (q|k|v at column 0, H*128, 2*H*128); rope: [L,64,2] f32; vt: [H,128,Lpad].
    rows < split use (q_scale, k_scale), the rest (q_scale2, k_scale2) when given.  parts: which of q / k / V^T to do."""
    _bf16(qkv, "qkv")
    if rope.dtype != torch.float32 or not rope.is_contiguous():
        raise VclozeHipError("rope table must be contiguous f32 [B?,L,64,2]")
    Lpad = vt.shape[-1]
    # B > 1: qkv rows are sample-major ([B*L, ld]), rope [B,L,64,2], vt [B,H,128,Lpad]
    _check(lib().vc_qknorm_rope_vt(qkv.data_ptr(), qkv.stride(0), L * qkv.stride(0), q_scale.data_ptr(), k_scale.data_ptr(),
                                   _p(q_scale2), _p(k_scale2), split, rope.data_ptr(), L * 128 if rope.dim() == 4 else 0,
                                   vt.data_ptr(), B, L, Lpad, H, parts,
                                   stream if stream is not None else cur_stream()), "vc_qknorm_rope_vt")


_attn_scratch = {}


def attention_scratch(device) -> torch.Tensor:
    """The partial-result buffer of the tail-split attention (variants 7 / 12 / 28), one per device; launches on one stream
    serialise their use of it.  ZERO-initialised: variant 28 combines the pieces inside the launch through flag words at the
    end of the buffer that are zero before and after every launch (VcAttention.variant bit 16)."""
    key = str(device)
    if key not in _attn_scratch:
        _attn_scratch[key] = torch.zeros(lib().vc_attention_scratch_bytes(), dtype=torch.uint8, device=device)
    return _attn_scratch[key]


def attention(qkv, vt, out, L, H, kv_len=None, variant=0, stream=None, B=1, scratch=None, q_norm=None, kv_gap=None,
              logit_bound=0.0, q_prescaled=False):
    """out: [B*L, >=H*128] rows (B L (H D)), sample-major like qkv; kv_len: optional int32 device tensor [B];
    scratch: uint8 device buffer of >= vc_attention_scratch_bytes() for the tail split (taken from attention_scratch()
    when omitted); q_norm = (q_scale, q_scale2 | None, split, rope): QKNorm + RoPE of the RAW query rows inside the kernel
    (variants 8 / 12; the pre-pass then runs with parts = QKN_K | QKN_VT); q_prescaled: the q columns hold normalised, rotated
    queries times 128^-0.5 * log2(e) (make_problem(qn_prescale=True) / QKN_QPRE; variants 8 / 12)."""
    _bf16(qkv, "qkv"); _bf16(vt, "vt"); _bf16(out, "out")
    if scratch is None and variant & 4:
        scratch = attention_scratch(qkv.device)
    a = Attention()
    a.qkv, a.ld, a.bstride = qkv.data_ptr(), qkv.stride(0), L * qkv.stride(0)
    a.vt, a.out, a.ldo, a.out_bstride = vt.data_ptr(), out.data_ptr(), out.stride(0), L * out.stride(0)
    a.kv_len = _p(kv_len)
    a.kv_gap = _p(kv_gap)      # int32 [B, 2] device tensor: (lo, hi) of a second masked range (needs kv_len)
    a.B, a.L, a.Lpad, a.H, a.variant = B, L, vt.shape[-1], H, variant
    a.scratch, a.scratch_bytes = _p(scratch), scratch.numel() if scratch is not None else 0
    a.q_prescaled = int(bool(q_prescaled))
    a.logit_bound = float(logit_bound)   # > 0: |q.k| * 128^-0.5 * log2(e) <= logit_bound guaranteed (variants 8 / 12: no running max)
    if q_norm is not None:
        qs, qs2, split, rope = q_norm
        _bf16(qs, "q_scale")
        if rope.dtype != torch.float32 or not rope.is_contiguous():
            raise VclozeHipError("rope table must be contiguous f32 [B?,L,64,2]")
        a.q_scale, a.q_scale2, a.split = qs.data_ptr(), _p(qs2), split
        a.rope, a.rope_bstride = rope.data_ptr(), L * 128 if rope.dim() == 4 else 0
    _check(lib().vc_attention(C.byref(a), stream if stream is not None else cur_stream()), "vc_attention")


def attention_plan(a: Attention, n_cu: int = 0) -> list:
    """vc_attention_plan: the sixteen integers of the launch plan of `a` on n_cu compute units (0 = the current device's);
    no launch, no GPU needed, no pointer of `a` is dereferenced (include/vcloze_hip.h has the layout)."""
    out = (C.c_int32 * 16)()
    _check(lib().vc_attention_plan(C.byref(a), n_cu, out), "vc_attention_plan")
    return list(out)


@functools.lru_cache(maxsize=None)
def attention_variant_by_size(B: int, L: int, H: int, n_cu: int) -> int:
    """the variant the planner chooses by size (out[0] of the plan; 28, 8 or 3)"""
    a = Attention()
    a.qkv = a.vt = a.out = 0x1000          # never dereferenced by the planner
    a.B, a.L, a.Lpad, a.H = B, L, (L + 63) // 64 * 64, H
    a.ld, a.bstride, a.ldo, a.out_bstride = 3 * H * 128, L * 3 * H * 128, H * 128, L * H * 128
    return attention_plan(a, n_cu)[0]


def timestep_embedding(t_f32, freqs_f32, out_bf16, round_t_bf16=False, stream=None):
    n, half = t_f32.numel(), freqs_f32.numel()
    _check(lib().vc_timestep_embedding(t_f32.data_ptr(), freqs_f32.data_ptr(), out_bf16.data_ptr(), n, half,
                                       int(round_t_bf16), stream if stream is not None else cur_stream()),
           "vc_timestep_embedding")


def silu(x, out=None, stream=None):
    out = torch.empty_like(x) if out is None else out
    _check(lib().vc_silu(x.data_ptr(), out.data_ptr(), x.numel(), stream if stream is not None else cur_stream()), "vc_silu")
    return out


def act2d(x, out, act, stream=None):
    """out = bf16(act(x)) on 2-D row views; act: "gelu" (tanh) or "silu"."""
    for t in (x, out):
        _bf16(t, "act2d")
        if t.dim() != 2 or t.stride(1) != 1 or t.shape != x.shape:
            raise VclozeHipError("act2d: 2-D views of one shape with contiguous rows expected")
    _check(lib().vc_act2d(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0], x.shape[1],
                          {"gelu": 0, "silu": 1}[act], stream if stream is not None else cur_stream()), "vc_act2d")
    return out


def gate_residual(y, res, gate, out, step_ptr=None, gate_step_stride=0, stream=None):
    """out = bf16(res + bf16(gate * y)) on 2-D row views (last dim contiguous); out may alias res."""
    for t in (y, res, out):
        _bf16(t, "gate_residual")
        if t.dim() != 2 or t.stride(1) != 1 or t.shape != y.shape:
            raise VclozeHipError("gate_residual: 2-D views of one shape with contiguous rows expected")
    _check(lib().vc_gate_residual(y.data_ptr(), y.stride(0), res.data_ptr(), res.stride(0), gate.data_ptr(), out.data_ptr(),
                                  out.stride(0), y.shape[0], y.shape[1], _p(step_ptr), gate_step_stride,
                                  stream if stream is not None else cur_stream()), "vc_gate_residual")


def add3(a, b, c=None, out=None, stream=None):
    out = torch.empty_like(a) if out is None else out
    _check(lib().vc_add3(a.data_ptr(), b.data_ptr(), _p(c), out.data_ptr(), a.numel(), b.numel(),
                         c.numel() if c is not None else 1, stream if stream is not None else cur_stream()), "vc_add3")
    return out


def copy(dst, src, stream=None):
    if dst.numel() * dst.element_size() != src.numel() * src.element_size() or not (dst.is_contiguous() and src.is_contiguous()):
        raise VclozeHipError("copy: size/contiguity mismatch")
    _check(lib().vc_copy(dst.data_ptr(), src.data_ptr(), src.numel() * src.element_size(),
                         stream if stream is not None else cur_stream()), "vc_copy")


def concat_cols(x, cond, out, stream=None):
    rows = x.shape[0]
    _check(lib().vc_concat_cols(x.data_ptr(), x.shape[1], cond.data_ptr(), cond.shape[1], out.data_ptr(), rows,
                                stream if stream is not None else cur_stream()), "vc_concat_cols")
    return out


def euler_step_f32(x32, shadow, v, dts, step_ptr=None, stream=None):
    """f32 master state: x32 += f32(bf16(bf16(dt) * (-v))); shadow = bf16(x32).  v None: refresh the shadow only."""
    _check(lib().vc_euler_step_f32(x32.data_ptr(), shadow.data_ptr(), _p(v), _p(dts), _p(step_ptr), x32.numel(),
                                   stream if stream is not None else cur_stream()), "vc_euler_step_f32")


def euler_step(x, v, dts, step_ptr=None, stream=None):
    _check(lib().vc_euler_step(x.data_ptr(), v.data_ptr(), dts.data_ptr(), _p(step_ptr), x.numel(),
                               stream if stream is not None else cur_stream()), "vc_euler_step")


def solver_evals(method) -> int:
    """vc_solver_evals: model evaluations per solver step of a method name or VC_SOLVER_* code (no GPU needed)"""
    code = SOLVERS.get(method, -1) if isinstance(method, str) else int(method)
    n = lib().vc_solver_evals(code)
    _check(0 if n > 0 else n, f"vc_solver_evals({method!r})")
    return n


def ode_stage(method, stage: int, y, v, k, y_in, dts, eval_ptr=None, stream=None):
    """vc_ode_stage: one stage combination of a midpoint / rk4 step.  y: the bf16 or f32 state (replaced by y1 by the last stage),
    v: this stage's bf16 model output, k: bf16 [3, n] (rk4; None for midpoint), y_in: bf16, the next evaluation's input;
    stage < 0: the stage is eval_ptr[0] % evals on the device; dt = dts[eval_ptr[0] // evals]."""
    code = SOLVERS[method] if isinstance(method, str) else int(method)
    if y.dtype not in (torch.bfloat16, torch.float32) or dts.dtype != torch.float32:
        raise VclozeHipError(f"vc_ode_stage: bf16 or f32 state and an f32 dt table expected, got {y.dtype} / {dts.dtype}")
    _bf16(v, "v"); _bf16(y_in, "y_in")
    if k is not None:
        _bf16(k, "k")
        if k.numel() < 3 * y.numel():
            raise VclozeHipError("vc_ode_stage: k must hold 3 * n values")
    if not (y.is_cuda and y.is_contiguous() and v.is_contiguous() and y_in.is_contiguous() and (k is None or k.is_contiguous())):
        raise VclozeHipError("vc_ode_stage: contiguous device tensors expected")
    if v.numel() != y.numel() or y_in.numel() != y.numel():
        raise VclozeHipError("vc_ode_stage: y, v, y_in must hold the same number of elements")
    _check(lib().vc_ode_stage(code, int(stage), y.data_ptr(), int(y.dtype == torch.bfloat16), v.data_ptr(), _p(k), y_in.data_ptr(),
                              dts.data_ptr(), _p(eval_ptr), y.numel(), stream if stream is not None else cur_stream()), "vc_ode_stage")


def step_advance(step_ptr, stream=None):
    _check(lib().vc_step_advance(step_ptr.data_ptr(), stream if stream is not None else cur_stream()), "vc_step_advance")


DOPRI5_MAX_BLOCKS = 256              # VC_DOPRI5_MAX_BLOCKS


def _dopri5_f32(what, **tensors):
    for name, t in tensors.items():
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise VclozeHipError(f"{what}: {name} must be a contiguous CUDA f32 tensor")


def _dopri5_k(what, k, n):
    _bf16(k, "k")
    if not k.is_contiguous() or k.numel() != 7 * n:
        raise VclozeHipError(f"{what}: k must be a contiguous bf16 [7, n] tensor")


def dopri5_stage(stage: int, y0, k, v, dt, eval_ptr=None, y_stage=None, y_in=None, stream=None):
    """vc_dopri5_stage: k[stage] = -v (v None: in place already) and the next evaluation's state y0 + dt * (row of the tableau) ->
    y_stage (f32) / y_in (bf16); stage 5 forms y1, stage 6 only stores k7, stage 7 (v None) the probe state y0 + dt * k1;
    stage < 0: eval_ptr[0] on the device.  y0: f32 [n], k: bf16 [7, n], dt: f32 [1] on the device."""
    n = y0.numel()
    _dopri5_f32("vc_dopri5_stage", y0=y0, dt=dt, y_stage=y_stage)
    _dopri5_k("vc_dopri5_stage", k, n)
    for name, t in (("v", v), ("y_in", y_in)):
        if t is not None:
            _bf16(t, name)
            if not t.is_contiguous() or t.numel() != n:
                raise VclozeHipError(f"vc_dopri5_stage: {name} must be contiguous and hold n values")
    if y_stage is not None and y_stage.numel() != n:
        raise VclozeHipError("vc_dopri5_stage: y_stage must hold n values")
    _check(lib().vc_dopri5_stage(int(stage), y0.data_ptr(), k.data_ptr(), _p(v), dt.data_ptr(), _p(eval_ptr), _p(y_stage), _p(y_in), n,
                                 stream if stream is not None else cur_stream()), "vc_dopri5_stage")


def dopri5_error_ratio(y0, y1, k, dt, rtol: float, atol: float, mode: int = 0, out=None, stream=None):
    """vc_dopri5_error_ratio: out[0] = sqrt(mean(q^2)) over all n elements in a fixed order (f32 [1], returned).  mode 0: the error
    ratio of the step (y0, y1, k, dt); modes 1, 2, 3: the initial-step norms of y0, k1, k2 - k1 over atol + rtol |y0|."""
    n = y0.numel()
    _dopri5_f32("vc_dopri5_error_ratio", y0=y0, y1=y1, dt=dt, out=out)
    if k is not None:
        _dopri5_k("vc_dopri5_error_ratio", k, n)
    if y1 is not None and y1.numel() != n:
        raise VclozeHipError("vc_dopri5_error_ratio: y1 must hold n values")
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=y0.device)
    scratch = torch.empty(DOPRI5_MAX_BLOCKS, dtype=torch.float32, device=y0.device)
    _check(lib().vc_dopri5_error_ratio(int(mode), y0.data_ptr(), _p(y1), _p(k), _p(dt), float(rtol), float(atol), out.data_ptr(),
                                       scratch.data_ptr(), n, stream if stream is not None else cur_stream()), "vc_dopri5_error_ratio")
    return out


def dopri5_interp(y0, y1, k, dt, theta: float, out=None, dtype=torch.float32, stream=None):
    """vc_dopri5_interp: the dense output of the step (y0, y1, k, dt) at theta in [0, 1] -> out (f32 or bf16, n values)"""
    n = y0.numel()
    _dopri5_f32("vc_dopri5_interp", y0=y0, y1=y1, dt=dt)
    _dopri5_k("vc_dopri5_interp", k, n)
    out = out if out is not None else torch.empty(y0.shape, dtype=dtype, device=y0.device)
    if out.dtype not in (torch.float32, torch.bfloat16) or not (out.is_cuda and out.is_contiguous()) or out.numel() != n or y1.numel() != n:
        raise VclozeHipError("vc_dopri5_interp: y1 and a contiguous f32 / bf16 out of n values expected")
    _check(lib().vc_dopri5_interp(y0.data_ptr(), y1.data_ptr(), k.data_ptr(), dt.data_ptr(), float(theta), out.data_ptr(),
                                  int(out.dtype == torch.bfloat16), n, stream if stream is not None else cur_stream()), "vc_dopri5_interp")
    return out


# ---- embedded Runge-Kutta pairs (vc_rk_*): the three ops above with the method as an argument
RK_METHODS = {"dopri5": 0, "bosh3": 1, "adaptive_heun": 2}      # VC_RK_*


def _rk_code(method) -> int:
    if isinstance(method, str):
        if method not in RK_METHODS:
            raise VclozeHipError(f"unknown embedded pair {method!r}: one of {sorted(RK_METHODS)} expected")
        return RK_METHODS[method]
    return int(method)


def rk_evals(method) -> dict:
    """vc_rk_evals: {"start", "per_attempt", "order", "stages"} of a method name or VC_RK_* code (no GPU needed)"""
    st, per, order = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    _check(lib().vc_rk_evals(_rk_code(method), C.byref(st), C.byref(per), C.byref(order)), f"vc_rk_evals({method!r})")
    return {"start": st.value, "per_attempt": per.value, "order": order.value, "stages": per.value + 1}


def _rk_k(what, k, n, stages):
    _bf16(k, "k")
    if not k.is_contiguous() or k.numel() < stages * n or k.numel() % n:
        raise VclozeHipError(f"{what}: k must be a contiguous bf16 [S, n] tensor of at least the method's {stages} planes")


def rk_stage(method, stage: int, y0, k, v, dt, eval_ptr=None, y_stage=None, y_in=None, stream=None):
    """vc_rk_stage: dopri5_stage with the tableau of `method` (a name of RK_METHODS or a VC_RK_* code).  k: bf16 [S, n] or more planes;
    stage S - 2 forms y1, stage S - 1 only stores kS, stage 7 (v None) the probe state; stage < 0: eval_ptr[0] on the device."""
    code, n = _rk_code(method), y0.numel()
    _dopri5_f32("vc_rk_stage", y0=y0, dt=dt, y_stage=y_stage)
    _rk_k("vc_rk_stage", k, n, rk_evals(code)["stages"])
    for name, t in (("v", v), ("y_in", y_in)):
        if t is not None:
            _bf16(t, name)
            if not t.is_contiguous() or t.numel() != n:
                raise VclozeHipError(f"vc_rk_stage: {name} must be contiguous and hold n values")
    if y_stage is not None and y_stage.numel() != n:
        raise VclozeHipError("vc_rk_stage: y_stage must hold n values")
    _check(lib().vc_rk_stage(code, int(stage), y0.data_ptr(), k.data_ptr(), _p(v), dt.data_ptr(), _p(eval_ptr), _p(y_stage), _p(y_in), n,
                             stream if stream is not None else cur_stream()), "vc_rk_stage")


def rk_error_ratio(method, y0, y1, k, dt, rtol: float, atol: float, mode: int = 0, out=None, stream=None):
    """vc_rk_error_ratio: dopri5_error_ratio with the e row of `method` in mode 0 (modes 1, 2, 3: the initial-step norms)"""
    code, n = _rk_code(method), y0.numel()
    _dopri5_f32("vc_rk_error_ratio", y0=y0, y1=y1, dt=dt, out=out)
    if k is not None:
        _rk_k("vc_rk_error_ratio", k, n, rk_evals(code)["stages"])
    if y1 is not None and y1.numel() != n:
        raise VclozeHipError("vc_rk_error_ratio: y1 must hold n values")
    out = out if out is not None else torch.empty(1, dtype=torch.float32, device=y0.device)
    scratch = torch.empty(DOPRI5_MAX_BLOCKS, dtype=torch.float32, device=y0.device)
    _check(lib().vc_rk_error_ratio(code, int(mode), y0.data_ptr(), _p(y1), _p(k), _p(dt), float(rtol), float(atol), out.data_ptr(),
                                   scratch.data_ptr(), n, stream if stream is not None else cur_stream()), "vc_rk_error_ratio")
    return out


def rk_interp(method, y0, y1, k, dt, theta: float, out=None, dtype=torch.float32, stream=None):
    """vc_rk_interp: the Hermite dense output of the step (y0, y1, k, dt) of "bosh3" / "adaptive_heun" at theta in [0, 1] -> out (f32 or
    bf16, n values)"""
    code, n = _rk_code(method), y0.numel()
    _dopri5_f32("vc_rk_interp", y0=y0, y1=y1, dt=dt)
    _rk_k("vc_rk_interp", k, n, rk_evals(code)["stages"])
    out = out if out is not None else torch.empty(y0.shape, dtype=dtype, device=y0.device)
    if out.dtype not in (torch.float32, torch.bfloat16) or not (out.is_cuda and out.is_contiguous()) or out.numel() != n or y1.numel() != n:
        raise VclozeHipError("vc_rk_interp: y1 and a contiguous f32 / bf16 out of n values expected")
    _check(lib().vc_rk_interp(code, y0.data_ptr(), y1.data_ptr(), k.data_ptr(), dt.data_ptr(), float(theta), out.data_ptr(),
                              int(out.dtype == torch.bfloat16), n, stream if stream is not None else cur_stream()), "vc_rk_interp")
    return out


RESIDUAL_CHANGE_MAX_BLOCKS = 256     # VC_RESIDUAL_CHANGE_MAX_BLOCKS


def _cstr(v):
    return None if v is None else str(v).encode()


def sde_plan(method: str, form: str, norm: float, last_step, last_step_size: float, t_grid) -> dict:
    """vc_sde_plan (host only): the coefficient rows and model times of a stochastic trajectory over the f32 grid `t_grid` ->
    {"rows": f32 [n_rows, 5] (mode, h, A, Bc, g; for "Heun" one injection row behind the evaluations'), "times": f32 [evals] (1 - t),
    "evals", "draws"}.  A refusal (unknown names, a grid that does not increase, a non-finite coefficient) raises VclozeHipError."""
    t = np.ascontiguousarray(t_grid.detach().cpu().numpy() if torch.is_tensor(t_grid) else t_grid, dtype=np.float32).reshape(-1)
    tp = t.ctypes.data_as(C.POINTER(C.c_float)) if t.size else None
    args = (_cstr(method), _cstr(form), float(norm), _cstr(last_step), float(last_step_size), tp, int(t.size))
    ne, nd = C.c_int32(0), C.c_int32(0)
    _check(lib().vc_sde_plan(*args, None, None, 0, C.byref(ne), C.byref(nd)), "vc_sde_plan")
    cap = ne.value + 1
    rows, times = np.zeros((cap, SDE_ROW), np.float32), np.zeros(cap, np.float32)
    _check(lib().vc_sde_plan(*args, rows.ctypes.data_as(C.POINTER(C.c_float)), times.ctypes.data_as(C.POINTER(C.c_float)), cap,
                             C.byref(ne), C.byref(nd)), "vc_sde_plan")
    n_rows = ne.value + (1 if method == "Heun" else 0)
    return {"rows": rows[:n_rows], "times": times[:ne.value], "evals": ne.value, "draws": nd.value}


def ms_plan(order: int, t_grid) -> dict:
    """vc_ms_plan (host only): the coefficient rows and model times of an Adams-Bashforth trajectory of `order` (1..4) over the f32
    grid `t_grid` -> {"rows": f32 [n - 1, 4], "times": f32 [n - 1] (1 - t), "evals": n - 1}.  A refusal (the order, fewer than two
    points, a grid that does not increase, a non-finite coefficient) raises VclozeHipError."""
    t = np.ascontiguousarray(t_grid.detach().cpu().numpy() if torch.is_tensor(t_grid) else t_grid, dtype=np.float32).reshape(-1)
    tp = t.ctypes.data_as(C.POINTER(C.c_float)) if t.size else None
    ne = C.c_int32(0)
    _check(lib().vc_ms_plan(int(order), tp, int(t.size), None, None, 0, C.byref(ne)), "vc_ms_plan")
    cap = ne.value
    rows, times = np.zeros((cap, MS_ROW), np.float32), np.zeros(cap, np.float32)
    _check(lib().vc_ms_plan(int(order), tp, int(t.size), rows.ctypes.data_as(C.POINTER(C.c_float)),
                            times.ctypes.data_as(C.POINTER(C.c_float)), cap, C.byref(ne)), "vc_ms_plan")
    return {"rows": rows, "times": times, "evals": ne.value}


def ms_stage(eval_index: int, table, y, v, hist, y_in, eval_ptr=None, stream=None) -> None:
    """vc_ms_stage: one Adams-Bashforth update on n = y.numel() elements.  table: f32 [n_rows, 4] (device); row = eval_index, or with
    eval_index < 0 the device-side counter eval_ptr (int32 [1]).  y: f32 [n]; v: the model's bf16 output [n]; hist: bf16 [3, n], the
    ring of past outputs (v_{e-j} in slot (e - j) % 3; v is stored into slot e % 3); y_in: bf16 [n] <- bf16(y)."""
    n = y.numel()
    for name, t, dt in (("table", table, torch.float32), ("y", y, torch.float32), ("v", v, torch.bfloat16), ("hist", hist, torch.bfloat16),
                        ("y_in", y_in, torch.bfloat16), ("eval_ptr", eval_ptr, torch.int32)):
        if t is None:
            if name == "eval_ptr":
                continue
            raise VclozeHipError(f"vc_ms_stage: {name} is required")
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise VclozeHipError(f"vc_ms_stage: {name} must be a contiguous CUDA {dt} tensor, got {t.dtype} on {t.device}")
        if name in ("v", "y_in") and t.numel() != n:
            raise VclozeHipError(f"vc_ms_stage: {name} must hold n = {n} values, got {t.numel()}")
    if table.dim() != 2 or table.shape[1] != MS_ROW or hist.numel() != MS_HIST * n:
        raise VclozeHipError(f"vc_ms_stage: table must be [n_rows, {MS_ROW}] and hist hold {MS_HIST} planes of n = {n} values")
    _check(lib().vc_ms_stage(int(eval_index), table.data_ptr(), table.shape[0], y.data_ptr(), v.data_ptr(), hist.data_ptr(), y_in.data_ptr(),
                             _p(eval_ptr), n, stream if stream is not None else cur_stream()), "vc_ms_stage")


def rng_words(seed, offset, device=None) -> torch.Tensor:
    """the (seed, offset) word pair vc_sde_stage reads from device memory: two uint64, held in an int64 tensor [2]"""
    w = np.array([_u64(seed, "seed"), _u64(offset, "offset")], dtype=np.uint64).view(np.int64)
    return torch.from_numpy(w.copy()).to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))


def sde_stage(eval_index: int, table, y, v, y_in, rng, xhat=None, k1=None, eval_ptr=None, stream=None) -> None:
    """vc_sde_stage: one update of the stochastic sampler on n = y.numel() elements.  table: f32 [n_rows, 5] (device); row =
    eval_index, or with eval_index < 0 the device-side counter eval_ptr (int32 [1]).  y, xhat, k1: f32 [n]; v: the model's bf16 output
    (None for an injection row); y_in: bf16 [n]; rng: `rng_words(seed, offset)`.  Draw d of the row takes stream positions
    offset + d * n + i."""
    n = y.numel()
    for name, t, dt in (("table", table, torch.float32), ("y", y, torch.float32), ("xhat", xhat, torch.float32), ("k1", k1, torch.float32),
                        ("v", v, torch.bfloat16), ("y_in", y_in, torch.bfloat16), ("rng", rng, torch.int64), ("eval_ptr", eval_ptr, torch.int32)):
        if t is None:
            continue
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise VclozeHipError(f"vc_sde_stage: {name} must be a contiguous CUDA {dt} tensor, got {t.dtype} on {t.device}")
        if name in ("xhat", "k1", "v", "y_in") and t.numel() != n:
            raise VclozeHipError(f"vc_sde_stage: {name} must hold n = {n} values, got {t.numel()}")
    if table.dim() != 2 or table.shape[1] != SDE_ROW or rng.numel() != 2:
        raise VclozeHipError("vc_sde_stage: table must be [n_rows, 5] and rng hold the two words (seed, offset)")
    _check(lib().vc_sde_stage(int(eval_index), table.data_ptr(), table.shape[0], y.data_ptr(), _p(v), y_in.data_ptr(), _p(xhat), _p(k1),
                              rng.data_ptr(), _p(eval_ptr), n, stream if stream is not None else cur_stream()), "vc_sde_stage")


def residual_change(h0, h1, p, r=None, stream=None):
    """vc_residual_change on [B, n] bf16 tensors (n = everything behind the first dimension): r = bf16(h1 - h0) and, per sample,
    (sum |r - p|, sum |p|) in f32.  Returns (r, sums [B, 2] f32, metric [1] f32 = max_b sums[b, 0] / sums[b, 1])."""
    for t, name in ((h0, "h0"), (h1, "h1"), (p, "p")):
        _bf16(t, name)
    if not (h0.shape == h1.shape == p.shape and h0.dim() >= 2 and h0.is_contiguous() and h1.is_contiguous() and p.is_contiguous()):
        raise VclozeHipError("vc_residual_change: contiguous [B, ...] tensors of one shape expected")
    r = torch.empty_like(h0) if r is None else r
    _bf16(r, "r")
    if r.shape != h0.shape or not r.is_contiguous():
        raise VclozeHipError("vc_residual_change: r must be a contiguous tensor of the inputs' shape")
    B = h0.shape[0]
    sums = torch.empty(B, 2, dtype=torch.float32, device=h0.device)
    metric = torch.empty(1, dtype=torch.float32, device=h0.device)
    scratch = torch.empty(B * 2 * RESIDUAL_CHANGE_MAX_BLOCKS, dtype=torch.float32, device=h0.device)
    _check(lib().vc_residual_change(h0.data_ptr(), h1.data_ptr(), p.data_ptr(), r.data_ptr(), sums.data_ptr(), metric.data_ptr(),
                                    scratch.data_ptr(), B, h0.numel() // B, stream if stream is not None else cur_stream()),
           "vc_residual_change")
    return r, sums, metric


STAT_DTYPE = np.dtype([("max_abs", np.float32), ("sum_sq", np.float32), ("nonfinite", np.uint32), ("count", np.uint32)])   # VcStat


def stats_to_numpy(log: torch.Tensor) -> np.ndarray:
    """a device tensor of VcStat records (uint8, 16 bytes each) -> a structured numpy array (fields of STAT_DTYPE)"""
    return log.detach().cpu().contiguous().view(torch.uint8).numpy().view(STAT_DTYPE)


def tensor_stats(x, out=None, row_ptr=None, capacity: int = 1, stream=None) -> torch.Tensor:
    """vc_tensor_stats on x [B, rows, cols], bf16 or f32, unit stride in the last dimension (any row / sample strides: views of a
    strided stream are fine): per sample (max |x| and sum x^2 over the finite elements, the number of non-finite elements, the number
    of elements).  out: a uint8 tensor of capacity * B records of 16 bytes (`stats_to_numpy` reads it); the records go to row
    *row_ptr (an int32 device tensor), or to row 0.  Returns out."""
    if x.dtype not in (torch.bfloat16, torch.float32) or x.dim() != 3 or x.stride(2) != 1:
        raise VclozeHipError("vc_tensor_stats: a [B, rows, cols] bf16 / f32 tensor with unit column stride expected")
    B, R, Cc = x.shape
    if out is None:
        out = torch.zeros(capacity * B * 16, dtype=torch.uint8, device=x.device)
    scratch = torch.empty(B * 4 * MONITOR_MAX_BLOCKS, dtype=torch.float32, device=x.device)
    _check(lib().vc_tensor_stats(x.data_ptr(), int(x.dtype == torch.float32), x.stride(0), x.stride(1), B, R, Cc, out.data_ptr(), B,
                                 _p(row_ptr), int(capacity), scratch.data_ptr(), stream if stream is not None else cur_stream()),
           "vc_tensor_stats")
    return out


FM_LOSS_MAX_BLOCKS = 256             # VC_FM_LOSS_MAX_BLOCKS
FM_MAX_HOST_COUNTS = 64              # VC_FM_MAX_HOST_COUNTS


def fm_plan(x1, t, xt, x0=None, seed=0, offset=0, ut=None, stream=None):
    """vc_fm_plan: the path sample of the flow-matching loss.  x1 [B, rows, cols] bf16 / f32 with unit column stride (any row / sample
    strides); t [B] f32 on the device; xt: a bf16 [B, rows, ld] tensor (or [B * rows, ld]) with ld >= cols whose first `cols` columns
    receive bf16(t x1 + (1 - t) x0) - the other columns are left alone; x0: a contiguous [B, rows, cols] tensor of x1's dtype, or None:
    drawn in the kernel at (seed, offset + flat index), what `randn(x1.shape, seed, offset, x1.dtype)` holds.  Returns ut = x1 - x0, f32
    [B, rows, cols]."""
    if x1.dtype not in (torch.bfloat16, torch.float32) or x1.dim() != 3 or x1.stride(2) != 1:
        raise VclozeHipError("vc_fm_plan: a [B, rows, cols] bf16 / f32 x1 with unit column stride expected")
    B, R, Cc = x1.shape
    _bf16(xt, "xt")
    if xt.dim() not in (2, 3) or xt.stride(-1) != 1 or xt.numel() == 0 or xt.shape[-1] < Cc or xt.numel() // xt.shape[-1] != B * R or \
            (xt.dim() == 3 and xt.stride(0) != R * xt.stride(1)):
        raise VclozeHipError(f"vc_fm_plan: xt must hold {B * R} evenly strided rows of at least {Cc} columns, got {tuple(xt.shape)}")
    if t.dtype != torch.float32 or not t.is_cuda or t.numel() != B or not t.is_contiguous():
        raise VclozeHipError(f"vc_fm_plan: t must be a contiguous f32 device tensor of {B} values")
    if x0 is not None and (x0.dtype != x1.dtype or tuple(x0.shape) != (B, R, Cc) or not x0.is_contiguous()):
        raise VclozeHipError(f"vc_fm_plan: x0 must be a contiguous {x1.dtype} tensor of shape {(B, R, Cc)}")
    if ut is None:
        ut = torch.empty(B, R, Cc, dtype=torch.float32, device=x1.device)
    elif ut.dtype != torch.float32 or ut.numel() != B * R * Cc or not ut.is_contiguous():
        raise VclozeHipError("vc_fm_plan: ut must be a contiguous f32 tensor of x1's element count")
    _check(lib().vc_fm_plan(x1.data_ptr(), int(x1.dtype == torch.float32), x1.stride(0), x1.stride(1), t.data_ptr(), _p(x0), _u64(seed, "seed"),
                            _u64(offset, "offset"), xt.data_ptr(), xt.stride(-2), ut.data_ptr(), B, R, Cc,
                            stream if stream is not None else cur_stream()), "vc_fm_plan")
    return ut


def fm_loss(out, ut, valid_rows=None, loss=None, stream=None):
    """vc_fm_loss: loss[b] = sum over the first valid_rows[b] rows of ((-out) - ut)^2 / (valid_rows[b] * cols), f32 [B], in the fixed
    summation order of include/vcloze_hip.h (`transport.fm_loss_terms(ordered=True)` restates it).  out: the model's bf16 output [B, rows,
    cols'] with unit column stride, rows stride(1) apart, samples rows * stride(1) apart (cols' >= cols: a column window is fine); ut f32
    [B, rows, cols] contiguous; valid_rows: None (every row), an int32 device tensor [B], or a sequence of B ints (at most
    FM_MAX_HOST_COUNTS, each in [1, rows])."""
    _bf16(out, "out")
    if ut.dtype != torch.float32 or ut.dim() != 3 or not ut.is_contiguous():
        raise VclozeHipError("vc_fm_loss: ut must be a contiguous f32 [B, rows, cols] tensor")
    B, R, Cc = ut.shape
    if out.dim() != 3 or tuple(out.shape) != (B, R, Cc) or out.stride(2) != 1 or (B > 1 and out.stride(0) != R * out.stride(1)):
        raise VclozeHipError(f"vc_fm_loss: out must be a bf16 view of shape {(B, R, Cc)} with evenly strided rows")
    host, vp, keep = 0, None, None
    if torch.is_tensor(valid_rows):
        if valid_rows.dtype != torch.int32 or not valid_rows.is_cuda or valid_rows.numel() != B or not valid_rows.is_contiguous():
            raise VclozeHipError(f"vc_fm_loss: device counts must be a contiguous int32 tensor of {B} values")
        vp = valid_rows.data_ptr()
    elif valid_rows is not None:
        keep = (C.c_int32 * len(valid_rows))(*[int(v) for v in valid_rows])
        if len(valid_rows) != B:
            raise VclozeHipError(f"vc_fm_loss: {len(valid_rows)} counts for {B} samples")
        host, vp = 1, C.cast(keep, C.c_void_p)
    if loss is None:
        loss = torch.empty(B, dtype=torch.float32, device=ut.device)
    scratch = torch.empty(B * FM_LOSS_MAX_BLOCKS, dtype=torch.float32, device=ut.device)
    _check(lib().vc_fm_loss(out.data_ptr(), out.stride(1), ut.data_ptr(), vp, host, loss.data_ptr(), scratch.data_ptr(), B, R, Cc,
                            stream if stream is not None else cur_stream()), "vc_fm_loss")
    return loss


def _residual_op(fn, what, a, b, out, stream):
    """a, b, out: [B, n...] bf16, each sample's n elements contiguous, samples stride(0) apart (views of row ranges are fine)"""
    _bf16(a, "a"); _bf16(b, "b")
    out = torch.empty(a.shape, dtype=torch.bfloat16, device=a.device) if out is None else out
    _bf16(out, "out")
    if not (a.shape == b.shape == out.shape and a.dim() >= 2):
        raise VclozeHipError(f"{what}: [B, ...] tensors of one shape expected")
    for t in (a, b, out):
        if not t[0].is_contiguous():
            raise VclozeHipError(f"{what}: every sample must be contiguous")
    B = a.shape[0]
    _check(fn(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), out.data_ptr(), out.stride(0), B, a[0].numel(),
              stream if stream is not None else cur_stream()), what)
    return out


def residual_sub(a, b, out=None, stream=None):
    """vc_residual_sub: bf16(f32(a) - f32(b))"""
    return _residual_op(lib().vc_residual_sub, "vc_residual_sub", a, b, out, stream)


def residual_add(a, b, out=None, stream=None):
    """vc_residual_add: bf16(f32(a) + f32(b))"""
    return _residual_op(lib().vc_residual_add, "vc_residual_add", a, b, out, stream)


def cfg_combine(cond, uncond, cfg_scale: float, out=None, stream=None):
    """vc_cfg_combine: out = bf16(uncond + bf16(f32(cfg_scale) * bf16(cond - uncond))), the conditional half of
    Flux.forward_with_cfg (model.py:126-145) with torch's roundings.  cond, uncond: contiguous bf16 tensors of one size; out: a new
    tensor, or `cond` / `uncond` itself (in place)."""
    _bf16(cond, "cond"); _bf16(uncond, "uncond")
    out = torch.empty_like(cond) if out is None else out
    _bf16(out, "out")
    if not (cond.is_contiguous() and uncond.is_contiguous() and out.is_contiguous()):
        raise VclozeHipError("vc_cfg_combine: contiguous tensors expected")
    if not (cond.numel() == uncond.numel() == out.numel()):
        raise VclozeHipError("vc_cfg_combine: cond, uncond and out must hold the same number of elements")
    _check(lib().vc_cfg_combine(cond.data_ptr(), uncond.data_ptr(), out.data_ptr(), cond.numel(), float(cfg_scale),
                                stream if stream is not None else cur_stream()), "vc_cfg_combine")
    return out


def sdedit_mix(noise, latent, strength, out=None, stream=None):
    _bf16(noise, "noise"); _bf16(latent, "latent")
    out = torch.empty_like(noise) if out is None else out
    _check(lib().vc_sdedit_mix(noise.data_ptr(), latent.data_ptr(), float(strength), out.data_ptr(), noise.numel(),
                               stream if stream is not None else cur_stream()), "vc_sdedit_mix")
    return out


def pack_latent(latent, tokens, col0=0, stream=None):
    """latent [C,h,w] bf16 (contiguous) -> tokens[:, col0:col0+4C] (rows of stride tokens.stride(0))."""
    _bf16(latent, "latent"); _bf16(tokens, "tokens")
    Cc, h, w = latent.shape[-3:]
    if not latent.is_contiguous() or tokens.shape[0] != (h // 2) * (w // 2):
        raise VclozeHipError("pack_latent: contiguous [C,h,w] latent and (h/2)(w/2) token rows expected")
    if Cc > 64:
        raise VclozeHipError(f"pack_latent: C={Cc} > 64 channels (the tile staged through LDS holds 64)")
    _check(lib().vc_pack_latent(latent.data_ptr(), tokens.data_ptr(), Cc, h, w, tokens.stride(0), col0,
                                stream if stream is not None else cur_stream()), "vc_pack_latent")


def pack_mask(mask, tokens, col0=0, stream=None):
    """pixel mask [H,W] bf16 -> tokens[:, col0:col0+256]."""
    _bf16(mask, "mask"); _bf16(tokens, "tokens")
    H, W = mask.shape[-2:]
    if not mask.is_contiguous() or tokens.shape[0] != (H // 16) * (W // 16):
        raise VclozeHipError("pack_mask: contiguous [H,W] mask and (H/16)(W/16) token rows expected")
    if mask.data_ptr() % 16 or tokens.data_ptr() % 16:
        raise VclozeHipError("pack_mask: the mask and the token rows must be 16-byte aligned (a view at an odd storage offset is not)")
    _check(lib().vc_pack_mask(mask.data_ptr(), tokens.data_ptr(), H, W, tokens.stride(0), col0,
                              stream if stream is not None else cur_stream()), "vc_pack_mask")


def unpack_latent(tokens, latent, col0=0, stream=None):
    _bf16(latent, "latent"); _bf16(tokens, "tokens")
    Cc, h, w = latent.shape[-3:]
    if not latent.is_contiguous() or tokens.shape[0] != (h // 2) * (w // 2):
        raise VclozeHipError("unpack_latent: contiguous [C,h,w] latent and (h/2)(w/2) token rows expected")
    if Cc > 64:
        raise VclozeHipError(f"unpack_latent: C={Cc} > 64 channels (the tile staged through LDS holds 64)")
    _check(lib().vc_unpack_latent(tokens.data_ptr(), tokens.stride(0), col0, latent.data_ptr(), Cc, h, w,
                                  stream if stream is not None else cur_stream()), "vc_unpack_latent")


# ---- the grid's host rules (csrc/grid_rules.hip; no GPU needed) and its pixel epilogue (csrc/pixels_out.hip) ----
def time_grid(n_points: int, n_tokens: int, t0: float = 0.0, t1: float = 1.0, do_shift: bool = True, time_shifting_factor=1.0) -> torch.Tensor:
    """vc_time_grid: the solver's n_points f32 time points, bit for bit transport.solver_time_grid(n_points, n_tokens, t0, t1, do_shift,
    time_shifting_factor) (None or 0 = no factor).  A CPU tensor."""
    out = torch.empty(max(int(n_points), 0), dtype=torch.float32)
    _check(lib().vc_time_grid(int(n_points), int(n_tokens), float(t0), float(t1), int(bool(do_shift)), float(time_shifting_factor or 0.0),
                              C.cast(out.data_ptr(), C.POINTER(C.c_float)) if out.numel() else None), "vc_time_grid")
    return out


def fm_times(base, snr_type: str, n_tokens: int, do_shift: bool = True) -> torch.Tensor:
    """vc_fm_times: the training times of Transport.sample for the f32 base draws `base` (uniforms, or standard normals for "lognorm"),
    bit for bit `transport.fm_times(base.float(), snr_type, n_tokens, do_shift)`.  A CPU f32 tensor; an unknown or malformed snr_type
    raises VclozeHipError."""
    b = torch.as_tensor(base).detach().to("cpu", torch.float32).contiguous().reshape(-1)
    out = torch.empty(b.numel(), dtype=torch.float32)
    fp = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_float)) if t.numel() else None  # noqa: E731
    _check(lib().vc_fm_times(_cstr(snr_type), fp(b), b.numel(), int(n_tokens), int(bool(do_shift)), fp(out)), "vc_fm_times")
    return out


def grid_tokens(rows_hw) -> int:
    """vc_grid_tokens: the image tokens of one sample whose grid rows have the LATENT sizes rows_hw = [(h, w), ...]"""
    k = len(rows_hw)
    hs, ws = (C.c_int32 * max(k, 1))(*[int(h) for h, _ in rows_hw]), (C.c_int32 * max(k, 1))(*[int(w) for _, w in rows_hw])
    n = lib().vc_grid_tokens(k, hs, ws)
    _check(0 if n >= 0 else int(n), "vc_grid_tokens")
    return int(n)


def grid_img_ids(rows_hw) -> torch.Tensor:
    """vc_grid_img_ids: [tokens, 3] f32 (CPU) = packing.grid_img_ids(rows_hw): axis 0 the row index + 1, axes 1 / 2 y and x"""
    k = len(rows_hw)
    hs, ws = (C.c_int32 * max(k, 1))(*[int(h) for h, _ in rows_hw]), (C.c_int32 * max(k, 1))(*[int(w) for _, w in rows_hw])
    out = torch.empty(grid_tokens(rows_hw), 3, dtype=torch.float32)
    _check(lib().vc_grid_img_ids(k, hs, ws, C.cast(out.data_ptr(), C.POINTER(C.c_float))), "vc_grid_img_ids")
    return out


def pixels_out(img, x0: int = 0, w: Optional[int] = None, uint8: bool = False, out=None, stream=None):
    """vc_pixels_out: columns [x0, x0 + w) of the decoded image img [3, H, W] (bf16 or f32, in [-1, 1]) as f32 [3, H, w] in [0, 1] =
    ((img.float() + 1.0) / 2.0).clamp_(0.0, 1.0), or with `uint8` as [H, w, 3] bytes = that .mul(255).to(torch.uint8) (truncating),
    HWC as PIL takes it."""
    if img.dim() != 3 or img.shape[0] != 3 or not img.is_cuda or img.dtype not in (torch.bfloat16, torch.float32) or not img.is_contiguous():
        raise VclozeHipError(f"pixels_out: a contiguous CUDA [3, H, W] bf16 / f32 image expected, got {img.dtype} {tuple(img.shape)} on {img.device}")
    H, W = img.shape[-2:]
    w = W - x0 if w is None else w
    shape, dt = ((H, w, 3), torch.uint8) if uint8 else ((3, H, w), torch.float32)
    if out is None:
        out = torch.empty([max(int(d), 0) for d in shape], dtype=dt, device=img.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != dt or not out.is_contiguous() or out.device != img.device:
        raise VclozeHipError(f"pixels_out: out must be a contiguous {dt} tensor of shape {tuple(shape)} on {img.device}")
    _check(lib().vc_pixels_out(img.data_ptr(), int(img.dtype == torch.float32), H, W, int(x0), int(w), out.data_ptr(),
                               PIXELS_U8 if uint8 else PIXELS_F32, stream if stream is not None else cur_stream()), "vc_pixels_out")
    return out


# ---- image comparison (csrc/image_metrics.hip) ----
def image_compare_scratch_bytes(Cn: int, H: int, W: int) -> int:
    """vc_image_compare_scratch_bytes (host-only): the device scratch one comparison of two [Cn, H, W] images needs"""
    n = C.c_int64()
    _check(lib().vc_image_compare_scratch_bytes(int(Cn), int(H), int(W), C.byref(n)), "vc_image_compare_scratch_bytes")
    return n.value


def image_form(a, b):
    """(form, C, H, W) of two images vc_image_compare takes: both uint8 [H, W, C] (what pixels_out(uint8=True) writes) or both f32
    [C, H, W] in [0, 1], contiguous, of one shape, on one CUDA device.  ValueError otherwise."""
    for name, t in (("a", a), ("b", b)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"image_compare: {name} must be a torch tensor, got {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"image_compare: {name} must live on a CUDA device, got {t.device}")
        if t.dim() != 3:
            raise ValueError(f"image_compare: {name} must have 3 dimensions ([H, W, C] uint8 or [C, H, W] float32), got shape {tuple(t.shape)}")
        if t.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"image_compare: {name} must be uint8 or float32, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"image_compare: {name} must be contiguous")
    if a.dtype != b.dtype:
        raise ValueError(f"image_compare: a is {a.dtype} and b is {b.dtype}: both images must have one form")
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"image_compare: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
    if a.device != b.device:
        raise ValueError(f"image_compare: devices differ: {a.device} and {b.device}")
    if a.dtype == torch.uint8:
        H, W, Cn = (int(d) for d in a.shape)
        form = IMG_U8_HWC
    else:
        Cn, H, W = (int(d) for d in a.shape)
        form = IMG_F32_CHW
    if H < 11 or W < 11:
        raise ValueError(f"image_compare: a {H}x{W} image is smaller than the 11 x 11 SSIM window")
    return form, Cn, H, W


def image_compare_raw(a, b, out=None, scratch=None, stream=None) -> torch.Tensor:
    """vc_image_compare: the VcImageMetrics of (a, b) as 48 bytes of device memory (uint8 [48]); nothing is read back, so the call
    may be captured.  `out` (uint8 [48]) and `scratch` (uint8, image_compare_scratch_bytes of it) may be the caller's."""
    form, Cn, H, W = image_form(a, b)
    need = image_compare_scratch_bytes(Cn, H, W)
    if out is None:
        out = torch.empty(C.sizeof(ImageMetrics), dtype=torch.uint8, device=a.device)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=a.device)
    for name, t, nbytes in (("out", out, C.sizeof(ImageMetrics)), ("scratch", scratch, need)):
        if t.dtype != torch.uint8 or t.dim() != 1 or t.numel() < nbytes or not t.is_contiguous() or t.device != a.device or t.data_ptr() % 16:
            raise ValueError(f"image_compare: {name} must be a contiguous 16-byte aligned uint8 tensor of at least {nbytes} bytes on {a.device}")
    _check(lib().vc_image_compare(a.data_ptr(), b.data_ptr(), form, Cn, H, W, out.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                  stream if stream is not None else cur_stream()), "vc_image_compare")
    return out


def image_metrics_of(raw: torch.Tensor) -> dict:
    """the dict of a copied-back VcImageMetrics: psnr_db is vc_image_psnr's double, mse = sse / n"""
    m = ImageMetrics.from_buffer_copy(bytes(raw.cpu().numpy().tobytes()[:C.sizeof(ImageMetrics)]))
    sse = float(m.sse_u64) if m.form == IMG_U8_HWC else float(m.sse_f32)
    psnr = C.c_double()
    _check(lib().vc_image_psnr(C.byref(m), C.byref(psnr)), "vc_image_psnr")
    return {"psnr_db": psnr.value, "ssim": float(m.ssim_mean), "mse": sse / float(m.n),
            "max_abs": float(m.max_abs), "n_diff": int(m.n_diff), "sse": int(m.sse_u64) if m.form == IMG_U8_HWC else float(m.sse_f32),
            "n": int(m.n), "n_windows": int(m.n_windows), "form": int(m.form)}


def image_compare(a, b, stream=None) -> dict:
    """How far two renderings lie apart (include/vcloze_hip.h: IMAGE COMPARE): {"psnr_db", "ssim", "mse", "max_abs", "n_diff", ...} of two
    uint8 [H, W, C] or two f32 [C, H, W] images of one shape on one device.  The form is inferred from the dtype.  Synchronises: the
    48-byte result is copied back."""
    return image_metrics_of(image_compare_raw(a, b, stream=stream))


# ---- the photo front end: resampling (csrc/resample.hip), pixels in (csrc/pixels_in.hip), the size rules (csrc/grid_rules.hip) ----
def _filter(f) -> int:
    if f in FILTERS:
        return FILTERS[f]
    if f in FILTERS.values():
        return int(f)
    raise VclozeHipError(f"unknown filter {f!r}: 'bicubic' or 'lanczos' expected")


def resample_coeffs(n_in: int, n_out: int, filter="bicubic"):
    """vc_resample_coeffs (host-only): the tables of one axis as int32 CPU tensors (xmin [out], len [out], ki [out, kmax])"""
    f = _filter(filter)
    kmax = lib().vc_resample_kmax(int(n_in), int(n_out), f)
    _check(0 if kmax >= 0 else kmax, "vc_resample_kmax")
    xmin, ln = torch.empty(n_out, dtype=torch.int32), torch.empty(n_out, dtype=torch.int32)
    ki = torch.empty(n_out, kmax, dtype=torch.int32)
    ip = lambda t: C.cast(t.data_ptr(), C.POINTER(C.c_int32))  # noqa: E731
    _check(lib().vc_resample_coeffs(int(n_in), int(n_out), f, ip(xmin), ip(ln), ip(ki), kmax), "vc_resample_coeffs")
    return xmin, ln, ki


def resample_u8(img, size, filter="bicubic", out=None, stream=None):
    """vc_resample_u8: img [H, W, 3] uint8 on the device resized to size = (w, h) - PIL's order - as [h, w, 3] uint8, byte for byte
    what PIL.Image.resize gives with BICUBIC / LANCZOS."""
    if img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8 or not img.is_cuda or not img.is_contiguous():
        raise VclozeHipError(f"resample_u8: a contiguous CUDA [H, W, 3] uint8 image expected, got {img.dtype} {tuple(img.shape)} on {img.device}")
    H, W = int(img.shape[0]), int(img.shape[1])
    w, h = int(size[0]), int(size[1])
    f = _filter(filter)
    need = lib().vc_resample_tmp_bytes(H, W, h, w, f)
    _check(0 if need >= 0 else int(need), "vc_resample_tmp_bytes")
    if out is None:
        out = torch.empty(h, w, 3, dtype=torch.uint8, device=img.device)
    if tuple(out.shape) != (h, w, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != img.device:
        raise VclozeHipError(f"resample_u8: out must be a contiguous uint8 tensor of shape {(h, w, 3)} on {img.device}")
    tmp = torch.empty(need + 256, dtype=torch.uint8, device=img.device)
    base = (tmp.data_ptr() + 255) & ~255
    _check(lib().vc_resample_u8(img.data_ptr(), H, W, out.data_ptr(), h, w, f, base, need, stream if stream is not None else cur_stream()),
           "vc_resample_u8")
    return out


def pixels_in(img, size, left: int = 0, top: int = 0, out=None, x0: int = 0, dtype=torch.bfloat16, stream=None):
    """vc_pixels_in: the window of size = (w, h) at (left, top) of img [H, W, 3] uint8 (it may reach outside: 0 there; img None: the
    blank cell) as ToTensor + Normalize(0.5, 0.5) give it, written to the columns [x0, x0 + w) of `out` [3, h, Wrow] (bf16 or f32;
    None: a new [3, h, w] tensor of `dtype`).  Returns out."""
    w, h = int(size[0]), int(size[1])
    if img is not None and (img.dim() != 3 or img.shape[2] != 3 or img.dtype != torch.uint8 or not img.is_cuda or not img.is_contiguous()):
        raise VclozeHipError(f"pixels_in: a contiguous CUDA [H, W, 3] uint8 image expected, got {img.dtype} {tuple(img.shape)} on {img.device}")
    if out is None:
        out = torch.empty(3, max(h, 0), max(w, 0), dtype=dtype, device=img.device if img is not None else "cuda")
    if out.dim() != 3 or out.shape[0] != 3 or out.shape[1] != h or out.dtype not in (torch.bfloat16, torch.float32) or not out.is_cuda \
            or not out.is_contiguous():
        raise VclozeHipError(f"pixels_in: out must be a contiguous CUDA [3, {h}, Wrow] bf16 / f32 tensor, got {out.dtype} {tuple(out.shape)}")
    H, W = (int(img.shape[0]), int(img.shape[1])) if img is not None else (0, 0)
    _check(lib().vc_pixels_in(None if img is None else img.data_ptr(), H, W, int(left), int(top), out.data_ptr(), int(out.dtype == torch.float32),
                              h, int(out.shape[2]), int(x0), w, stream if stream is not None else cur_stream()), "vc_pixels_in")
    return out


def mask_fill(mask, x0: int, w: int, value: int, stream=None):
    """vc_mask_fill: the columns [x0, x0 + w) of the bf16 pixel mask [h, Wrow] set to 0 or 1"""
    if mask.dim() != 2 or mask.dtype != torch.bfloat16 or not mask.is_cuda or not mask.is_contiguous():
        raise VclozeHipError(f"mask_fill: a contiguous CUDA [h, Wrow] bf16 mask expected, got {mask.dtype} {tuple(mask.shape)}")
    _check(lib().vc_mask_fill(mask.data_ptr(), int(mask.shape[0]), int(mask.shape[1]), int(x0), int(w), int(value),
                              stream if stream is not None else cur_stream()), "vc_mask_fill")
    return mask


def fit_size(w: int, h: int, resolution: int):
    """vc_fit_size (host-only): the (w, h) an image of w x h is fitted to at `resolution`"""
    a, b = C.c_int32(), C.c_int32()
    _check(lib().vc_fit_size(int(w), int(h), int(resolution), C.byref(a), C.byref(b)), "vc_fit_size")
    return a.value, b.value


def grid_layout(sizes, resolution: int):
    """vc_grid_layout (host-only): sizes[i][j] = (w, h) of the image in row i, column j, or None where it is absent; returns the
    CellPlan of every cell, rows of lists"""
    gh, gw = len(sizes), len(sizes[0]) if sizes else 0
    if any(len(r) != gw for r in sizes):
        raise VclozeHipError("grid_layout: every row must hold the same number of cells")
    flat = [c for r in sizes for c in r]
    n = max(len(flat), 1)
    ws = (C.c_int32 * n)(*[0 if c is None else int(c[0]) for c in flat])
    hs = (C.c_int32 * n)(*[0 if c is None else int(c[1]) for c in flat])
    out = (CellPlan * n)()
    _check(lib().vc_grid_layout(gh, gw, ws, hs, int(resolution), out), "vc_grid_layout")
    return [[out[i * gw + j] for j in range(gw)] for i in range(gh)]


def upsampling_size(target_size):
    """vc_upsampling_size (host-only): pipeline.upsampling_size - (w, h) or None in, (w, h) out"""
    w, h = (0, 0) if target_size is None else (int(target_size[0]), int(target_size[1]))
    a, b = C.c_int32(), C.c_int32()
    _check(lib().vc_upsampling_size(w, h, C.byref(a), C.byref(b)), "vc_upsampling_size")
    return a.value, b.value


# ---- noise source (csrc/rng.hip): the library's own counter-based Gaussian stream (torch's is `randn_torch` below) ----
RNG_BF16, RNG_F32, RNG_U32 = 0, 1, 2                        # VC_RNG_*
RNG_MAX_BLOCKS = 2048                                       # workgroups of 256 threads per launch; a grid-stride loop takes the rest
_RNG_DTYPES = {torch.bfloat16: RNG_BF16, torch.float32: RNG_F32, torch.int32: RNG_U32}


def _u64(v, name: str) -> int:
    v = int(v)
    if not 0 <= v < 1 << 64:
        raise VclozeHipError(f"{name} = {v}: an unsigned 64-bit value expected")
    return v


def randn(shape, seed, offset=0, dtype=torch.bfloat16, device=None, out=None, stream=None):
    """vc_randn: elements offset .. offset + numel of the Gaussian stream of `seed` (include/vcloze_hip.h has the contract: Philox4x32-10
    + Box-Muller in f32; every element depends on (seed, position) only).  dtype: torch.bfloat16 (the f32 normal rounded to
    nearest-even), torch.float32, or torch.int32 = the raw 32-bit Philox words (VC_RNG_U32, for exact tests).  `out`: a contiguous
    device tensor to fill instead of a new one (any base aligned to its element size; `shape` may be None).  Captured in a graph, a
    replay repeats the same noise."""
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device if device is not None else "cuda")
    elif shape is not None and tuple(out.shape) != tuple(shape):
        raise VclozeHipError(f"randn: out has shape {tuple(out.shape)}, not {tuple(shape)}")
    if out.dtype not in _RNG_DTYPES or not out.is_cuda or not out.is_contiguous():
        raise VclozeHipError(f"randn: a contiguous CUDA bf16 / f32 / int32 tensor expected, got {out.dtype} on {out.device}")
    if stream is None and out.device.index != torch.cuda.current_device():
        raise VclozeHipError(f"randn: the tensor is on {out.device}, the current stream on cuda:{torch.cuda.current_device()}")
    _check(lib().vc_randn(out.data_ptr(), _RNG_DTYPES[out.dtype], out.numel(), _u64(seed, "seed"), _u64(offset, "offset"),
                          stream if stream is not None else cur_stream()), "vc_randn")
    return out


def randn_tokens(C_, h, w, seed, offset=0, tokens=None, col0=0, device=None, stream=None):
    """vc_randn_tokens: a [C_, h, w] draw at stream positions offset + (c*h + y)*w + x, written as bf16 into tokens[:, col0:col0+4C_]
    in pack_latent's layout - bit-identical to pack_latent(randn([C_, h, w], seed, offset), tokens, col0) in one launch.  tokens:
    [(h/2)(w/2), >= col0 + 4C_] bf16 rows (last dim contiguous), or None for a new [(h/2)(w/2), 4C_] tensor.  Returns tokens."""
    if tokens is None:
        tokens = torch.empty((h // 2) * (w // 2), col0 + 4 * C_, dtype=torch.bfloat16, device=device if device is not None else "cuda")
    _bf16(tokens, "tokens")
    if tokens.dim() != 2 or tokens.stride(1) != 1 or tokens.shape[0] != (h // 2) * (w // 2) or tokens.shape[1] < col0 + 4 * C_:
        raise VclozeHipError(f"randn_tokens: [(h/2)(w/2), >= col0 + 4C] token rows with contiguous last dim expected, got {tuple(tokens.shape)}")
    if stream is None and tokens.device.index != torch.cuda.current_device():
        raise VclozeHipError(f"randn_tokens: the tensor is on {tokens.device}, the current stream on cuda:{torch.cuda.current_device()}")
    _check(lib().vc_randn_tokens(tokens.data_ptr(), C_, h, w, tokens.stride(0), col0, _u64(seed, "seed"), _u64(offset, "offset"),
                                 stream if stream is not None else cur_stream()), "vc_randn_tokens")
    return tokens


# ---- noise source, opt-in (csrc/rng_torch.hip): torch's device generator stream, bit for bit ----
NOISE_OWN, NOISE_TORCH = 0, 1                               # VC_NOISE_*


def torch_randn_policy(n, sm_count=0, threads_per_sm=0):
    """vc_torch_randn_policy (host-only): (G, advance) - the blocks of 256 threads torch.randn launches for n elements on a device of
    `sm_count` multiprocessors and `threads_per_sm` threads each, and what the generator's Philox offset advances by.  0 = the
    current device's value (only then is a device needed)."""
    g, adv = C.c_int32(0), C.c_uint64(0)
    _check(lib().vc_torch_randn_policy(int(n), int(sm_count), int(threads_per_sm), C.byref(g), C.byref(adv)), "vc_torch_randn_policy")
    return g.value, adv.value


def randn_torch(shape, seed, offset=0, dtype=torch.bfloat16, device=None, sm_count=0, threads_per_sm=0, out=None, stream=None):
    """vc_randn_torch: what torch.randn(shape, device=device, generator=G) gives for a generator of `seed` standing at Philox offset
    `offset` (a multiple of 4, `G.get_offset()`), bit for bit (include/vcloze_hip.h, THE TORCH STREAM).  dtype: torch.float32,
    torch.bfloat16 (= the f32 draw .to(bfloat16)), or torch.int32 = the raw Philox words.  The caller advances its offset
    (`torch_randn_policy`).  sm_count / threads_per_sm: another device's properties instead of the current one's."""
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device if device is not None else "cuda")
    elif shape is not None and tuple(out.shape) != tuple(shape):
        raise VclozeHipError(f"randn_torch: out has shape {tuple(out.shape)}, not {tuple(shape)}")
    if out.dtype not in _RNG_DTYPES or not out.is_cuda or not out.is_contiguous():
        raise VclozeHipError(f"randn_torch: a contiguous CUDA bf16 / f32 / int32 tensor expected, got {out.dtype} on {out.device}")
    if out.device.index != torch.cuda.current_device():          # the grid cap is the CURRENT device's
        raise VclozeHipError(f"randn_torch: the tensor is on {out.device}, the current device is cuda:{torch.cuda.current_device()}")
    _check(lib().vc_randn_torch(out.data_ptr(), _RNG_DTYPES[out.dtype], out.numel(), _u64(seed, "seed"), _u64(offset, "offset"),
                                int(sm_count), int(threads_per_sm), stream if stream is not None else cur_stream()), "vc_randn_torch")
    return out


def randn_torch_tokens(C_, h, w, seed, offset=0, tokens=None, col0=0, device=None, sm_count=0, threads_per_sm=0, stream=None):
    """vc_randn_torch_tokens: the [C_, h, w] draw of `randn_torch` written as bf16 into tokens[:, col0:col0+4C_] in pack_latent's
    layout, in one launch; `tokens` as in `randn_tokens`.  Returns tokens."""
    if tokens is None:
        tokens = torch.empty((h // 2) * (w // 2), col0 + 4 * C_, dtype=torch.bfloat16, device=device if device is not None else "cuda")
    _bf16(tokens, "tokens")
    if tokens.dim() != 2 or tokens.stride(1) != 1 or tokens.shape[0] != (h // 2) * (w // 2) or tokens.shape[1] < col0 + 4 * C_:
        raise VclozeHipError(f"randn_torch_tokens: [(h/2)(w/2), >= col0 + 4C] token rows with contiguous last dim expected, got {tuple(tokens.shape)}")
    if tokens.device.index != torch.cuda.current_device():
        raise VclozeHipError(f"randn_torch_tokens: the tensor is on {tokens.device}, the current device is cuda:{torch.cuda.current_device()}")
    _check(lib().vc_randn_torch_tokens(tokens.data_ptr(), C_, h, w, tokens.stride(0), col0, _u64(seed, "seed"), _u64(offset, "offset"),
                                       int(sm_count), int(threads_per_sm), stream if stream is not None else cur_stream()), "vc_randn_torch_tokens")
    return tokens


# ---- VAE decoder glue (activations NHWC bf16 [H*W, C]) ----
def im2col3x3(src, dst, H, W, up=False, down=False, stream=None):
    """(H, W) is the OUTPUT map; `up`: src is the half-resolution map (nearest 2x folded in); `down`: src is the
    double-resolution map (pad (0,1,0,1) + stride 2)."""
    _bf16(src, "src"); _bf16(dst, "dst")
    Cc = src.shape[1]
    hs, ws = (H >> 1, W >> 1) if up else (2 * H, 2 * W) if down else (H, W)
    if (up and down) or src.shape[0] != hs * ws or tuple(dst.shape) != (H * W, 9 * Cc) or not (src.is_contiguous() and dst.is_contiguous()):
        raise VclozeHipError("im2col3x3: src [Hs*Ws, C] and dst [H*W, 9C] contiguous expected")
    _check(lib().vc_im2col3x3(src.data_ptr(), dst.data_ptr(), H, W, Cc, 1 if up else 2 if down else 0,
                              stream if stream is not None else cur_stream()), "vc_im2col3x3")


def conv3x3(x, w, bias, out, H, W, up=False, down=False, res=None, gate=None, stream=None):
    """One-launch 3x3 convolution (implicit GEMM).  x: [Hs*Ws + 1, C] NHWC map whose last row is zero; w [O, 9C];
    out [H*W, O]; optional residual: out = res + gate * (conv + bias)."""
    _bf16(x, "x"); _bf16(w, "w"); _bf16(out, "out")
    Cc, O = x.shape[1], w.shape[0]
    hs, ws = (H >> 1, W >> 1) if up else (2 * H, 2 * W) if down else (H, W)
    if (up and down) or x.shape[0] != hs * ws + 1 or not x.is_contiguous() or w.shape[1] != 9 * Cc or not w.is_contiguous() \
            or tuple(out.shape) != (H * W, O) or out.stride(1) != 1:
        raise VclozeHipError("conv3x3: x [Hs*Ws + 1, C] (last row zero), w [O, 9C], out [H*W, O] expected")
    if res is not None:
        if gate is None:
            raise VclozeHipError("conv3x3: res needs a gate")
        _bf16(res, "res"); _bf16(gate, "gate")
    _check(lib().vc_conv3x3(x.data_ptr(), w.data_ptr(), _p(bias), out.data_ptr(), out.stride(0), _p(res),
                            res.stride(0) if res is not None else 0, _p(gate), H, W, Cc, O, 1 if up else 2 if down else 0,
                            stream if stream is not None else cur_stream()), "vc_conv3x3")


def groupnorm(x, gamma, beta, y, scratch, groups=32, eps=1e-6, swish=False, stream=None):
    _bf16(x, "x"); _bf16(y, "y"); _bf16(gamma, "gamma"); _bf16(beta, "beta")
    HW, Cc = x.shape
    if not (x.is_contiguous() and y.is_contiguous()) or y.shape != x.shape or scratch.dtype != torch.float32:
        raise VclozeHipError("groupnorm: contiguous [HW, C] x, y and an f32 scratch tensor expected")
    _check(lib().vc_groupnorm(x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), scratch.data_ptr(),
                              scratch.numel() * 4, HW, Cc, groups, eps, int(bool(swish)),
                              stream if stream is not None else cur_stream()), "vc_groupnorm")


def groupnorm_scratch_floats(HW, groups=32):
    return ((HW + 127) // 128 + 1) * 2 * groups


def softmax_rows(x, scale, bias=None, causal_period=0, stream=None):
    _bf16(x, "x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise VclozeHipError("softmax_rows: 2-D tensor with contiguous rows expected")
    ldb = 0
    if bias is not None:
        _bf16(bias, "bias")
        if bias.dim() != 2 or bias.stride(1) != 1 or bias.shape != x.shape:
            raise VclozeHipError("softmax_rows: bias must match x")
        ldb = bias.stride(0)
    _check(lib().vc_softmax_rows(x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], scale, _p(bias), ldb, causal_period,
                                 stream if stream is not None else cur_stream()), "vc_softmax_rows")


# ---- text-encoder glue ----
def embedding(ids, table, out, stream=None):
    _bf16(table, "table"); _bf16(out, "out")
    if ids.dtype != torch.int32 or not ids.is_cuda or ids.dim() != 1 or not ids.is_contiguous():
        raise VclozeHipError("embedding: ids must be a contiguous CUDA int32 vector")
    if table.stride(1) != 1 or not out.is_contiguous() or tuple(out.shape) != (ids.shape[0], table.shape[1]):
        raise VclozeHipError("embedding: out [L, D] contiguous expected")
    _check(lib().vc_embedding(ids.data_ptr(), table.data_ptr(), table.stride(0), table.shape[0], out.data_ptr(), ids.shape[0],
                              table.shape[1], stream if stream is not None else cur_stream()), "vc_embedding")


def rmsnorm(x, weight, y, eps, stream=None):
    _bf16(x, "x"); _bf16(weight, "weight"); _bf16(y, "y")
    if not (x.is_contiguous() and y.is_contiguous()) or x.shape != y.shape or weight.numel() != x.shape[1]:
        raise VclozeHipError("rmsnorm: contiguous [rows, D] x, y and weight [D] expected")
    _check(lib().vc_rmsnorm(x.data_ptr(), weight.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], eps,
                            stream if stream is not None else cur_stream()), "vc_rmsnorm")


def layernorm(x, weight, bias, y, eps, stream=None):
    _bf16(x, "x"); _bf16(weight, "weight"); _bf16(bias, "bias"); _bf16(y, "y")
    if not (x.is_contiguous() and y.is_contiguous()) or x.shape != y.shape or weight.numel() != x.shape[1]:
        raise VclozeHipError("layernorm: contiguous [rows, D] x, y and weight/bias [D] expected")
    _check(lib().vc_layernorm(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], eps,
                              stream if stream is not None else cur_stream()), "vc_layernorm")


def _ew(fn, name, a, b, y, stream):
    for t in (a, b, y):
        if t is not None:
            _bf16(t, name)
            if not t.is_contiguous() or t.numel() != y.numel():
                raise VclozeHipError(f"{name}: contiguous tensors of equal size expected")
    args = [a.data_ptr()] + ([b.data_ptr()] if b is not None else []) + [y.data_ptr(), y.numel(), stream if stream is not None else cur_stream()]
    _check(fn(*args), name)


def mul(a, b, y, stream=None):
    _ew(lib().vc_mul, "vc_mul", a, b, y, stream)


def add(a, b, y, stream=None):
    _ew(lib().vc_add, "vc_add", a, b, y, stream)


def quick_gelu(x, y, stream=None):
    _ew(lib().vc_quick_gelu, "vc_quick_gelu", x, None, y, stream)


def t5_relative_buckets(L: int, num_buckets: int, max_distance: int) -> list:
    """vc_t5_relative_buckets: the 2L - 1 bucket ids of relative positions -(L-1) .. L-1 (no GPU needed)"""
    out = (C.c_int32 * (2 * L - 1))()
    _check(lib().vc_t5_relative_buckets(L, num_buckets, max_distance, out), "vc_t5_relative_buckets")
    return list(out)


def t5_position_bias(table, L: int, max_distance: int, out=None, stream=None):
    """table: relative_attention_bias.weight [num_buckets, H] bf16 -> out [H * L, L] bf16, out[h * L + i, j] = table[bucket(j - i), h]"""
    _bf16(table, "table")
    if table.dim() != 2 or table.stride(1) != 1:
        raise VclozeHipError("t5_position_bias: table [num_buckets, H] with contiguous rows expected")
    nb, H = table.shape
    out = torch.empty(H * L, L, dtype=torch.bfloat16, device=table.device) if out is None else out
    _bf16(out, "out")
    if tuple(out.shape) != (H * L, L) or not out.is_contiguous():
        raise VclozeHipError("t5_position_bias: contiguous out [H * L, L] expected")
    _check(lib().vc_t5_position_bias(table.data_ptr(), table.stride(0), H, L, nb, max_distance, out.data_ptr(),
                                     stream if stream is not None else cur_stream()), "vc_t5_position_bias")
    return out


def clip_embed(ids, tok, pos, out, stream=None):
    """ids [L] int32, tok [vocab, D], pos [>= L, D], out [Lp >= L, D]: rows < L = tok[ids] + pos, the rest tok[0]"""
    _bf16(tok, "tok"); _bf16(pos, "pos"); _bf16(out, "out")
    if ids.dtype != torch.int32 or not ids.is_cuda or ids.dim() != 1 or not ids.is_contiguous():
        raise VclozeHipError("clip_embed: ids must be a contiguous CUDA int32 vector")
    L, D = ids.shape[0], tok.shape[1]
    if tok.stride(1) != 1 or pos.stride(1) != 1 or pos.shape[0] < L or pos.shape[1] != D or not out.is_contiguous() or out.shape[1] != D \
            or out.shape[0] < L:
        raise VclozeHipError("clip_embed: tok [V, D], pos [>= L, D] and contiguous out [Lp >= L, D] expected")
    _check(lib().vc_clip_embed(ids.data_ptr(), tok.data_ptr(), tok.stride(0), tok.shape[0], pos.data_ptr(), pos.stride(0), out.data_ptr(),
                               L, out.shape[0], D, stream if stream is not None else cur_stream()), "vc_clip_embed")


def clip_pool(ids, hidden, eos_token_id: int, pooled=None, stream=None):
    """pooled [D] = hidden[first i with ids[i] == eos_token_id, or 0]; hidden [>= L, D] rows"""
    _bf16(hidden, "hidden")
    if ids.dtype != torch.int32 or not ids.is_cuda or ids.dim() != 1 or not ids.is_contiguous():
        raise VclozeHipError("clip_pool: ids must be a contiguous CUDA int32 vector")
    if hidden.dim() != 2 or hidden.stride(1) != 1 or hidden.shape[0] < ids.shape[0]:
        raise VclozeHipError("clip_pool: hidden [>= L, D] with contiguous rows expected")
    pooled = torch.empty(hidden.shape[1], dtype=torch.bfloat16, device=hidden.device) if pooled is None else pooled
    _bf16(pooled, "pooled")
    if tuple(pooled.shape) != (hidden.shape[1],) or not pooled.is_contiguous():
        raise VclozeHipError("clip_pool: contiguous pooled [D] expected")
    _check(lib().vc_clip_pool(ids.data_ptr(), hidden.data_ptr(), hidden.stride(0), ids.shape[0], hidden.shape[1], int(eos_token_id),
                              pooled.data_ptr(), stream if stream is not None else cur_stream()), "vc_clip_pool")
    return pooled


def transpose(src, dst, stream=None):
    _bf16(src, "src"); _bf16(dst, "dst")
    if src.dim() != 2 or src.stride(1) != 1 or dst.stride(1) != 1 or tuple(dst.shape) != (src.shape[1], src.shape[0]):
        raise VclozeHipError("transpose: [R, C] -> [C, R] with contiguous rows expected")
    _check(lib().vc_transpose(src.data_ptr(), src.stride(0), dst.data_ptr(), dst.stride(0), src.shape[0], src.shape[1],
                              stream if stream is not None else cur_stream()), "vc_transpose")


def nchw_to_nhwc(src, dst, div=1.0, add=0.0, stream=None):
    _bf16(dst, "dst")
    if src.dtype not in (torch.float32, torch.bfloat16) or not (src.is_contiguous() and dst.is_contiguous()):
        raise VclozeHipError("nchw_to_nhwc: contiguous f32/bf16 [C, H, W] source expected")
    Cc, HW = src.shape[0], src[0].numel()
    if dst.shape[0] != HW or dst.shape[1] < Cc:
        raise VclozeHipError("nchw_to_nhwc: dst [H*W, Cp >= C] expected")
    _check(lib().vc_nchw_to_nhwc(src.data_ptr(), int(src.dtype == torch.float32), dst.data_ptr(), Cc, dst.shape[1], HW,
                                 div, add, stream if stream is not None else cur_stream()), "vc_nchw_to_nhwc")


def nhwc_to_nchw(src, dst, stream=None):
    _bf16(src, "src")
    if dst.dtype not in (torch.float32, torch.bfloat16) or not (src.is_contiguous() and dst.is_contiguous()):
        raise VclozeHipError("nhwc_to_nchw: contiguous f32/bf16 [C, H, W] destination expected")
    Cc, HW = dst.shape[0], dst[0].numel()
    if src.shape[0] != HW or src.shape[1] < Cc:
        raise VclozeHipError("nhwc_to_nchw: src [H*W, Cp >= C] expected")
    _check(lib().vc_nhwc_to_nchw(src.data_ptr(), dst.data_ptr(), int(dst.dtype == torch.float32), Cc, src.shape[1], HW,
                                 stream if stream is not None else cur_stream()), "vc_nhwc_to_nchw")


def gaussian_sample(moments, noise, out, scale, shift, stream=None):
    _bf16(moments, "moments"); _bf16(out, "out")
    Z, HW = out.shape[0], out[0].numel()
    if noise is not None:
        _bf16(noise, "noise")
        if noise.shape != out.shape or not noise.is_contiguous():
            raise VclozeHipError("gaussian_sample: noise must match out [Z, h, w]")
    if moments.shape[0] != HW or moments.shape[1] < 2 * Z or not (moments.is_contiguous() and out.is_contiguous()):
        raise VclozeHipError("gaussian_sample: moments [H*W, Cp >= 2Z] and contiguous out [Z, h, w] expected")
    _check(lib().vc_gaussian_sample(moments.data_ptr(), moments.shape[1], _p(noise), out.data_ptr(), Z, HW, scale, shift,
                                    stream if stream is not None else cur_stream()), "vc_gaussian_sample")


class Graph:
    """hipGraph captured from the launches issued on `stream` inside the with-block."""

    def __init__(self, stream: int):
        self.stream = stream
        self.exec = C.c_void_p()

    def __enter__(self):
        _check(lib().vc_graph_begin(self.stream), "vc_graph_begin")
        return self

    def __exit__(self, et, ev, tb):
        rc = lib().vc_graph_end(self.stream, C.byref(self.exec))
        if et is None:
            _check(rc, "vc_graph_end")
        return False

    def launch(self, stream: Optional[int] = None):
        _check(lib().vc_graph_launch(self.exec, stream if stream is not None else self.stream), "vc_graph_launch")

    def __del__(self):
        try:
            if self.exec:
                lib().vc_graph_destroy(self.exec)
        except Exception:
            pass


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().vc_event_create(C.byref(self.h)), "vc_event_create")

    def record(self, stream=None):
        _check(lib().vc_event_record(self.h, stream if stream is not None else cur_stream()), "vc_event_record")

    def elapsed_ms(self, stop: "Event") -> float:
        ms = C.c_float()
        _check(lib().vc_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "vc_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            lib().vc_event_destroy(self.h)
        except Exception:
            pass
