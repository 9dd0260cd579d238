"""ctypes binding of ``libanemoi_amd.so`` -- the C ABI declared in ``include/anemoi_amd.h``.

There is no CPU fallback: if the library is missing or a kernel call fails the caller gets an
exception.  The product path never routes through ``oracle/``.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p
from ctypes import c_float
from ctypes import c_int
from ctypes import c_int64
from ctypes import c_uint32
from ctypes import c_void_p

import torch  # noqa: F401  -- FIRST: puts torch's bundled HIP runtime (libamdhip64.so.7) in the process so that
#                        this library binds to the same runtime instance that owns torch's device memory

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libanemoi_amd.so")

ANEMOI_OK = 0
ANEMOI_ERR_INVALID = 1
ANEMOI_ERR_UNSUPPORTED = 2
ANEMOI_ERR_LAUNCH = 3

F32 = 0
BF16 = 1
I32 = 2  # launch-trail records only
U8 = 3

ACT_NONE, ACT_GELU, ACT_SILU, ACT_RELU = 0, 1, 2, 3
ACT_CODES = {"Identity": ACT_NONE, "GELU": ACT_GELU, "SiLU": ACT_SILU, "ReLU": ACT_RELU}

LOSS_MSE, LOSS_MAE, LOSS_HUBER, LOSS_LOGCOSH = 0, 1, 2, 3
LOSS_KINDS = {"mse": LOSS_MSE, "mae": LOSS_MAE, "huber": LOSS_HUBER, "logcosh": LOSS_LOGCOSH}

ENS_AFCRPS, ENS_MEAN_SE, ENS_VARIANCE = 0, 1, 2
ENS_KINDS = {"afcrps": ENS_AFCRPS, "mean_se": ENS_MEAN_SE, "variance": ENS_VARIANCE}
ENS_MAX_MEMBERS = 16

HEAD_NORM_MAX_D = 128  # the widest head of anemoi_head_norm (HN_MAX_D of csrc/head_norm.hip)
COND_LN_MAX_K = 32  # the fused conditional LayerNorm's widest condition (CLN_MAX_K of csrc/cond_layer_norm.hip)


def cond_ln_padded_k(k: int) -> int:
    """The column count (4, 8, 16 or 32) the fused conditional LayerNorm takes a condition of ``k <= 32`` columns padded to."""
    return 4 if k <= 4 else (8 if k <= 8 else (16 if k <= 16 else 32))


ABI_VERSION = 55

LINEAR_ENTRIES = {"linear": 0, "ln": 1, "stats": 2, "dual": 3, "actgrad": 4, "batched": 5}  # ANEMOI_LINEAR_ENTRY_*
LINEAR_KERNEL_NONE, LINEAR_KERNEL_128, LINEAR_KERNEL_PERSISTENT = 0, 1, 2
LINEAR_REST_NONE, LINEAR_REST_IN_LAUNCH, LINEAR_REST_SKINNY, LINEAR_REST_128 = 0, 1, 2, 3


class LinearArgs(ctypes.Structure):
    """``anemoi_linear_args`` of include/anemoi_amd.h (``anemoi_linear_route``), field for field."""

    _fields_ = [
        ("struct_bytes", c_int64),
        ("entry", ctypes.c_int32), ("dtype", ctypes.c_int32), ("out_dtype", ctypes.c_int32), ("act", ctypes.c_int32),
        ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("colsum", c_void_p), ("stats", c_void_p),
        ("residual", c_void_p), ("y", c_void_p),
        ("ldx", c_int64), ("ldr", c_int64), ("ldy", c_int64), ("M", c_int64),
        ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("workspace", c_void_p), ("workspace_bytes", c_int64), ("stats_out", c_void_p),
        ("stride_x", c_int64), ("stride_w", c_int64), ("stride_y", c_int64),
        ("batch", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LinearRouteLaunch(ctypes.Structure):
    """``anemoi_linear_route_launch``: one launch of the persistent kernel."""

    _fields_ = [
        ("row0", c_int64), ("rows", c_int64), ("tiles", c_int64),
        ("mh", ctypes.c_int32), ("blocks", ctypes.c_int32), ("tail_rows", ctypes.c_int32),
        ("stagger_phases", ctypes.c_int32), ("stagger_unit", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class LinearRoute(ctypes.Structure):
    """``anemoi_linear_route_info``: what the fused Linear family does with a call (the library's own plan)."""

    _fields_ = [
        ("struct_bytes", c_int64),
        ("kernel", ctypes.c_int32), ("n_launches", ctypes.c_int32),
        ("launch", LinearRouteLaunch * 2),
        ("main_rows", c_int64),
        ("rest", ctypes.c_int32), ("nt", ctypes.c_int32),
        ("rest_row0", c_int64), ("rest_rows", c_int64), ("rs_rows", c_int64),
        ("vec_ok", ctypes.c_int32), ("split", ctypes.c_int32), ("model", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


def linear_route(entry: str, **fields):
    """``(status, LinearRoute)`` of ``anemoi_linear_route`` for the arguments ``fields`` of entry point ``entry`` (pointers as
    integers; whatever is left out is 0 / NULL).  Launches nothing and needs no GPU: for tests and diagnostics."""
    args, route = LinearArgs(), LinearRoute()
    args.struct_bytes, route.struct_bytes = ctypes.sizeof(LinearArgs), ctypes.sizeof(LinearRoute)
    args.entry = LINEAR_ENTRIES[entry]
    for name, value in fields.items():
        setattr(args, name, value)
    return load().anemoi_linear_route(ctypes.byref(args), ctypes.byref(route)), route


MHSA_ENTRIES = {"forward": 0, "backward": 1}  # ANEMOI_MHSA_ENTRY_*
MHSA_KERNEL_GENERIC, MHSA_KERNEL_W8, MHSA_KERNEL_W4, MHSA_KERNEL_BWD_MFMA = 0, 1, 2, 3
MHSA_KERNEL_NAMES = {MHSA_KERNEL_GENERIC: "generic", MHSA_KERNEL_W8: "w8", MHSA_KERNEL_W4: "w4", MHSA_KERNEL_BWD_MFMA: "mfma"}


class MhsaArgs(ctypes.Structure):
    """``anemoi_mhsa_args`` of include/anemoi_amd.h (``anemoi_mhsa_route``), field for field."""

    _fields_ = [
        ("struct_bytes", c_int64),
        ("entry", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("qkv", c_void_p), ("out", c_void_p), ("lse", c_void_p), ("dout", c_void_p), ("delta", c_void_p),
        ("dqkv", c_void_p), ("workspace", c_void_p), ("dropout_seed_dev", c_void_p),
        ("ld", c_int64), ("ldo", c_int64), ("lddo", c_int64), ("lddq", c_int64),
        ("B", ctypes.c_int32), ("S", ctypes.c_int32), ("H", ctypes.c_int32), ("D", ctypes.c_int32),
        ("window", ctypes.c_int32), ("dropout_p", c_float), ("dropout_seed", c_uint32),
        ("dropout_h0", ctypes.c_int32), ("dropout_h_total", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class MhsaLayout(ctypes.Structure):
    """``anemoi_mhsa_workspace_layout``: byte offsets into the workspace, and its size."""

    _fields_ = [(name, c_int64) for name in ("vt", "tail", "flag", "qt", "kt", "dot", "lse2p", "deltap", "total")]


class MhsaRoute(ctypes.Structure):
    """``anemoi_mhsa_route_info``: what self attention does with a call (the library's own plan)."""

    _fields_ = [
        ("struct_bytes", c_int64),
        ("kernel", ctypes.c_int32), ("drop", ctypes.c_int32), ("win", ctypes.c_int32), ("dmax", ctypes.c_int32),
        ("S_pad", ctypes.c_int32), ("tail_rows", ctypes.c_int32), ("tail_splits", ctypes.c_int32),
        ("tail_chunk", ctypes.c_int32),
        ("grid", c_uint32 * 3), ("reserved", ctypes.c_int32),
        ("layout", MhsaLayout),
    ]


def mhsa_route(entry: str, **fields):
    """``(status, MhsaRoute)`` of ``anemoi_mhsa_route`` for the arguments ``fields`` of ``anemoi_mhsa`` (``entry`` "forward") or
    ``anemoi_mhsa_backward`` ("backward"): pointers as integers, whatever is left out is 0 / NULL.  Launches nothing and needs
    no GPU: for tests and diagnostics."""
    args, route = MhsaArgs(), MhsaRoute()
    args.struct_bytes, route.struct_bytes = ctypes.sizeof(MhsaArgs), ctypes.sizeof(MhsaRoute)
    args.entry = MHSA_ENTRIES[entry]
    for name, value in fields.items():
        setattr(args, name, value)
    return load().anemoi_mhsa_route(ctypes.byref(args), ctypes.byref(route)), route


class LinearThinArgs(ctypes.Structure):
    """``anemoi_linear_thin_args`` of include/anemoi_amd.h (``anemoi_linear_thin``), field for field."""

    _fields_ = [
        ("struct_bytes", c_int64),
        ("out_dtype", ctypes.c_int32), ("batch", ctypes.c_int32),
        ("x", c_void_p), ("w", c_void_p), ("bias", c_void_p), ("colsum", c_void_p), ("stats", c_void_p),
        ("residual", c_void_p), ("y", c_void_p), ("stats_out", c_void_p),
        ("ldx", c_int64), ("ldr", c_int64), ("ldy", c_int64), ("M", c_int64),
        ("N", ctypes.c_int32), ("K", ctypes.c_int32),
        ("stride_x", c_int64), ("stride_w", c_int64), ("stride_y", c_int64), ("stride_r", c_int64),
        ("eps", c_float), ("reserved", ctypes.c_int32),
    ]


THIN_SHAPES = ((256, 64), (64, 256), (256, 256), (80, 1024), (16, 1024), (16, 256), (256, 128))  # (N, K) of csrc/gemm_thin_plan.hpp::SHAPES


class GtBlockArgs(ctypes.Structure):
    """``anemoi_gt_block_args`` of include/anemoi_amd.h (block-level entry points), field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_dst", c_int64),
        ("dtype", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("up", ctypes.c_int32),
        ("hidden", ctypes.c_int32), ("act", ctypes.c_int32), ("k_proj", ctypes.c_int32), ("n_in", ctypes.c_int32),
        ("eps_mlp", c_float), ("eps_out", c_float),
        ("x", c_void_p), ("ldx", c_int64), ("x_stats", c_void_p),
        ("w_in", c_void_p), ("b_in", c_void_p), ("cs_in", c_void_p),
        ("sq", c_void_p), ("ld_sq", c_int64),
        ("q", c_void_p), ("k", c_void_p), ("v", c_void_p), ("x_r", c_void_p), ("u", c_void_p),
        ("ldq", c_int64), ("ldkv", c_int64), ("ldr", c_int64), ("ldu", c_int64),
        ("edge_attr", c_void_p), ("rowptr", c_void_p), ("col", c_void_p),
        ("att", c_void_p), ("ld_att", c_int64),
        ("w_proj", c_void_p), ("b_proj", c_void_p), ("res", c_void_p), ("ld_res", c_int64), ("y", c_void_p),
        ("y_stats", c_void_p),
        ("w_fc1", c_void_p), ("b_fc1", c_void_p), ("cs_fc1", c_void_p), ("h", c_void_p),
        ("w_fc2", c_void_p), ("b_fc2", c_void_p), ("out", c_void_p), ("out_stats", c_void_p),
        ("stats_ws", c_void_p), ("stats_ws_bytes", c_int64),
        ("run_ptr", c_void_p), ("run_perm", c_void_p), ("n_runs", c_int64),
        ("sched", c_void_p), ("sched_slots", ctypes.c_int32), ("sched_steps", ctypes.c_int32), ("n_src", c_int64),
        ("run_dst", c_void_p), ("n_edges", c_int64),
        ("tile_hdr", c_void_p), ("tile_dst", c_void_p), ("tile_src", c_void_p), ("tile_slot", c_void_p), ("tile_xcd", c_void_p),
        ("tile_max_per_xcd", ctypes.c_int32), ("tile_src_cap", ctypes.c_int32), ("tile_edge_cap", ctypes.c_int32),
        ("tile_pad", ctypes.c_int32),
    ]

class TfmBlockArgs(ctypes.Structure):
    """``anemoi_tfm_block_args`` of include/anemoi_amd.h (``anemoi_transformer_block_forward``), field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("rows", c_int64),
        ("dtype", ctypes.c_int32), ("B", ctypes.c_int32), ("S", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32),
        ("hidden", ctypes.c_int32), ("act", ctypes.c_int32), ("window", ctypes.c_int32),
        ("eps1", c_float), ("eps2", c_float),
        ("dropout_p", c_float), ("dropout_seed", c_uint32), ("dropout_seed_dev", c_void_p),
        ("dropout_h0", ctypes.c_int32), ("dropout_h_total", ctypes.c_int32),
        ("x", c_void_p), ("ldx", c_int64),
        ("ln1_w", c_void_p), ("ln1_b", c_void_p), ("ln2_w", c_void_p), ("ln2_b", c_void_p),
        ("w_qkv", c_void_p), ("b_qkv", c_void_p), ("w_proj", c_void_p), ("b_proj", c_void_p),
        ("w_fc1", c_void_p), ("b_fc1", c_void_p), ("w_fc2", c_void_p), ("b_fc2", c_void_p),
        ("h_ln", c_void_p), ("qkv", c_void_p), ("att", c_void_p), ("y", c_void_p), ("h", c_void_p),
        ("mhsa_ws", c_void_p), ("out", c_void_p),
    ]


OPT_MAX_TENSORS = 88  # tensors per launch of the multi-tensor optimizer kernels (anemoi_multi_tensor_max_tensors())
OPT_CHUNK = 4096      # elements per workgroup (anemoi_multi_tensor_chunk())
OPT_CONSTS = 8        # floats per block of anemoi_adamw_constants
OPT_SKIP_ALL = 3      # index of the list-wide skip flag in block 0 (norm, clip, finite, skip)
OPT_SUMSQ_DEPTH = OPT_CHUNK // 256 + 6 + 3  # longest chain of f32 additions in anemoi_multi_sumsq (csrc/optim.hip)


class MultiTensorArgs(ctypes.Structure):
    """``anemoi_multi_tensor_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_tensors", c_int64),
        ("numel", c_void_p), ("params", c_void_p), ("grads", c_void_p), ("exp_avg", c_void_p), ("exp_avg_sq", c_void_p),
        ("workspace", c_void_p), ("workspace_floats", c_int64), ("sumsq", c_void_p), ("consts", c_void_p), ("coef", c_void_p),
        ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
    ]


class AdamwConstantsArgs(ctypes.Structure):
    """``anemoi_adamw_constants_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_groups", c_int64),
        ("step", c_void_p), ("lr_dev", c_void_p), ("lr", c_void_p), ("beta1", c_void_p), ("beta2", c_void_p),
        ("weight_decay", c_void_p), ("sumsq", c_void_p), ("skipped", c_void_p), ("consts", c_void_p),
        ("max_norm", c_float), ("has_max_norm", ctypes.c_int32), ("skip_nonfinite", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


AVERAGE_EMA, AVERAGE_SWA = 0, 1  # ANEMOI_AVERAGE_EMA / ANEMOI_AVERAGE_SWA
AVG_CONSTS = 4                    # floats of the block of anemoi_average_constants: w, active, copy, n_after
LR_MAX_GROUPS = 32                # parameter groups per call of anemoi_lr_schedule


class AverageConstantsArgs(ctypes.Structure):
    """``anemoi_average_constants_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_averaged", c_void_p), ("step", c_void_p), ("skip", c_void_p), ("avg", c_void_p),
        ("decay", ctypes.c_double), ("start_step", c_int64), ("every", c_int64),
        ("kind", ctypes.c_int32), ("use_warmup", ctypes.c_int32),
    ]


class MultiAverageArgs(ctypes.Structure):
    """``anemoi_multi_average_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_tensors", c_int64), ("numel", c_void_p), ("params", c_void_p), ("shadow", c_void_p),
        ("avg", c_void_p),
    ]


class MultiSwapArgs(ctypes.Structure):
    """``anemoi_multi_swap_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [("struct_bytes", c_int64), ("n_tensors", c_int64), ("numel", c_void_p), ("a", c_void_p), ("b", c_void_p)]


class LrScheduleArgs(ctypes.Structure):
    """``anemoi_lr_schedule_args`` of include/anemoi_amd.h, field for field."""

    _fields_ = [
        ("struct_bytes", c_int64), ("n_groups", c_int64), ("step", c_void_p), ("lr", c_void_p), ("base", c_void_p),
        ("lr_min", c_void_p), ("warmup_start", c_void_p), ("warmup_steps", c_void_p), ("total_steps", c_void_p),
        ("warmup_prefix", c_void_p),
    ]


# name -> (restype, argtypes); must list every symbol of include/anemoi_amd.h (checked by tests/test_abi.py)
SIGNATURES = {
    "anemoi_abi_version": (c_int, []),
    "anemoi_build_info": (ctypes.c_char_p, []),
    "anemoi_last_error": (c_char_p, []),
    "anemoi_layer_norm": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int,
                                  c_float, c_void_p]),
    "anemoi_layer_norm_residual": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                           c_int64, c_int, c_float, c_void_p]),
    "anemoi_layer_norm_stats": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                        c_int, c_float, c_void_p]),
    "anemoi_linear": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                              c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_linear_stats": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                    c_void_p, c_int64, c_int64, c_int, c_int, c_void_p, c_int64, c_float, c_void_p,
                                    c_void_p]),
    "anemoi_row_stats": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "anemoi_linear_ln": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_edge_attr_csr": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_int, c_int,
                                     c_int64, c_void_p]),
    "anemoi_gt_edge_attention_folded": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                                c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_void_p]),
    "anemoi_gt_edge_attention_raw": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                             c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                             c_int, c_int, c_int, c_int, c_void_p]),
    "anemoi_gt_edge_attention_folded_runs": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                     c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                                     c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int,
                                                     c_int, c_void_p]),
    "anemoi_gt_edge_attention_folded_groups": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                       c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64,
                                                       c_void_p, c_int64, c_int, c_int, c_void_p]),
    "anemoi_edge_schedule_shape": (c_int, [c_int, c_int64, c_int, c_void_p, c_void_p]),
    "anemoi_gt_edge_attention_folded_sched": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                      c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                                      c_void_p, c_int, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                                      c_int64, c_int, c_int, c_void_p]),
    "anemoi_gt_edge_attention_folded_tiles": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                                      c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                                      c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                                      c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int,
                                                      c_void_p]),
    "anemoi_linear_dual": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                   c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_linear_route": (c_int, [ctypes.POINTER(LinearArgs), ctypes.POINTER(LinearRoute)]),
    "anemoi_linear_thin": (c_int, [ctypes.POINTER(LinearThinArgs), c_void_p]),
    "anemoi_linear_actgrad": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                      c_int, c_int, c_int, c_void_p]),
    "anemoi_gt_conv": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                               c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_float, c_uint32,
                               c_void_p, c_void_p]),
    "anemoi_gt_conv_backward_dst": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                            c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int64, c_int64, c_int, c_int, c_float, c_uint32, c_void_p,
                                            c_void_p]),
    "anemoi_gt_conv_backward_src": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                            c_int64, c_int, c_int, c_float, c_uint32, c_void_p, c_void_p]),
    "anemoi_gt_edge_attention": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                         c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int64, c_int64, c_int, c_int, c_void_p]),
    "anemoi_gather_add_act": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_int64, c_int64, c_int, c_int, c_void_p]),
    "anemoi_segment_sum": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_segment_sum_cat": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                       c_int, c_void_p]),
    "anemoi_mhsa_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "anemoi_mhsa": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                            c_int, c_float, c_uint32, c_void_p, c_int, c_int, c_void_p]),
    "anemoi_mhsa_backward_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "anemoi_mhsa_backward": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                     c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_uint32,
                                     c_void_p, c_int, c_int, c_void_p]),
    "anemoi_mhsa_route": (c_int, [ctypes.POINTER(MhsaArgs), ctypes.POINTER(MhsaRoute)]),
    "anemoi_assemble_nodes": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int,
                                      c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "anemoi_finalize_output": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "anemoi_assemble_node_rows": (c_int, [c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_int, c_void_p, c_int,
                                          c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "anemoi_finalize_output_rows": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_int64,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "anemoi_bound_output": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p]),
    "anemoi_assemble_nodes_imputed": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int,
                                              c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_int, c_void_p]),
    "anemoi_finalize_output_imputed": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                               c_void_p, c_void_p]),
    "anemoi_bound_output_imputed": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                            c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "anemoi_bound_output_leaky": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                          c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p,
                                          c_void_p]),
    "anemoi_bound_output_train": (c_int, [c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int, c_void_p]),
    "anemoi_bound_output_backward": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "anemoi_assemble_nodes_remapped": (c_int, [c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int, c_void_p, c_int,
                                               c_void_p, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "anemoi_residual_remapped": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p]),
    "anemoi_unmap_output": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "anemoi_prognostic_residual": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p,
                                           c_void_p, c_int, c_void_p]),
    "anemoi_advance_input": (c_int, [c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_void_p, c_int,
                                     c_void_p, c_void_p]),
    "anemoi_advance_state": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_void_p, c_int, c_void_p,
                                     c_int, c_void_p, c_void_p]),
    "anemoi_advance_state_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int,
                                              c_void_p, c_void_p, c_int, c_void_p]),
    "anemoi_assemble_nodes_backward": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int, c_int, c_int, c_int64, c_int,
                                               c_void_p]),
    "anemoi_prognostic_residual_backward": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int64, c_int,
                                                    c_void_p, c_void_p]),
    "anemoi_csr_project": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int, c_int,
                                   c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                   c_void_p, c_int, c_void_p]),
    "anemoi_weighted_mse_workspace_floats": (c_int64, [c_int64, c_int]),
    "anemoi_weighted_mse": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_float,
                                    c_void_p, c_void_p, c_int64, c_void_p]),
    "anemoi_weighted_mse_backward": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_float, c_void_p, c_void_p, c_void_p]),
    "anemoi_weighted_error_workspace_floats": (c_int64, [c_int64, c_int64, c_int]),
    "anemoi_weighted_error": (c_int, [c_int, c_float, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "anemoi_weighted_error_backward": (c_int, [c_int, c_float, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p,
                                               c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "anemoi_ensemble_score_workspace_floats": (c_int64, [c_int64, c_int64, c_int, c_int]),
    "anemoi_ensemble_score": (c_int, [c_int, c_float, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_int64, c_void_p,
                                      c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_int64, c_void_p]),
    "anemoi_ensemble_score_backward": (c_int, [c_int, c_float, c_void_p, c_void_p, c_int64, c_int, c_int64, c_int, c_int64,
                                               c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "anemoi_cond_layer_norm": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "anemoi_cond_layer_norm_backward_workspace_floats": (c_int64, [c_int64, c_int, c_int]),
    "anemoi_cond_layer_norm_backward": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int,
                                                c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p]),
    "anemoi_head_norm": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int,
                                 c_float, c_void_p]),
    "anemoi_head_norm_backward_workspace_floats": (c_int64, [c_int64, c_int, c_int, c_int]),
    "anemoi_head_norm_backward": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                          c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p]),
    "anemoi_gaussian_noise": (c_int, [c_void_p, c_int64, c_int, c_float, c_uint32, c_void_p, c_void_p]),
    "anemoi_transpose": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_transpose_colsum_rows": (c_int64, [c_int64, c_int64]),
    "anemoi_transpose_chunked": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int64, c_void_p,
                                         c_void_p]),
    "anemoi_weight_grad_tn": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                      c_int, c_int, c_int, c_void_p]),
    "anemoi_linear_batched": (c_int, [c_int, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                      c_int64, c_int, c_int64, c_int, c_int, c_void_p]),
    "anemoi_col_sum_workspace_floats": (c_int64, [c_int64, c_int]),
    "anemoi_col_sum": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "anemoi_row_dot": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "anemoi_row_scale": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_float, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_raw_row_tail": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_act_forward": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int,
                                   c_void_p]),
    "anemoi_act_backward": (c_int, [c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int,
                                    c_void_p]),
    "anemoi_layer_norm_backward_workspace_floats": (c_int64, [c_int64, c_int]),
    "anemoi_layer_norm_backward": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                           c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                           c_int64, c_void_p]),
    "anemoi_gt_edge_attention_folded_backward_dst": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64,
                                                             c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                                             c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p,
                                                             c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                                             c_void_p, c_int64, c_int64, c_int, c_int, c_void_p]),
    "anemoi_gt_edge_attention_folded_backward_src": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                             c_void_p, c_int64, c_int64, c_int, c_int, c_void_p]),
    "anemoi_gt_edge_attr_grad": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                         c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_convert_pad": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_add": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "anemoi_gt_block_tail": (c_int, [ctypes.POINTER(GtBlockArgs), c_void_p]),
    "anemoi_gt_processor_block_forward": (c_int, [ctypes.POINTER(GtBlockArgs), c_void_p]),
    "anemoi_transformer_block_forward": (c_int, [ctypes.POINTER(TfmBlockArgs), c_void_p]),
    "anemoi_mx_quantize": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_float, c_void_p, c_int64, c_void_p,
                                   c_int64, c_int64, c_int, c_int, c_void_p]),
    "anemoi_linear_mx": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                 c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_split_weight": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "anemoi_linear_split": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                    c_int64, c_int, c_int, c_int, c_void_p]),
    "anemoi_weight_grad_split": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int, c_int,
                                         c_int, c_void_p]),
    "anemoi_multi_tensor_max_tensors": (c_int, []),
    "anemoi_multi_tensor_chunk": (c_int, []),
    "anemoi_multi_sumsq_workspace_floats": (c_int64, [c_void_p, c_int64]),
    "anemoi_multi_sumsq": (c_int, [ctypes.POINTER(MultiTensorArgs), c_void_p]),
    "anemoi_adamw_constants": (c_int, [ctypes.POINTER(AdamwConstantsArgs), c_void_p]),
    "anemoi_multi_adamw": (c_int, [ctypes.POINTER(MultiTensorArgs), c_void_p]),
    "anemoi_multi_scale": (c_int, [ctypes.POINTER(MultiTensorArgs), c_void_p]),
    "anemoi_average_constants": (c_int, [ctypes.POINTER(AverageConstantsArgs), c_void_p]),
    "anemoi_multi_average": (c_int, [ctypes.POINTER(MultiAverageArgs), c_void_p]),
    "anemoi_multi_swap": (c_int, [ctypes.POINTER(MultiSwapArgs), c_void_p]),
    "anemoi_lr_schedule": (c_int, [ctypes.POINTER(LrScheduleArgs), c_void_p]),
    "anemoi_trail_begin": (c_int, [c_void_p, c_int64]),
    "anemoi_trail_end": (c_int, [ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "anemoi_trail_entry": (c_int, [c_int64, ctypes.POINTER(c_char_p), ctypes.POINTER(c_int), ctypes.POINTER(c_int64),
                                   ctypes.POINTER(c_int64)]),
    "anemoi_trail_note": (c_int, [c_char_p, c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
}

_lib = None


class KernelLibraryMissing(RuntimeError):
    pass


def load(build_if_missing: bool = False) -> ctypes.CDLL:
    """Load the kernel library (once).  Raises :class:`KernelLibraryMissing` if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        if build_if_missing:
            from ._build import build

            build()
        else:
            raise KernelLibraryMissing(
                f"{LIB_PATH} not found: the HIP kernel library has not been built "
                "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
            )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = ABI mismatch between header and library
        fn.restype = restype
        fn.argtypes = argtypes
    got = lib.anemoi_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"libanemoi_amd.so ABI version {got} != expected {ABI_VERSION}; rebuild the library")
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    """Map a C status code to the exception type the reference raises in the same situation."""
    if status == ANEMOI_OK:
        return
    msg = load().anemoi_last_error()
    msg = msg.decode() if msg else what
    if status == ANEMOI_ERR_INVALID:
        raise ValueError(msg)
    if status == ANEMOI_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)
