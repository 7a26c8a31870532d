"""ctypes binding of include/grandplus.h (libgrandplus.so, hand-written HIP for gfx950).

There is no CPU fallback: if the shared library is missing this module raises at first
use, and if no GPU is visible `gp_graph_create` returns GP_ERR_NO_DEVICE (RuntimeError).
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# GRANDPLUS_DIAG=1 selects the diagnostic build (in-kernel phase stamps); never the default.
# GRANDPLUS_LIB=<file name in this directory> selects another HIP build of the same sources (A/B runs of
# two kernel variants on the same GPU box, see tools/ab_libs.sh); there is no non-HIP implementation to select.
LIB_PATH = os.path.join(_HERE, os.environ.get("GRANDPLUS_LIB") or
                        ("libgrandplus_diag.so" if os.environ.get("GRANDPLUS_DIAG") == "1" else "libgrandplus.so"))

GP_OK = 0
GP_ERR_NULL, GP_ERR_INVALID_CSR, GP_ERR_INVALID_SEED, GP_ERR_INVALID_ARG = 1, 2, 3, 4
GP_ERR_NO_DEVICE, GP_ERR_HIP, GP_ERR_NOMEM, GP_ERR_OVERFLOW = 5, 6, 7, 8
GP_MAX_K = 1024

GP_LOSS_KL, GP_LOSS_L2 = 0, 1
GP_MAX_SAMPLES = 16


GP_MLP_RELU, GP_MLP_NORM, GP_MLP_BN, GP_MLP_TRAINING = 1, 2, 4, 8


GP_OPTIM_MAX_TENSORS = 32
GP_OPTIM_CLIP_ONLY, GP_OPTIM_NORM_ONLY, GP_OPTIM_NORM_READY = 1, 2, 4


def optim_workspace_bytes() -> int:
    """GP_OPTIM_WORKSPACE_BYTES of grandplus.h."""
    return 8192


GP_EVAL_WRONG, GP_EVAL_CORRECT, GP_EVAL_IGNORED, GP_EVAL_BAD = 0, 1, 2, 3
GP_MAX_CLASSES = 4096


def eval_workspace_bytes() -> int:
    """GP_EVAL_WORKSPACE_BYTES of grandplus_eval.h."""
    return 1024 * 40


# GP_EVAL_TAIL_MAX_ROWS and GP_EVAL_TAIL_WORKSPACE_BYTES of csrc/eval_tail_abi.hpp, a private header: the names with a GP_ prefix
# and the *_bytes functions of this module are the public headers' (the workspace is the ticket counter, padded)
EVAL_TAIL_MAX_ROWS = 65536
EVAL_TAIL_WORKSPACE_BYTES = 64


def scatter_rows_workspace_bytes(n_samples: int, n_batch: int) -> int:
    """GP_SCATTER_ROWS_WORKSPACE_BYTES of grandplus_scatter.h."""
    return 4 * n_samples * n_batch


def scatter_bag_workspace_bytes(n_rows: int) -> int:
    """GP_SCATTER_BAG_WORKSPACE_BYTES of grandplus_scatter.h."""
    return 4 * n_rows


GP_STEP_MAX_GROUPS, GP_STEP_MAX_LAYERS = 8, 8
GP_STEP_SEG_ROWS, GP_STEP_SEG_LAYER = 0, 1


class GpStepState(ctypes.Structure):
    """gp_step_state of grandplus_step.h: the image of the device struct (StepState.read copies it to the host)."""
    _fields_ = [("tick", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("weight", ctypes.c_float),
                ("step_size", ctypes.c_float * GP_STEP_MAX_GROUPS), ("rsqrt_bc2", ctypes.c_float * GP_STEP_MAX_GROUPS)]


class GpStepSegment(ctypes.Structure):
    """gp_step_segment of grandplus_step.h: device pointers as integers."""
    _fields_ = [("keep", ctypes.c_void_p), ("keep_stride", ctypes.c_int64), ("batch_rows", ctypes.c_void_p),
                ("filled", ctypes.c_void_p), ("kind", ctypes.c_int32), ("n_samples", ctypes.c_int32),
                ("n_batch", ctypes.c_int32), ("K", ctypes.c_int32), ("width", ctypes.c_int32), ("layer", ctypes.c_int32),
                ("p", ctypes.c_float), ("pad", ctypes.c_int32)]


GP_FIT_STOP_ACC, GP_FIT_STOP_BOTH = 0, 1
GP_FIT_MAX_COPIES = 32


class GpFitTrack(ctypes.Structure):
    """gp_fit_track of grandplus_fit.h: the image of the device struct (BestTracker.read copies it to the host)."""
    _fields_ = [("best_loss", ctypes.c_float), ("best_acc", ctypes.c_float), ("best_tick", ctypes.c_uint64),
                ("stop_tick", ctypes.c_uint64), ("bad_counter", ctypes.c_int32), ("n_evals", ctypes.c_int32),
                ("copy_now", ctypes.c_int32), ("stopped", ctypes.c_int32)]


class GpFitCopy(ctypes.Structure):
    """gp_fit_copy of grandplus_fit.h: device pointers as integers, 4-byte words."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n_words", ctypes.c_int64)]


class GpOptimTensor(ctypes.Structure):
    """gp_optim_tensor of grandplus.h: device pointers as integers."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_int64)]


def mlp_saved_floats(S: int, B: int, f_in: int) -> int:
    """GP_MLP_SAVED_FLOATS of grandplus.h."""
    return S * B + 4 * S * f_in


def mlp_forward_workspace_bytes(S: int) -> int:
    """GP_MLP_FORWARD_WORKSPACE_BYTES of grandplus.h."""
    return S * 2097152


def mlp_backward_workspace_bytes(S: int, B: int, f_in: int) -> int:
    """GP_MLP_BACKWARD_WORKSPACE_BYTES of grandplus.h."""
    return 4 * (S * B * f_in + 524288)


def grand_loss_workspace_bytes(n_rows: int) -> int:
    """GP_GRAND_LOSS_WORKSPACE_BYTES of grandplus.h."""
    return 20 * n_rows


def mlp_infer_workspace_bytes(n_rows: int, f_in: int) -> int:
    """GP_MLP_INFER_WORKSPACE_BYTES of grandplus_infer.h."""
    return (4 * (n_rows + 2 * f_in) + 15) // 16 * 16


GP_MLP_CHAIN_MAX_HIDDEN, GP_MLP_CHAIN_MAX_OUT = 1024, 64


def mlp_infer_chain_workspace_bytes(n_rows: int, f_in: int, f_hidden: int) -> int:
    """GP_MLP_INFER_CHAIN_WORKSPACE_BYTES of grandplus_infer_chain.h."""
    return (4 * (n_rows + 2 * f_in + 2 * f_hidden) + 15) // 16 * 16


class GpStats(ctypes.Structure):
    _fields_ = [
        ("rows", ctypes.c_int64), ("pushes", ctypes.c_int64), ("edges", ctypes.c_int64),
        ("filled", ctypes.c_int64), ("support", ctypes.c_int64), ("frontier", ctypes.c_int64),
        ("lds_levels", ctypes.c_int64), ("global_levels", ctypes.c_int64),
        ("failed_rows", ctypes.c_int64), ("degree_lookups", ctypes.c_int64), ("kernel_ms", ctypes.c_double),
        ("workgroups", ctypes.c_int32), ("block_threads", ctypes.c_int32),
        ("lds_bytes", ctypes.c_int32), ("lds_slots", ctypes.c_int32),
        ("workspace_bytes", ctypes.c_int64),
        ("diag_ticks_scan", ctypes.c_int64), ("diag_ticks_expand", ctypes.c_int64),
        ("diag_ticks_topk", ctypes.c_int64), ("diag_ticks_total", ctypes.c_int64),
        ("diag_ticks_scan_hbm", ctypes.c_int64), ("diag_ticks_expand_hbm", ctypes.c_int64),
        ("diag_sub", ctypes.c_int64 * 16),
        ("retried_rows", ctypes.c_int64), ("max_level_edges", ctypes.c_int64), ("max_log_records", ctypes.c_int64),
        ("kernel", ctypes.c_int32), ("sketch_pad", ctypes.c_int32),
        ("sketch_candidate_edges", ctypes.c_int64), ("sketch_second_sweeps", ctypes.c_int64),
        ("choice_ms", ctypes.c_float * 3), ("choice_pad", ctypes.c_int32),
    ]

    def as_dict(self):
        d = {name: getattr(self, name) for name, _ in self._fields_}
        d["diag_sub"] = list(self.diag_sub)
        d["choice_ms"] = list(self.choice_ms)
        return d


# The C ABI, declared once: public header (in the order include/grandplus.h includes them) -> entry point -> (restype,
# argtypes, required).  tests/test_host_abi.py holds every entry against its header's prototype, type by type.  The convention:
#   * a pointer parameter named d_* travels as c_void_p (an integer, from tensor.data_ptr()); so do void* (untyped device
#     memory, a stream), gp_graph* and gp_step_state*;
#   * T** is POINTER(c_void_p);
#   * const char* is c_char_p;
#   * every other T* is a host array and travels as POINTER(T), with gp_stats, gp_optim_tensor, gp_step_segment and gp_fit_copy
#     mapping to their Structure classes;
#   * scalars map one to one.
# A name that is not required may be missing from an older build selected with GRANDPLUS_LIB (an A/B run): calling it there
# raises a clear error.  A missing required name fails at load.  (gp_internal_graph_csr, gp_internal_multi_plan and
# gp_internal_set_error were never needed at load, so they are not required either; nothing outside grandplus.h is.)
_int, _i32, _i64, _u32, _u64, _f32, _f64 = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64,
                                            ctypes.c_float, ctypes.c_double)
_vp, _str = ctypes.c_void_p, ctypes.c_char_p
_intp, _i32p, _i64p, _u32p, _f64p, _vpp = (ctypes.POINTER(t) for t in (_int, _i32, _i64, _u32, _f64, _vp))
_bag = [_int, _vp, _i64, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _int, _vp, _f32, _int, _u64, _vp, _vp, _vp, _vp]
_loss = [_int, _vp, _i32, _i64, _i32, _vp, _i64, _i64, _f32, _f32, _f32, _int, _int]
# gp_mag_prop_rows' arguments between the table and the outputs; a block of the eval MLP: weight, bias, flags, the four
# BatchNorm tensors and eps
_mag = [_i64, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _f32, _f32, _int, _u64, _vp, _i64]
_block = [_vp, _vp, _int, _vp, _vp, _vp, _vp, _f32]
ABI = {
    "grandplus.h": {
        "gp_abi_version": (_int, [], True),
        "gp_strerror": (_str, [_int], True),
        "gp_last_error": (_str, [], True),
        "gp_device_count": (_int, [], True),
        "gp_graph_create": (_int, [_i32p, _i64, _i32p, _i64, _int, _vpp], True),
        "gp_graph_create_multi": (_int, [_i32p, _i64, _i32p, _i64, _int, _vpp], True),
        "gp_graph_create_multi_on": (_int, [_i32p, _i64, _i32p, _i64, _intp, _int, _vpp], False),
        "gp_graph_num_gpus": (_int, [_vp], True),
        "gp_graph_destroy": (None, [_vp], True),
        "gp_graph_num_nodes": (_i64, [_vp], True),
        "gp_graph_nnz": (_i64, [_vp], True),
        "gp_graph_device": (_int, [_vp], True),
        "gp_gfpush": (_int, [_vp, _i32p, _i64, _f64p, _int, _f64, _int, _i32p, _i32p, _f64p], True),
        "gp_gfpush_device": (_int, [_vp, _vp, _i64, _f64p, _int, _f64, _int, _vp, _vp, _vp, _vp, _vp], True),
        "gp_get_stats": (_int, [_vp, ctypes.POINTER(GpStats)], True),
        "gp_reset_stats": (_int, [_vp], True),
        "gp_set_option": (_int, [_vp, _str, _i64], True),
        "gp_random_prop_rows": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _f32, _int, _u64, _vp, _vp, _vp], True),
        "gp_seed_positions": (_int, [_int, _vp, _i64, _i64, _vp, _vp, _vp], False),
        "gp_batch_positions": (_int, [_int, _vp, _i64, _vp, _i64, _vp, _vp, _vp], False),
        "gp_random_prop_coo": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _f32, _int, _u64, _vp, _vp, _vp], True),
        "gp_random_prop_coo_backward": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _f32, _int, _u64, _vp, _vp, _vp], False),
        "gp_random_prop_rows_backward": (_int, [_int, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _f32, _int, _u64, _vp, _vp, _i64, _vp],
                                         False),
        "gp_embedding_bag": (_int, _bag, False),
        "gp_embedding_bag_backward": (_int, _bag, False),
        "gp_random_prop_rows_multi": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _f32, _int, _u64, _vp, _i64,
                                             _vp, _vp], False),
        "gp_random_prop_coo_multi": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _f32, _int, _u64, _vp, _vp, _vp], False),
        "gp_random_prop_coo_multi_backward": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _f32, _int, _u64, _vp, _vp, _vp], False),
        "gp_random_prop_rows_multi_backward": (_int, [_int, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _f32, _int, _u64, _vp, _i64,
                                                      _vp, _i64, _vp], False),
        "gp_grand_loss": (_int, _loss + [_vp, _vp, _vp, _vp], False),
        "gp_grand_loss_backward": (_int, _loss + [_vp, _vp, _vp, _vp, _vp, _vp], False),
        "gp_mlp_block_forward": (_int, [_int, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _int, _vp, _vp, _vp, _vp, _vp, _f32, _f32,
                                        _f32, _u64, _i32, _vp, _vp, _vp, _vp, _vp, _vp], False),
        "gp_mlp_block_backward": (_int, [_int, _vp, _i32, _i64, _i32, _i32, _vp, _int, _vp, _f32, _u64, _i32, _vp,
                                         _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp], False),
        "gp_clip_adam_step": (_int, [_int, ctypes.POINTER(GpOptimTensor), _i32, _int, _f32, _f32, _f64, _f64, _f32, _f32, _f32, _f32,
                                     _vp, _vp, _vp], False),
        "gp_propagate_features": (_int, [_vp, _vp, _i32, _vp, _int, _int, _f64, _vp, _vp], True),
        "gp_internal_graph_csr": (_int, [_vp, _vpp, _vpp, _u32p, _vp], False),
        # h_acsr, h_node_pos and h_unit_info are host arrays declared c_void_p, the three exceptions to the convention: the one
        # caller (api.Graph) passes .ctypes.data_as(c_void_p), and a typed pointer would change that call site
        "gp_internal_graph_acsr": (_int, [_vp, _vp, _vp, _vp, _i64p, _intp, _u32p], False),
        "gp_internal_diag_counters": (_int, [_vp, _i64p, _int], True),
        "gp_internal_multi_plan": (_int, [_i64, _int, _int, _i64, _int, _int, _i64p, _int], False),
        "gp_internal_set_error": (None, [_int, _str, _str], False),
        "gp_internal_create_ms": (None, [_f64p], False),
        "gp_internal_warm_device": (_int, [_int], False),
    },
    "grandplus_eval.h": {
        "gp_eval_head": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp], False),
        "gp_eval_reduce": (_int, [_int, _vp, _vp, _i64, _vp, _vp, _vp, _vp], False),
    },
    # each takes the arguments of its atomic counterpart, then the sorted order (entry numbers, sorted keys[, sorted rows],
    # their length) and the scratch
    "grandplus_scatter.h": {
        "gp_random_prop_rows_backward_det": (_int, [_int, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _f32, _int, _u64, _vp, _i64,
                                                    _vp, _i64, _vp, _vp, _i64, _vp, _vp], False),
        "gp_embedding_bag_backward_det": (_int, _bag[:-1] + [_vp, _vp, _vp, _i64, _vp, _vp], False),
    },
    "grandplus_infer.h": {
        "gp_mlp_infer_block": (_int, [_int, _vp, _i64, _i32, _i32] + _block + [_vp, _vp, _vp], False),
    },
    "grandplus_infer_chain.h": {
        "gp_mlp_infer_chain2": (_int, [_int, _vp, _i64, _i32, _i32, _i32] + _block + _block + [_vp, _vp, _vp], False),
    },
    # the backward takes the forward's arguments with grad_out for the table and dW for the output, and no counter
    "grandplus_mag.h": {
        "gp_mag_prop_rows": (_int, [_int, _vp] + _mag + [_vp, _vp, _vp], False),
        "gp_mag_prop_rows_backward": (_int, [_int, _vp] + _mag + [_vp, _vp], False),
    },
    "grandplus_order.h": {
        "gp_internal_row_order": (_int, [_vp, _u32p, _i64, _i64p, _intp, _u32p], False),
        "gp_internal_wg_log": (_int, [_vp, _i64p, _int], False),
    },
    # gp_clip_adam_step_dev is gp_clip_adam_step with two device pointers where that takes step_size and rsqrt_bc2
    "grandplus_step.h": {
        "gp_step_advance": (_int, [_int, _vp, _u64, _f64, _f64, _i32, _f64p, _f64p, _f64p, _vp], False),
        "gp_step_masks": (_int, [_int, _vp, ctypes.POINTER(GpStepSegment), _i32, _vp], False),
        "gp_clip_adam_step_dev": (_int, [_int, ctypes.POINTER(GpOptimTensor), _i32, _int, _f32, _f32, _f64, _f64, _f32, _f32, _vp, _vp,
                                         _vp, _vp, _vp], False),
    },
    "grandplus_fit.h": {
        "gp_fit_select": (_int, [_int, _vp, _u64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp], False),
        "gp_fit_track_update": (_int, [_int, _vp, _vp, _vp, _i32, _i32, _vp], False),
        "gp_fit_snapshot": (_int, [_int, _vp, ctypes.POINTER(GpFitCopy), _i32, _vp], False),
    },
}

# The entry points outside C ABI 4: extern "C" symbols of libgrandplus.so whose prototypes stand in the private headers
# csrc/*_abi.hpp, not under include/, so GP_ABI_VERSION and ABI above stay what they are.  Private header -> entry point ->
# (restype, argtypes, False), under the same convention; tests/test_host_abi.py holds both tables against their headers.  No
# private name is required: lib() declares the ones the library has, and calling one it lacks raises (_missing).
_rows_step = [_int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _int, _f32, _f32, _f64, _f64, _f32, _f32]   # device .. weight_decay
# a chunked twin takes its unchunked twin's arguments up to the stream, then chunk, d_scratch, scratch_bytes and the stream
_scatter, _chunk = ABI["grandplus_scatter.h"], [_i32, _vp, _i64, _vp]
_defer = [_vp, _vp, _vp, _i32, _vp]                                   # d_tick, d_last, d_hist, capacity, d_flag
_mag_dseed = _mag[:-3] + [_vp] + _mag[-2:]                            # _mag with d_seed, a device pointer, where seed stands
PRIVATE_ABI = {
    "mag_det_abi.hpp": {
        "gp_mag_det_keys": (_int, [_int, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp], False),
        "gp_mag_prop_rows_backward_det": (_int, [_int, _vp] + _mag + [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp], False),
    },
    "optim_rows_abi.hpp": {
        "gp_optim_rows_sqnorm": (_int, [_int, _vp, _i64, _i64, _i32, _vp, _int, _vp, _vp], False),
        "gp_clip_adam_rows": (_int, _rows_step + [_f32, _f32, _vp, _vp, _vp], False),
        "gp_clip_adam_rows_dev": (_int, _rows_step + [_vp, _vp, _vp, _vp, _vp], False),
    },
    # the deferred exact step: table, moments[, dW], [keys, n_sorted,] V, H, the group's constants, then the
    # tick's address, last, the ring, its capacity and the flag; the step also takes gp_clip_adam_rows_dev's two corrections
    # and its tail
    "optim_defer_abi.hpp": {
        "gp_optim_defer_catch_up": (_int, [_int, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _f64, _f64, _f32, _f32] + _defer + [_vp], False),
        "gp_optim_defer_step": (_int, [_int, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _f32, _f32, _f64, _f64, _f32, _f32, _vp, _vp] +
                                _defer + [_vp, _vp, _vp], False),
        "gp_optim_defer_flush": (_int, [_int, _vp, _vp, _vp, _i64, _i32, _f64, _f64, _f32, _f32] + _defer + [_vp], False),
    },
    "row_mark_abi.hpp": {
        "gp_row_mark_mag": (_int, [_int, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _vp], False),
        "gp_row_list_compact": (_int, [_int, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp], False),
        "gp_row_list_zero": (_int, [_int, _vp, _i64, _i64, _i32, _vp, _vp], False),
    },
    "fit_rows_abi.hpp": {
        "gp_fit_rows_mark": (_int, [_int, _vp, _i64, _i64, _vp, _vp], False),
        "gp_fit_rows_snapshot": (_int, [_int, _vp, _vp, _vp, _i64, _i32, _vp, _vp], False),
    },
    "gather_chunk_abi.hpp": {
        "gp_random_prop_rows_backward_det_chunked": (_int, _scatter["gp_random_prop_rows_backward_det"][1][:-1] + _chunk, False),
        "gp_embedding_bag_backward_det_chunked": (_int, _scatter["gp_embedding_bag_backward_det"][1][:-1] + _chunk, False),
        "gp_mag_prop_rows_backward_det_chunked": (_int, [_int, _vp] + _mag + [_vp, _vp, _vp, _i64, _vp, _vp, _vp] + _chunk, False),
    },
    # the two forms of grandplus_mag.h's pair with a device pointer where those take the seed; the deterministic backward with
    # input dropout takes gp_mag_prop_rows_backward_det's arguments with d_seed after seed and the chunk's three before the stream
    "mag_drop_abi.hpp": {
        "gp_mag_prop_rows_dseed": (_int, [_int, _vp] + _mag_dseed + [_vp, _vp, _vp], False),
        "gp_mag_prop_rows_backward_dseed": (_int, [_int, _vp] + _mag_dseed + [_vp, _vp], False),
        "gp_mag_prop_rows_backward_det_drop": (_int, [_int, _vp] + _mag[:-2] + [_vp] + _mag[-2:] + [_vp, _vp, _vp, _i64, _vp, _vp, _vp] + _chunk,
                                               False),
    },
    # gp_eval_head's arguments without the offset and the capacity, then gp_eval_reduce's from the workspace on
    "eval_tail_abi.hpp": {
        "gp_eval_tail": (_int, [_int, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp], False),
    },
}

_LIB = None


def _missing(name):
    """Stands in for an entry point an older build (GRANDPLUS_LIB=... for an A/B run) lacks: calling it raises a clear error."""
    def missing(*_a, **_k):
        raise RuntimeError(f"{LIB_PATH} does not export {name} (an older build?): rebuild the library")
    return missing


def lib():
    """Load libgrandplus.so (once).  Raises RuntimeError if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64 / libhsa-runtime64.  If this library were loaded first it
    # would pull in /opt/rocm's copies and the process would hold TWO HIP runtimes; whichever initialises
    # second can then report "no ROCm-capable device".  Loading torch first makes the dynamic loader bind
    # libgrandplus.so to the runtime torch already mapped, so device pointers and streams are shared.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    for entries in (*ABI.values(), *PRIVATE_ABI.values()):
        for name, (restype, argtypes, required) in entries.items():
            if not required and not hasattr(L, name):
                setattr(L, name, _missing(name))
                continue
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    # (ABI 3 is accepted only for an older build named explicitly through GRANDPLUS_LIB for an A/B run: its gp_stats is a prefix of
    #  this one, and the entry points it lacks raise a clear error where they are called -- _missing)
    abi = L.gp_abi_version()
    if abi != 4 and not (abi == 3 and os.environ.get("GRANDPLUS_LIB")):
        raise RuntimeError(f"libgrandplus.so ABI version {abi}, this package needs 4: rebuild (python -c 'import __graft_entry__ as g; g.build()')")
    _LIB = L
    return L


def raise_for_status(status: int):
    """Map a C-ABI status to the Python exception the shims document."""
    if status == GP_OK:
        return
    L = lib()
    detail = L.gp_last_error().decode() or L.gp_strerror(status).decode()
    if status in (GP_ERR_INVALID_CSR, GP_ERR_INVALID_SEED, GP_ERR_INVALID_ARG, GP_ERR_NULL):
        raise ValueError(detail)
    if status == GP_ERR_NOMEM:
        raise MemoryError(detail)
    raise RuntimeError(detail)
