"""The embedding table's gradient as a row list, and the clip + Adam step over it: the calls of
csrc/optim_rows_abi.hpp's entry points and `RowGrad`, the object that carries the touched rows from MAG's deterministic
backward to `ClipAdam`.

A MAG batch touches a small part of the [V, H] table, and the deterministic backward (mag_det.py, §7o) knows which: it
holds the sorted key list, and its gather writes every touched row of dW exactly once.  Handed a `RowGrad`, that backward
writes dW into the RowGrad's persistent buffer -- never zeroed, never read outside the touched rows -- hands over the key
list, and gives the weight no `.grad`.  `ClipAdam.set_row_grad(param, row_grad, mode)` then steps the table from it:

  * mode "exact": every element of the table gets the update the dense path gives it, bit for bit (an untouched row takes
    g = 0.0f through the same expression).  What is saved is the zero-fill of dW and its two dense reads.
  * mode "lazy": only the touched rows of the parameter, `exp_avg` and `exp_avg_sq` are read and written; every other
    row keeps its bits.  THIS IS NOT THE REFERENCE'S TRAJECTORY: model_mag.py:312 uses dense torch.optim.Adam, under
    which an untouched row still moves while its moments decay.  weight_decay must be 0 in this mode.

The entry points are extern "C" symbols of libgrandplus.so declared in csrc/optim_rows_abi.hpp; they are not part of
C ABI 4, so `_native.PRIVATE_ABI` binds them, not `_native.ABI`, as it binds mag_det's.

`BitmapRowGrad` is a RowGrad for the ATOMIC backward, which keeps no key list: the rows a batch can touch are
marked in a bitmap of V bits (csrc/row_mark_abi.hpp, bound by `_native.PRIVATE_ABI` too), the bitmap is compacted into the
same kind of list -- ascending, each row once, sentinel V in the tail -- and the listed rows of `values` are zeroed for the
atomics to add into.  `ClipAdam.set_row_grad` and both row kernels take it unchanged.

`RowGrad.track_dirty()` has every `fill` also mark the rows it is handed in a bitmap `dirty` that only
accumulates here: `fit.BestTracker(row_grad=)` reads it to snapshot the table row by row, and clears it.

Left out: amsgrad, lazy mode with weight decay, Adam's moments in the best-weights snapshot (the reference
saves the state_dict alone).
"""
from __future__ import annotations

import torch

from . import _native
from ._common import _ptr, _stream

__all__ = ["RowGrad", "BitmapRowGrad", "MODES", "check_mode"]

ROW_LIST_PARTIALS = 1024                  # GP_ROW_LIST_PARTIALS
MODES = {"exact": 1, "lazy": 2}           # GP_OPTIM_ROWS_EXACT, GP_OPTIM_ROWS_LAZY


def lib():
    """`_native.lib()`, looked up at each call: this module binds nothing, and a patch of `_native.lib` reaches it."""
    return _native.lib()


def check_mode(mode):
    """`mode` as "exact" or "lazy" (ValueError otherwise)."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"the table step's mode must be 'exact' or 'lazy', got {mode!r}")
    return mode


class RowGrad:
    """The gradient of one [V, H] embedding table as (values, keys): `values` is a persistent float32 [V, H] buffer on the
    parameter's device that is never zeroed; after a deterministic backward of `mag_prop_rows(..., row_grad=this)`, `keys`
    is that backward's sorted key list (int64 [n_sorted], ascending, sentinel V in the tail) and the rows of `values`
    that occur in it hold the batch's dW.  Every other row of `values` holds anything at all and is never read.

    `keys` and `n_sorted` are set when Python runs the backward: in an eager step, and once when a graph is captured.  A
    captured graph carries its own key tensor and its own length in its launches, so replays are right whatever these
    attributes say; but with several graphs over one RowGrad (`MagTrainStep.step_sampled`, a graph per batch shape, each
    with its own `max_entries`) they describe the graph captured LAST, not the one replayed last.  Read them after a
    replay only when the step has one graph; `values` is the one buffer of every graph.

    param: the table, a contiguous float32 CUDA [V, H] tensor (TypeError / ValueError otherwise; no CPU fallback)."""

    def __init__(self, param):
        if not isinstance(param, torch.Tensor) or param.is_sparse or param.dtype != torch.float32 or not param.is_contiguous():
            raise TypeError("RowGrad takes a dense contiguous float32 table")
        if param.dim() != 2 or param.shape[0] < 1 or param.shape[1] < 1:
            raise ValueError(f"RowGrad takes a 2-D [V, H] table, got shape {tuple(param.shape)}")
        if not param.is_cuda:
            raise TypeError("RowGrad takes a CUDA table: the row-list step runs on the GPU only (no CPU fallback)")
        self.param = param
        self.shape = tuple(param.shape)
        self.device = param.device
        self.values = torch.empty(self.shape, dtype=torch.float32, device=param.device)
        self.keys = None
        self.n_sorted = 0
        self.dirty = None

    def track_dirty(self):
        """Makes `dirty` (int32 [(V + 31) // 32], zeros, made once): from here on every `fill` sets the bits of the rows it is
        handed (one gp_fit_rows_mark), and `fit.BestTracker(row_grad=this)`, the one reader, copies those rows
        and clears the bits.  To be called before a step over this RowGrad is captured: the mark is a launch of the
        backward, so a graph captured earlier lacks it.  Returns `dirty`."""
        if self.dirty is None:
            self.dirty = torch.zeros((self.shape[0] + 31) // 32, dtype=torch.int32, device=self.device)
        return self.dirty

    def check_weight(self, weight):
        """Refuses a weight that is not this RowGrad's table (before any device call)."""
        if weight is not self.param:
            raise ValueError("row_grad was made for another tensor: RowGrad(param) takes the weight itself")
        if tuple(weight.shape) != self.shape or weight.device != self.device:
            raise ValueError(f"row_grad holds a {self.shape} table on {self.device}, the weight is {tuple(weight.shape)} on "
                             f"{weight.device}")

    def fill(self, sorted_keys):
        """What the backward calls once `values` holds the batch's rows: takes the key list over.  With `dirty` set it marks
        the list's rows there, on the current stream: inside the backward, so inside every captured graph of the step, with
        that graph's own key tensor and length."""
        self.keys = sorted_keys
        self.n_sorted = sorted_keys.numel()
        if self.dirty is not None:
            from .fit import rows_mark
            rows_mark(sorted_keys, self.shape[0], self.dirty)

    def filled(self):
        return self.keys is not None


class BitmapRowGrad(RowGrad):
    """A RowGrad that the ATOMIC backward of `mag_prop_rows(..., row_grad=this, deterministic=False, max_entries=M)` fills
    (DESIGN §7u).  Besides `values` it holds `bitmap` (int32 [(V + 31) // 32], zeros, made once: one bit per row, all zero
    between two backwards), `count` (int64 [1]: how many rows the last backward marked, unclamped) and `partials`, the
    workspace of the compaction.  After a backward `keys` is int64 [min(V, M)]: the distinct rows of the batch's bags,
    ascending, the sentinel V in the tail; the listed rows of `values` hold the batch's dW, every other row anything at all.
    `values` is never zero-filled as a whole.

    `reset()` zeroes the bitmap: for a caller whose backward raised between the mark and the compaction."""

    def __init__(self, param):
        super().__init__(param)
        V = self.shape[0]
        self.bitmap = torch.zeros((V + 31) // 32, dtype=torch.int32, device=self.device)
        self.count = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.partials = torch.empty(ROW_LIST_PARTIALS, dtype=torch.int64, device=self.device)

    def reset(self):
        self.bitmap.zero_()


def mark_and_list(rg, call, capacity, overflow):
    """The row list of one batch for a BitmapRowGrad, on the current stream: gp_row_mark_mag over the batch of `call` (a
    mag._Call), gp_row_list_compact into a fresh int64 [capacity] and gp_row_list_zero of the listed rows of `rg.values`.
    Four launches, no host read.  Returns the keys; bit 0 of `overflow` is set when more than `capacity` rows were marked."""
    attr_indptr, attr_indices, _, col, _, filled, batch_rows, _ = call.tensors
    S_rows, K, B = call.scalars[:3]
    V, H = rg.shape
    dev, stream, L = rg.device.index, _stream(rg.values), _native.lib()
    keys = torch.empty(capacity, dtype=torch.int64, device=rg.device)
    rc = L.gp_row_mark_mag(dev, V, attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_indptr.numel() - 1, col.data_ptr(),
                           _ptr(filled), S_rows, K, _ptr(batch_rows), B, rg.bitmap.data_ptr(), stream)
    _native.raise_for_status(rc)
    rc = L.gp_row_list_compact(dev, V, rg.bitmap.data_ptr(), capacity, keys.data_ptr(), rg.count.data_ptr(),
                               rg.partials.data_ptr(), overflow.data_ptr(), stream)
    _native.raise_for_status(rc)
    rc = L.gp_row_list_zero(dev, keys.data_ptr(), capacity, V, H, rg.values.data_ptr(), stream)
    _native.raise_for_status(rc)
    return keys


def sqnorm(rg, accumulate, ws):
    """gp_optim_rows_sqnorm of a filled RowGrad into the workspace `ws`, on the current stream."""
    V, H = rg.shape
    rc = _native.lib().gp_optim_rows_sqnorm(rg.device.index, rg.keys.data_ptr(), rg.n_sorted, V, H, rg.values.data_ptr(),
                                            int(bool(accumulate)), ws.data_ptr(), _stream(rg.values))
    _native.raise_for_status(rc)


def clip_adam_rows(rg, mode, exp_avg, exp_avg_sq, ws, norm, *, max_norm, lr, betas, eps, weight_decay, step_size=None,
                   rsqrt_bc2=None, d_step_size=None, d_rsqrt_bc2=None):
    """gp_clip_adam_rows (step_size, rsqrt_bc2 as numbers) or gp_clip_adam_rows_dev (their device addresses) of a filled
    RowGrad: the workspace holds the norm's partials."""
    V, H = rg.shape
    head = (rg.device.index, rg.param.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), rg.values.data_ptr(),
            rg.keys.data_ptr(), rg.n_sorted, V, H, MODES[mode], max_norm, lr, betas[0], betas[1], eps, weight_decay)
    tail = (ws.data_ptr(), norm.data_ptr(), _stream(rg.values))
    if d_step_size is None:
        rc = _native.lib().gp_clip_adam_rows(*head, step_size, rsqrt_bc2, *tail)
    else:
        rc = _native.lib().gp_clip_adam_rows_dev(*head, d_step_size, d_rsqrt_bc2, *tail)
    _native.raise_for_status(rc)
