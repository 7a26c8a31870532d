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

`DeferredRows` is the state of mode "deferred": the trajectory of "exact", bit for bit, at the memory traffic of
"lazy".  The zero-gradient update of an untouched row is put off and replayed, step by step through the dense step's own
element update, when the row is next read and by a flush (csrc/optim_defer_abi.hpp, bound by `_native.PRIVATE_ABI` too).
Between flushes the table and its moments show lagging rows.

Left out: amsgrad, lazy mode with weight decay, Adam's moments in the best-weights snapshot (the reference
saves the state_dict alone).
"""
from __future__ import annotations

import torch

from . import _native
from ._common import _ptr, _stream

__all__ = ["RowGrad", "BitmapRowGrad", "DeferredRows", "MODES", "check_mode"]

ROW_LIST_PARTIALS = 1024                  # GP_ROW_LIST_PARTIALS
# GP_OPTIM_ROWS_EXACT, GP_OPTIM_ROWS_LAZY; "deferred" has entry points of its own (csrc/optim_defer_abi.hpp) and no C constant
MODES = {"exact": 1, "lazy": 2, "deferred": 3}
DEFER_MIN_CAPACITY, DEFER_MAX_CAPACITY, DEFER_CAPACITY = 4, 65536, 1024   # kMinCapacity, kMaxCapacity; the default ring
DEFER_FLAG_BIT = 2                        # gp_optim_defer::kFlagBit: bit 1 of the flag word, a row that could not be served


def lib():
    """`_native.lib()`, looked up at each call: this module binds nothing, and a patch of `_native.lib` reaches it."""
    return _native.lib()


def check_mode(mode):
    """`mode` as "exact", "lazy" or "deferred" (ValueError otherwise)."""
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"the table step's mode must be 'exact' or 'lazy', or 'deferred', got {mode!r}")
    return mode


def check_capacity(capacity):
    """`capacity` of a DeferredRows ring as an int: a power of two in [4, 65536] (ValueError otherwise; None: 1024)."""
    if capacity is None:
        return DEFER_CAPACITY
    if isinstance(capacity, bool) or not isinstance(capacity, int) or not DEFER_MIN_CAPACITY <= capacity <= DEFER_MAX_CAPACITY or \
            capacity & (capacity - 1):
        raise ValueError(f"the deferred step's capacity must be a power of two in [{DEFER_MIN_CAPACITY}, {DEFER_MAX_CAPACITY}], "
                         f"got {capacity!r}")
    return capacity


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
        self.prelisted = None                                        # the batch's row list, when it was made before the forward (§7za)

    def reset(self):
        self.bitmap.zero_()
        self.prelisted = None


def list_rows(marks, V, attr_indptr, attr_indices, col, filled, S_rows, K, batch_rows, B, capacity, overflow):
    """The rows of the table that a batch's bags name, as a fresh int64 [capacity] list (ascending, each row once, sentinel V
    in the tail), on the current stream: gp_row_mark_mag, then gp_row_list_compact.  marks: what owns `bitmap`, `count` and
    `partials` (a BitmapRowGrad, a DeferredRows).  Bit 0 of `overflow` is set when more than `capacity` rows were marked."""
    dev, stream, L = marks.device.index, _stream(marks.bitmap), _native.lib()
    keys = torch.empty(capacity, dtype=torch.int64, device=marks.device)
    rc = L.gp_row_mark_mag(dev, V, attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_indptr.numel() - 1, col.data_ptr(),
                           _ptr(filled), S_rows, K, _ptr(batch_rows), B, marks.bitmap.data_ptr(), stream)
    _native.raise_for_status(rc)
    rc = L.gp_row_list_compact(dev, V, marks.bitmap.data_ptr(), capacity, keys.data_ptr(), marks.count.data_ptr(),
                               marks.partials.data_ptr(), overflow.data_ptr(), stream)
    _native.raise_for_status(rc)
    return keys


def mark_and_list(rg, call, capacity, overflow):
    """The row list of one batch for a BitmapRowGrad, on the current stream: gp_row_mark_mag over the batch of `call` (a
    mag._Call), gp_row_list_compact into a fresh int64 [capacity] and gp_row_list_zero of the listed rows of `rg.values`.
    Four launches, no host read.  Returns the keys; bit 0 of `overflow` is set when more than `capacity` rows were marked.
    A list that `rg.prelisted` holds (the deferred step made it before the forward, DESIGN §7za: the same batch, the same
    capacity, so the same list) is taken over instead of marking again: the zeroing alone is launched."""
    attr_indptr, attr_indices, _, col, _, filled, batch_rows, _ = call.tensors
    S_rows, K, B = call.scalars[:3]
    V, H = rg.shape
    keys, rg.prelisted = rg.prelisted, None
    if keys is None or keys.numel() != capacity:
        keys = list_rows(rg, V, attr_indptr, attr_indices, col, filled, S_rows, K, batch_rows, B, capacity, overflow)
    rc = _native.lib().gp_row_list_zero(rg.device.index, keys.data_ptr(), capacity, V, H, rg.values.data_ptr(), _stream(rg.values))
    _native.raise_for_status(rc)
    return keys


class DeferredRows:
    """The deferred exact Adam step of one [V, H] embedding table: the dense trajectory, bit for bit, at the
    memory traffic of the touched rows.  Made by `ClipAdam.set_row_grad(param, row_grad, "deferred", capacity=)`; one per table.

    Under dense Adam a row no batch touches still takes the zero-gradient update of every step.  Here that update is put off
    until the row is next read: `last` (int32 [V]) says which step each row is current through, `hist` is a ring of
    `capacity` 16-byte entries {step_size, rsqrt_bc2, coef, tag} with the entry of step s in slot s % capacity, and the
    missed steps are replayed in order through the dense step's own element update.  The step number is the optimiser's
    StepState tick, read on the device: the mode needs ClipAdam(capturable=True).  All state is device memory owned here;
    `bitmap`, `count` and `partials` are the workspace of `list_batch`.

      * `catch_up(keys)`: before the forward of a step (after `state.advance`), the rows listed in `keys` -- either kind
        of list: the deterministic backward's keys or the bitmap list -- are brought through the step before.
      * `step(...)`: what `ClipAdam.step()` calls in place of gp_clip_adam_rows_dev.
      * `flush()`: every row through the current tick; afterwards the table and both moments hold the dense step's bits.
        BETWEEN FLUSHES `param` AND THE MOMENTS SHOW LAGGING ROWS: flush before reading them.

    A row is served while tick - last[r] <= capacity, so a flush is due at least every `capacity` steps; a row that is not
    served keeps its bits and sets bit 1 of `flag` (int32 [1]; a caller's own flag word may be passed in)."""

    def __init__(self, optimizer, param, group_index, capacity=None, flag=None):
        self.capacity = check_capacity(capacity)
        self.optimizer, self.param, self.group_index = optimizer, param, group_index
        self.shape, self.device = tuple(param.shape), param.device
        if flag is not None and (not isinstance(flag, torch.Tensor) or flag.dtype != torch.int32 or flag.numel() != 1 or
                                 flag.device != param.device):
            raise TypeError(f"flag must be an int32 tensor of one element on {param.device}")
        V = self.shape[0]
        dev = param.device
        self.flag = flag if flag is not None else torch.zeros(1, dtype=torch.int32, device=dev)
        self.last = torch.zeros(V, dtype=torch.int32, device=dev)
        self.hist = torch.zeros(self.capacity * 4, dtype=torch.int32, device=dev)
        self.bitmap = torch.zeros((V + 31) // 32, dtype=torch.int32, device=dev)
        self.count = torch.zeros(1, dtype=torch.int64, device=dev)
        self.partials = torch.empty(ROW_LIST_PARTIALS, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self):
        """Every row is current through the state's tick as it stands and the ring is empty: at construction and after a
        checkpoint was loaded.  Device copies on the current stream, no host read."""
        tick = self.optimizer.step_state.buf[:1]
        self.last.copy_(tick.to(torch.int32).expand_as(self.last))
        self.hist.zero_()

    def _head(self):
        """The arguments every entry point begins with, and the ones every entry point ends with."""
        state = self.optimizer._init_state(self.param)
        return (self.device.index, self.param.data_ptr(), state["exp_avg"].data_ptr(), state["exp_avg_sq"].data_ptr())

    def _constants(self):
        group = self.optimizer.param_groups[self.group_index]
        beta1, beta2 = group["betas"]
        return float(beta1), float(beta2), float(group["eps"]), float(group["weight_decay"])

    def _tail(self):
        return (self.optimizer.step_state.buf.data_ptr(), self.last.data_ptr(), self.hist.data_ptr(), self.capacity,
                self.flag.data_ptr())

    def list_batch(self, attr_indptr, attr_indices, col, filled, S_rows, K, batch_rows, capacity, overflow):
        """`list_rows` of a batch over this object's bitmap: the list that `catch_up` takes before the forward."""
        B = S_rows if batch_rows is None else batch_rows.numel()
        return list_rows(self, self.shape[0], attr_indptr, attr_indices, col, filled, S_rows, K, batch_rows, B, capacity, overflow)

    def catch_up(self, keys):
        """gp_optim_defer_catch_up of an ascending int64 list on the current stream."""
        V, H = self.shape
        rc = _native.lib().gp_optim_defer_catch_up(*self._head(), keys.data_ptr(), keys.numel(), V, H, *self._constants(),
                                                   *self._tail(), _stream(self.param))
        _native.raise_for_status(rc)

    def step(self, rg, ws, norm, max_norm, d_step_size, d_rsqrt_bc2):
        """gp_optim_defer_step of a filled RowGrad: the workspace holds the norm's partials."""
        V, H = self.shape
        group = self.optimizer.param_groups[self.group_index]
        beta1, beta2, eps, weight_decay = self._constants()
        rc = _native.lib().gp_optim_defer_step(*self._head(), rg.values.data_ptr(), rg.keys.data_ptr(), rg.n_sorted, V, H, max_norm,
                                               float(group["lr"]), beta1, beta2, eps, weight_decay, d_step_size, d_rsqrt_bc2,
                                               *self._tail(), ws.data_ptr(), norm.data_ptr(), _stream(self.param))
        _native.raise_for_status(rc)

    def flush(self):
        """gp_optim_defer_flush on the current stream: one launch, capturable."""
        V, H = self.shape
        rc = _native.lib().gp_optim_defer_flush(*self._head(), V, H, *self._constants(), *self._tail(), _stream(self.param))
        _native.raise_for_status(rc)


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
