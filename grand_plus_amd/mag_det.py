"""The deterministic table gradient of `mag_prop_rows`: the backward built on the entry points of
csrc/mag_det_abi.hpp.

The atomic backward of mag.py adds one fp32 atomic per (entry, column) into dW: fast, capturable, not reproducible.  The
composed path has a deterministic backward, but it asks the host how many entries the batch has.  Here the host never
learns that number: the caller fixes a capacity `max_entries` beforehand, `gp_mag_det_keys` writes the entries' attribute
ids into a key buffer of that size (sentinel V in the tail, a flag instead of a write past the end), `torch.sort(stable=True)`
orders them, and `gp_mag_prop_rows_backward_det` sums every table row's contributions in entry order (b, k, t), left to
right from 0.0f.  Nothing is read back, so the backward runs under `torch.cuda.set_sync_debug_mode("error")` and inside a
captured graph.

The entry points are extern "C" symbols of libgrandplus.so declared in csrc/mag_det_abi.hpp; they are not part of C ABI 4,
so `_native.PRIVATE_ABI` binds them, not `_native.ABI`.

`segment_chunk=C` sums a hub attribute's segment in chunks of C entries (gather_chunk.py).

Input dropout is not this backward's: its keyed mask needs S values of U per slot, which mag_drop.py keeps
(`mag_prop_rows(..., det_input_dropout=True)`); `backward_det` and its two entry points refuse it.
"""
from __future__ import annotations

import torch

from . import _native
from ._common import _dev_index, _ptr, _stream

__all__ = ["backward_det", "check_max_entries", "check_overflow"]

_MAX_SLOTS = 2 ** 31


def lib():
    """`_native.lib()`, looked up at each call: this module binds nothing, and a patch of `_native.lib` reaches it."""
    return _native.lib()


def check_max_entries(max_entries):
    """`max_entries` as an int >= 1 (ValueError otherwise): the capacity of the key buffer, in entries."""
    if isinstance(max_entries, bool) or not isinstance(max_entries, int) or max_entries < 1:
        raise ValueError(f"max_entries must be an int >= 1, got {max_entries!r}")
    return max_entries


def check_overflow(overflow, device):
    """`overflow` as the int32 [1] tensor on `device` that receives the overflow flag (TypeError otherwise)."""
    if not isinstance(overflow, torch.Tensor) or overflow.dtype != torch.int32 or overflow.numel() != 1 or \
            not overflow.is_contiguous() or overflow.device != device:
        raise TypeError(f"overflow must be a contiguous int32 tensor of one element on {device}")
    return overflow


def backward_det(weight_shape, grad_out, call, max_entries, overflow, row_grad=None, segment_chunk=None):
    """dW [V, H] of mag_prop_rows by the order contract of mag_det_abi.hpp.  call: mag._Call, the forward's operands;
    overflow: int32 [1], bit 0 is set when the batch has more than max_entries entries (the gradient then lacks the rest).
    Six launches, torch.sort between the third and the fourth; no host read.
    row_grad: an optim_rows.RowGrad.  The gather then writes the touched rows into `row_grad.values`, which
    nobody zeroes, the RowGrad takes the sorted key list over, and None is returned in place of dW.
    segment_chunk: None, or the chunk C of the chunked gather: one launch and a scratch more, the same keys."""
    V, H = weight_shape
    attr_indptr, attr_indices, attr_data, col, val, filled, batch_rows, keep = call.tensors
    S_rows, K, B, S, p_node, p_in, training, seed = call.scalars
    if training and p_in > 0.0:
        raise ValueError("the deterministic backward of mag_prop_rows does not support input dropout (DESIGN §9)")
    if B * K >= _MAX_SLOTS:
        raise ValueError(f"the deterministic backward of mag_prop_rows takes fewer than 2**31 slots, got {B} x {K}")
    g = grad_out.contiguous()
    dev = g.device
    dW = torch.zeros((V, H), dtype=torch.float32, device=dev) if row_grad is None else row_grad.values
    if B == 0:
        if row_grad is None:
            return dW
        row_grad.fill(torch.full((1,), V, dtype=torch.int64, device=dev))       # the sentinel alone: no row is touched
        return None
    slot_base = torch.empty(B * K + 1, dtype=torch.int64, device=dev)
    keys = torch.empty(max_entries, dtype=torch.int64, device=dev)
    L = _native.lib()
    rc = L.gp_mag_det_keys(_dev_index(g), V, attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_indptr.numel() - 1,
                           col.data_ptr(), _ptr(filled), S_rows, K, _ptr(batch_rows), B, max_entries, slot_base.data_ptr(),
                           keys.data_ptr(), overflow.data_ptr(), _stream(g))
    _native.raise_for_status(rc)
    sorted_keys, order = torch.sort(keys, stable=True)
    U = torch.empty((B * K, H), dtype=torch.float32, device=dev)
    inv = torch.empty((S, B), dtype=torch.float32, device=dev)
    args = (_dev_index(g), g.data_ptr(), V, H, *call.args(), slot_base.data_ptr(), order.data_ptr(), sorted_keys.data_ptr(),
            max_entries, U.data_ptr(), inv.data_ptr(), dW.data_ptr())
    if segment_chunk is None:
        rc = L.gp_mag_prop_rows_backward_det(*args, _stream(g))
    else:
        from . import gather_chunk
        scratch, nbytes = gather_chunk.scratch(max_entries, segment_chunk, H, dev)
        rc = L.gp_mag_prop_rows_backward_det_chunked(*args, segment_chunk, scratch.data_ptr(), nbytes, _stream(g))
    _native.raise_for_status(rc)
    if row_grad is None:
        return dW
    row_grad.fill(sorted_keys)
    return None
