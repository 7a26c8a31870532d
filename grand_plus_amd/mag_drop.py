"""The deterministic table gradient of `mag_prop_rows` with input dropout: the backward built on
`gp_mag_prop_rows_backward_det_drop` of csrc/mag_drop_abi.hpp.

mag_det.py's backward sums the samples into one slot gradient U[e, :] before the gather.  With input dropout every
(sample, bag position, column) has a mask factor of its own, so here the slot gradient is kept per sample, U[s, e, :], and
the gather applies sample s's mask -- hashed from the seed, the sample, the RESIDENT slot r * K + k and t * H + h, as the
forward hashed it -- to U[s, e_j, :] * d_j before it sums the samples and then the entries, left to right from 0.0f.  Keys,
`slot_base`, `torch.sort(stable=True)` and the overflow flag are mag_det.py's, unchanged; nothing is read back, so the
backward runs under `torch.cuda.set_sync_debug_mode("error")` and inside a captured graph.

The seed may stand in device memory (an int64 [1] tensor): the kernels read it when they run, so a captured step draws a
fresh mask at every replay.  A call with such a seed and a hashed DropNode mask comes here too when no input-dropout mask is
drawn, because only these entry points read a device seed; the mask factor is then 1.

The entry points are extern "C" symbols of libgrandplus.so declared in csrc/mag_drop_abi.hpp; they are not part of C ABI 4,
so `_native.PRIVATE_ABI` binds them, not `_native.ABI`.

Left out: an explicit input-dropout mask, more than 16 samples.
"""
from __future__ import annotations

import ctypes

import torch

from . import _native
from ._common import _dev_index, _ptr, _stream

__all__ = ["backward_det_drop"]

_MAX_SLOTS = 2 ** 31


def lib():
    """`_native.lib()`, looked up at each call: this module binds nothing, and a patch of `_native.lib` reaches it."""
    return _native.lib()


def backward_det_drop(weight_shape, grad_out, call, max_entries, overflow, row_grad=None, segment_chunk=None):
    """dW [V, H] of mag_prop_rows by the order contract of mag_drop_abi.hpp.  The arguments and the returns are
    mag_det.backward_det's; `call.scalars`' seed may be an int or the int64 [1] device tensor.  Five launches (six with
    segment_chunk), torch.sort between the third and the fourth; the scratch U is S times backward_det's; no host read."""
    V, H = weight_shape
    attr_indptr, attr_indices, attr_data, col, val, filled, batch_rows, keep = call.tensors
    S_rows, K, B, S, p_node, p_in, training, seed = call.scalars
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
    L = lib()
    rc = L.gp_mag_det_keys(_dev_index(g), V, attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_indptr.numel() - 1,
                           col.data_ptr(), _ptr(filled), S_rows, K, _ptr(batch_rows), B, max_entries, slot_base.data_ptr(),
                           keys.data_ptr(), overflow.data_ptr(), _stream(g))
    _native.raise_for_status(rc)
    sorted_keys, order = torch.sort(keys, stable=True)
    U = torch.empty((S, B * K, H), dtype=torch.float32, device=dev)
    inv = torch.empty((S, B), dtype=torch.float32, device=dev)
    if segment_chunk is None:
        chunk, scratch_ptr, nbytes = 0, None, 0
    else:
        from . import gather_chunk
        scratch, nbytes = gather_chunk.scratch(max_entries, segment_chunk, H, dev)
        chunk, scratch_ptr = segment_chunk, scratch.data_ptr()
    seed_value, d_seed = (0, seed.data_ptr()) if call.dseed else (seed, None)
    rc = L.gp_mag_prop_rows_backward_det_drop(
        _dev_index(g), g.data_ptr(), V, H, attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_data.data_ptr(),
        attr_indptr.numel() - 1, col.data_ptr(), val.data_ptr(), _ptr(filled), S_rows, K, _ptr(batch_rows), B, S, float(p_node),
        float(p_in), int(bool(training)), ctypes.c_uint64(seed_value), d_seed, _ptr(keep), col.numel(), slot_base.data_ptr(),
        order.data_ptr(), sorted_keys.data_ptr(), max_entries, U.data_ptr(), inv.data_ptr(), dW.data_ptr(), chunk, scratch_ptr, nbytes,
        _stream(g))
    _native.raise_for_status(rc)
    if row_grad is None:
        return dW
    row_grad.fill(sorted_keys)
    return None
