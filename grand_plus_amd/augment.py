"""Feature augmentation ("random propagation") of GRAND+ on MI355X -- SURVEY.md 8(f) next-1.

Host-side mirror of `Grand_Plus.random_prop(feats, mat_scores, mat_idx, dropnode_rate)`
(`model.py:80-87`, `model_mag.py:80-86`) over the fused HIP kernels of csrc/augment.hip:

  * `random_prop`       -- the reference's own argument shape (gathered feats, scores, sorted ids);
  * `random_prop_rows`  -- the MI355X-native form: reads the `[S x K]` rows `Graph.gfpush_device`
                           left in HBM and the node-feature matrix, so the per-step scipy slicing,
                           host-side feature gather and upload of `model.py:310-316` disappear.

The reference's dropout draws from torch's global generator (`F.dropout`, `model.py:82`); here the
keep decision of entry e is a counter-based RNG of (seed, e), or an explicit `keep` mask.  Both keep
an entry with probability 1 - dropnode_rate and scale kept scores by 1/(1 - dropnode_rate).

Both are differentiable with respect to the feature operand (`feats` / `features`) when grad mode is on
and that tensor requires grad (MAG trains its embedding table through random_prop, model_mag.py:355-356).
Scores, `val` and `keep` are constants, as in the reference, where they come from numpy
(model_mag.py:342-343).  The backward kernels recompute the forward's mask from its seed.  Every other
call takes the plain path: same launch, same output, no grad_fn.

`samples=S` (2 <= S <= 16) runs the S augmentations of one training step (`--sample S`, model.py:321-322) in one
launch and returns [S, n_out, F]: out[s] equals, bit for bit, the single-sample call with
`sample_seed(seed, s)` (or with `keep[s]`) -- DESIGN §7e.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._common import _check, _deterministic, _dev_index, _new_seed, _ptr, _stream, sample_seed  # noqa: F401  (sample_seed: public here)

# In the helpers and Functions below `samples` is None for the single-sample C entry point (output [n_out, F]) or an int S for
# the S-sample one (output [S, n_out, F], S = 1 included).  The public functions pass None for samples=1.


def _check_samples(samples):
    if not isinstance(samples, int) or not 1 <= samples <= _native.GP_MAX_SAMPLES:
        raise ValueError(f"samples must be an int in [1, {_native.GP_MAX_SAMPLES}], got {samples!r}")


def _check_keep(keep, samples, L):
    """An explicit mask: uint8, L entries of the single call; [S, L] (or its flat form) for S samples, row s = the single call's keep."""
    _check(keep, torch.uint8, "keep")
    if samples is not None and keep.numel() != samples * L:
        raise ValueError(f"keep must hold samples x {L} = {samples * L} entries, got {keep.numel()}")


def _wants_grad(t):
    return torch.is_grad_enabled() and t.requires_grad


def _coo_forward(feats, mat_scores, mat_idx, n_out, samples, dropnode_rate, training, seed, keep, stream):
    M, F = feats.shape
    L = _native.lib()
    fn, shape, S = (L.gp_random_prop_coo, (n_out, F), ()) if samples is None else \
                   (L.gp_random_prop_coo_multi, (samples, n_out, F), (samples,))
    out = torch.empty(shape, dtype=torch.float32, device=feats.device)
    rc = fn(_dev_index(feats), feats.data_ptr(), M, F, mat_scores.data_ptr(), mat_idx.data_ptr(), n_out, *S,
            float(dropnode_rate), int(bool(training)), ctypes.c_uint64(seed), _ptr(keep), out.data_ptr(), _stream(feats, stream))
    _native.raise_for_status(rc)
    return out


def _coo_backward(grad_out, mat_scores, mat_idx, M, n_out, samples, dropnode_rate, training, seed, keep):
    g = grad_out.contiguous()
    F = g.shape[-1]
    L = _native.lib()
    fn, S = (L.gp_random_prop_coo_backward, ()) if samples is None else (L.gp_random_prop_coo_multi_backward, (samples,))
    if n_out == 0:                                                     # no launch: every entry is cut off
        return torch.zeros((M, F), dtype=torch.float32, device=g.device)
    # every row is written by the kernel: an entry's segment writes it, and entries with mat_idx >= n_out get exact zeros
    grad = torch.empty((M, F), dtype=torch.float32, device=g.device)
    rc = fn(_dev_index(g), g.data_ptr(), n_out, F, mat_scores.data_ptr(), mat_idx.data_ptr(), M, *S,
            float(dropnode_rate), int(bool(training)), ctypes.c_uint64(seed), _ptr(keep), grad.data_ptr(), _stream(g))
    _native.raise_for_status(rc)
    return grad


def _rows_forward(features, col, val, filled, K, batch_rows, B, samples, dropnode_rate, training, seed, keep, stream):
    N, F = features.shape
    L = _native.lib()
    fn, shape, S, stride = (L.gp_random_prop_rows, (B, F), (), ()) if samples is None else \
                           (L.gp_random_prop_rows_multi, (samples, B, F), (samples,), (col.numel(),))
    out = torch.empty(shape, dtype=torch.float32, device=features.device)
    rc = fn(_dev_index(features), features.data_ptr(), N, F, col.data_ptr(), val.data_ptr(), _ptr(filled), int(K),
            _ptr(batch_rows), B, *S, float(dropnode_rate), int(bool(training)), ctypes.c_uint64(seed), _ptr(keep), *stride,
            out.data_ptr(), _stream(features, stream))
    _native.raise_for_status(rc)
    return out


def _rows_backward(grad_out, col, val, filled, K, batch_rows, B, N, samples, dropnode_rate, training, seed, keep):
    g = grad_out.contiguous()
    F = g.shape[-1]
    L = _native.lib()
    fn, S, stride = (L.gp_random_prop_rows_backward, (), ()) if samples is None else \
                    (L.gp_random_prop_rows_multi_backward, (samples,), (col.numel(),))
    grad = torch.zeros((N, F), dtype=torch.float32, device=g.device)
    rc = fn(_dev_index(g), g.data_ptr(), B, F, col.data_ptr(), val.data_ptr(), _ptr(filled), int(K), _ptr(batch_rows), *S,
            float(dropnode_rate), int(bool(training)), ctypes.c_uint64(seed), _ptr(keep), *stride, grad.data_ptr(), N, _stream(g))
    _native.raise_for_status(rc)
    return grad


def _rows_det_order(col, filled, K, batch_rows, N):
    """The sorted order the deterministic backward takes: (order, keys).  All B*K slots of the batch, entry e = b*K + k,
    keyed by their column id, or by the sentinel N when the slot is unfilled or its id outside [0, N), so that it sorts
    last; a stable sort by key.  Device ops only: nothing here reads the host."""
    cols = col.view(-1, K) if batch_rows is None else col.view(-1, K)[batch_rows.long()]
    live = (cols >= 0) & (cols < N)
    if filled is not None:
        n = filled if batch_rows is None else filled[batch_rows.long()]
        live &= torch.arange(K, device=col.device)[None, :] < n[:, None]
    keys, order = torch.sort(torch.where(live, cols.long(), N).reshape(-1), stable=True)
    return order, keys


def _rows_backward_det(grad_out, col, val, filled, K, batch_rows, B, N, samples, dropnode_rate, training, seed, keep,
                       segment_chunk=None):
    """_rows_backward without atomics (csrc/scatter_det.hip): the batch's slots ordered by column id
    (_rows_det_order), one gather kernel that sums each gradient row in that order.  segment_chunk = C: the chunked gather
    of DESIGN §7w over the same order, two kernels and a scratch."""
    g = grad_out.contiguous()
    F = g.shape[-1]
    grad = torch.zeros((N, F), dtype=torch.float32, device=g.device)
    if B == 0:
        return grad
    order, keys = _rows_det_order(col, filled, int(K), batch_rows, N)
    S = 1 if samples is None else samples
    inv_den = torch.empty(_native.scatter_rows_workspace_bytes(S, B) // 4, dtype=torch.float32, device=g.device)
    args = (_dev_index(g), g.data_ptr(), B, F, col.data_ptr(), val.data_ptr(), _ptr(filled), int(K), _ptr(batch_rows), S,
            float(dropnode_rate), int(bool(training)), ctypes.c_uint64(seed), _ptr(keep), col.numel(), grad.data_ptr(), N,
            order.data_ptr(), keys.data_ptr(), keys.numel(), inv_den.data_ptr())
    if segment_chunk is None:
        rc = _native.lib().gp_random_prop_rows_backward_det(*args, _stream(g))
    else:
        from . import gather_chunk
        scratch, nbytes = gather_chunk.scratch(keys.numel(), segment_chunk, F, g.device)
        rc = _native.lib().gp_random_prop_rows_backward_det_chunked(*args, segment_chunk, scratch.data_ptr(), nbytes, _stream(g))
    _native.raise_for_status(rc)
    return grad


# Both forward helpers under the names the S-sample ones had before the single and S-sample forms were merged (same arguments):
# tests/test_gpu_multisample.py reaches the S-sample entry points with S = 1 through them.
_coo_multi_forward, _rows_multi_forward = _coo_forward, _rows_forward


class _CooFn(torch.autograd.Function):
    """random_prop with the gradient to feats (summed over the samples of an S-sample call)."""

    @staticmethod
    def forward(ctx, feats, mat_scores, mat_idx, n_out, samples, dropnode_rate, training, seed, keep, stream):
        ctx.save_for_backward(mat_scores, mat_idx, keep)
        ctx.args = (feats.shape[0], n_out, samples, dropnode_rate, training, seed)
        return _coo_forward(feats, mat_scores, mat_idx, n_out, samples, dropnode_rate, training, seed, keep, stream)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        mat_scores, mat_idx, keep = ctx.saved_tensors
        return (_coo_backward(grad_out, mat_scores, mat_idx, *ctx.args, keep),) + (None,) * 9


class _RowsFn(torch.autograd.Function):
    """random_prop_rows with the gradient to features (summed over the samples of an S-sample call)."""

    @staticmethod
    def forward(ctx, features, col, val, filled, K, batch_rows, B, samples, dropnode_rate, training, seed, keep, stream,
                deterministic=False, segment_chunk=None):
        ctx.save_for_backward(col, val, filled, batch_rows, keep)
        ctx.args = (K, B, features.shape[0], samples, dropnode_rate, training, seed)
        ctx.deterministic, ctx.segment_chunk = deterministic, segment_chunk
        return _rows_forward(features, col, val, filled, K, batch_rows, B, samples, dropnode_rate, training, seed, keep, stream)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        col, val, filled, batch_rows, keep = ctx.saved_tensors
        K, B, *rest = ctx.args
        if not ctx.deterministic:
            grad = _rows_backward(grad_out, col, val, filled, K, batch_rows, B, *rest, keep)
        else:
            grad = _rows_backward_det(grad_out, col, val, filled, K, batch_rows, B, *rest, keep, ctx.segment_chunk)
        return (grad,) + (None,) * 14


def random_prop(feats, mat_scores, mat_idx, dropnode_rate, training=True, seed=None, keep=None, stream=None,
                samples=1, n_out=None):
    """Drop-in for `Grand_Plus.random_prop` (`model.py:80-87`) on CUDA tensors.

    feats [M, F] float32, mat_scores [M] float32, mat_idx [M] int64 sorted ascending (the order
    scipy's `.nonzero()` yields, `model.py:312`).  Returns [mat_idx[-1] + 1, F] float32.
    `training` plays the role of `self.training`.  Differentiable with respect to `feats`.
    `n_out` (optional) is the number of output rows; given, it saves the host read of mat_idx[-1].  Above mat_idx[-1] + 1
    it adds zero rows; below, the output is the first n_out rows and the entries of later rows get a gradient of exactly 0.
    `samples` = S > 1 returns [S, n_out, F] from one launch (keep: uint8 [S, M]); see the module docstring.
    """
    _check_samples(samples)
    _check(feats, torch.float32, "feats")
    _check(mat_scores, torch.float32, "mat_scores")
    _check(mat_idx, torch.int64, "mat_idx")
    M, F = feats.shape
    if mat_scores.numel() != M or mat_idx.numel() != M:
        raise ValueError("feats, mat_scores and mat_idx must have the same number of entries")
    if n_out is None:
        if M == 0:
            return feats.new_zeros((0, F)) if samples == 1 else feats.new_zeros((samples, 0, F))
        n_out = int(mat_idx[-1].item()) + 1                               # model.py:84 dim_size
    elif int(n_out) < 0:
        raise ValueError("n_out must be >= 0")
    n_out = int(n_out)
    if seed is None:
        seed = _new_seed()
    samples = None if samples == 1 else samples
    if samples is None and M == 0:
        return feats.new_zeros((n_out, F))
    if keep is not None:
        _check_keep(keep, samples, M)
    args = (feats, mat_scores, mat_idx, n_out, samples, dropnode_rate, training, seed, keep, stream)
    return _CooFn.apply(*args) if _wants_grad(feats) else _coo_forward(*args)   # gradient to feats only (model_mag.py:355)


def random_prop_rows(features, col, val, filled, K, batch_rows=None, dropnode_rate=0.5, training=True,
                     seed=None, keep=None, stream=None, samples=1, deterministic=None, segment_chunk=None):
    """Fused augmentation straight from the GFPush row matrix.

    features [N, F] float32 (node features resident on the GPU); col int32 [S*K], val float64 [S*K],
    filled int32 [S] as returned by `Graph.gfpush_device`; batch_rows int32 [B] = positions of the
    batch's seeds in the seed list (None = all S rows).  Returns [B, F] float32:
        out[b] = sum_k w_k X[col[r,k]] / (sum_k w_k + 1e-12),  r = batch_rows[b]
    Differentiable with respect to `features` (the backward adds into a dense [N, F] gradient with fp32
    atomics: not bitwise reproducible unless `deterministic=True`).
    `deterministic` chooses the backward alone; the forward is the same bit for bit.  False: the atomic kernel.  True: the
    batch's slots are sorted by column id and each gradient row is summed in a fixed order with plain stores (DESIGN §7i;
    slower, bitwise the same run to run, no host synchronisation).  None follows
    `torch.are_deterministic_algorithms_enabled()`.
    `segment_chunk` = C (a power of two in [64, 4096]; None: off) cuts the deterministic backward's segment sums into
    chunks of C entries summed by separate waves and folded in a fixed order: a node that sits in many rows is
    no longer one serial chain.  Still bitwise the same run to run; a node with at most C entries gets the unchunked bits.
    It needs the deterministic backward: ValueError when the mode resolves to False.
    `samples` = S > 1 returns [S, B, F] from one launch (keep: uint8 [S, S_rows * K]); see the module docstring.
    """
    deterministic = _deterministic(deterministic)
    from .gather_chunk import resolve
    segment_chunk = resolve(segment_chunk, deterministic, "random_prop_rows")
    _check_samples(samples)
    _check(features, torch.float32, "features")
    _check(col, torch.int32, "col")
    _check(val, torch.float64, "val")
    N, F = features.shape
    S = col.numel() // K
    if filled is not None:
        _check(filled, torch.int32, "filled")
    if batch_rows is not None:
        _check(batch_rows, torch.int32, "batch_rows")
    B = S if batch_rows is None else batch_rows.numel()
    if seed is None:
        seed = _new_seed()
    samples = None if samples == 1 else samples
    if keep is not None:
        _check_keep(keep, samples, col.numel())
    args = (features, col, val, filled, K, batch_rows, B, samples, dropnode_rate, training, seed, keep, stream)
    return _RowsFn.apply(*args, deterministic, segment_chunk) if _wants_grad(features) else _rows_forward(*args)


def algorithmic_bytes(n_kept_entries: int, n_out: int, feat_dim: int) -> int:
    """HBM gather bound of SURVEY.md 8(f): one feature row per kept neighbour + the output rows."""
    return 4 * feat_dim * (n_kept_entries + n_out) + 16 * n_kept_entries
