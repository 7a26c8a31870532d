"""MAG's front end fused on the resident rows: `MLP.emb` of every neighbour of a batch followed by
`random_prop` (model_mag.py:48-55, 80-86, 354-356) as ONE op over csrc/mag_prop.hip, and MAG's `valid` / `predict` over it.

    e_{s,k}   = sum_t dropout(W[a_t], input_droprate) * d_t / (sum_t d_t + 1e-10)        t over the bag of col[r, k]
    out[s, b] = sum_k w'_{s,k} e_{s,k} / (sum_k w'_{s,k} + 1e-12),   w' = float(val[r, k]) * DropNode mask,  r = batch_rows[b]

`mag_prop_rows` replaces `flatten_rows -> embedding_bag_csr(nodes=...) -> random_prop(..., samples=S)`: one launch forward,
`torch.zeros` and one launch backward, no [B*K, H] intermediate, no bag layout rebuilt per call and no host read, so a MAG
step runs under `torch.cuda.set_sync_debug_mode("error")` like every other step here.  The DropNode mask is
`random_prop_rows`'s for the same seed (entry r*K + k); the input dropout of (sample s, slot e, bag position t, column h)
is keyed (`mag_slot_seed(seed, s, e)`, t*H + h).  out[s] of an S-sample call equals the single-sample call with
`sample_seed(seed, s)` (or `keep[s]`) bit for bit, and the forward is bitwise the same run to run.

The gradient reaches `weight` only.  By default the backward adds into a dense dW with fp32 atomics: fast, and not bitwise
reproducible.  The deterministic backward (mag_det.py) needs a capacity for its key buffer, because the host
never learns how many entries a batch has: with `max_entries=` given, a call in deterministic mode (`deterministic=True`, or
torch's deterministic mode) takes it -- keys, `torch.sort(stable=True)`, a sequential sum per table row, no host read, the
same bits run to run.  Without `max_entries` such a call still raises and names the composed path.  With `max_entries` and
the mode resolving to non-deterministic the atomic backward runs and `max_entries` is ignored, so a caller may pass it always
and let torch's flag decide.  The forward is the same in every mode.  There is no CPU fallback.

With input dropout the deterministic backward is mag_drop.py's (`det_input_dropout=True`), and `seed=` may be
an int64 [1] device tensor that the kernels read when they run, so that a captured call draws fresh masks at every replay.

Either backward can hand the table's gradient to the optimiser as a row list instead of a dense tensor (`row_grad=`): the
deterministic one its sorted keys (an `optim_rows.RowGrad`), the atomic one the rows it marked in a bitmap (an
`optim_rows.BitmapRowGrad`).

`valid_mag` is `valid_mag_pass(valid_mag_plan(...))`, as `evaluate.valid` is `valid_pass(valid_plan(...))`: the fit loop
 plans once and passes at every validation.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._common import _check, _deterministic, _dev_index, _new_seed, _ptr, _stream


class _Call:
    """The constant operands of one call, which the forward and the backward pass to the library alike: the attribute
    CSR, the resident rows, the batch and the masks' parameters."""

    def __init__(self, tensors, S_rows, K, B, samples, p_node, p_in, training, seed):
        self.tensors = tensors             # attr_indptr, attr_indices, attr_data, col, val, filled, batch_rows, keep
        self.scalars = (S_rows, K, B, samples, p_node, p_in, training, seed)

    @property
    def dseed(self):
        """Whether the seed stands in device memory (an int64 [1] tensor): the call then goes to the entry
        points of csrc/mag_drop_abi.hpp, which take its address where the value forms take the value."""
        return isinstance(self.scalars[7], torch.Tensor)

    def entry(self, name):
        """The entry point `name` of grandplus_mag.h, or its device-seed form."""
        return getattr(_native.lib(), name + "_dseed" if self.dseed else name)

    def args(self):
        attr_indptr, attr_indices, attr_data, col, val, filled, batch_rows, keep = self.tensors
        S_rows, K, B, samples, p_node, p_in, training, seed = self.scalars
        return (attr_indptr.data_ptr(), attr_indices.data_ptr(), attr_data.data_ptr(), attr_indptr.numel() - 1, col.data_ptr(),
                val.data_ptr(), _ptr(filled), S_rows, K, _ptr(batch_rows), B, samples, float(p_node), float(p_in),
                int(bool(training)), seed.data_ptr() if self.dseed else ctypes.c_uint64(seed), _ptr(keep), col.numel())


def _forward(weight, call, n_bad):
    V, H = weight.shape
    _, _, B, S = call.scalars[:4]
    out = torch.empty((S, B, H), dtype=torch.float32, device=weight.device)
    rc = call.entry("gp_mag_prop_rows")(_dev_index(weight), weight.data_ptr(), V, H, *call.args(), out.data_ptr(), n_bad.data_ptr(),
                                        _stream(weight))
    _native.raise_for_status(rc)
    return out


def _backward(weight_shape, grad_out, call):
    V, H = weight_shape
    g = grad_out.contiguous()
    dW = torch.zeros((V, H), dtype=torch.float32, device=g.device)
    rc = call.entry("gp_mag_prop_rows_backward")(_dev_index(g), g.data_ptr(), V, H, *call.args(), dW.data_ptr(), _stream(g))
    _native.raise_for_status(rc)
    return dW


def _backward_rows(weight_shape, grad_out, call, capacity, overflow, row_grad):
    """The atomic backward into a BitmapRowGrad: mark the rows the batch can touch, compact them into a list of
    `capacity` keys, zero those rows of `row_grad.values`, then the atomic launch of `_backward` into that buffer.  Five
    launches, no `torch.zeros` of [V, H], no host read.  Bit 0 of `overflow` is set when the batch marked more rows than
    `capacity`; the adds into the rows past it land in memory nobody reads."""
    from .optim_rows import mark_and_list
    V, H = weight_shape
    g = grad_out.contiguous()
    if call.scalars[2] == 0:
        row_grad.fill(torch.full((1,), V, dtype=torch.int64, device=g.device))   # the sentinel alone: no row is touched
        return None
    keys = mark_and_list(row_grad, call, capacity, overflow)
    rc = call.entry("gp_mag_prop_rows_backward")(_dev_index(g), g.data_ptr(), V, H, *call.args(), row_grad.values.data_ptr(),
                                                 _stream(g))
    _native.raise_for_status(rc)
    row_grad.fill(keys)
    return None


class _MagRowsFn(torch.autograd.Function):
    """mag_prop_rows with the gradient to weight (summed over the samples)."""

    @staticmethod
    def forward(ctx, weight, call, n_bad, det=None):
        """det: None for the atomic backward, (max_entries, overflow, row_grad, segment_chunk, per_sample) for the
        deterministic one (mag_det.backward_det, or with per_sample mag_drop.backward_det_drop: input dropout or a device
        seed); with a row_grad the weight's gradient is None and dW goes to the RowGrad.
        (capacity, overflow, a BitmapRowGrad): the atomic backward into that row gradient (`_backward_rows`)."""
        ctx.save_for_backward(*call.tensors)
        ctx.args = (weight.shape, call.scalars, det)
        return _forward(weight, call, n_bad)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        shape, scalars, det = ctx.args
        call = _Call(ctx.saved_tensors, *scalars)
        if det is None:
            return _backward(shape, grad_out, call), None, None, None
        from .optim_rows import BitmapRowGrad
        if isinstance(det[2], BitmapRowGrad):
            return _backward_rows(shape, grad_out, call, *det), None, None, None
        if det[4]:
            from .mag_drop import backward_det_drop
            return backward_det_drop(shape, grad_out, call, *det[:4]), None, None, None
        from .mag_det import backward_det
        return backward_det(shape, grad_out, call, *det[:4]), None, None, None


def mag_prop_rows(weight, attr_indptr, attr_indices, attr_data, col, val, filled, K, batch_rows=None, *, samples=1,
                  dropnode_rate=0.5, input_droprate=0.0, training=True, seed=None, keep=None, validate=False, deterministic=None,
                  max_entries=None, overflow=None, row_grad=None, segment_chunk=None, det_input_dropout=False):
    """The S augmented embeddings of a batch of resident rows, in one launch.

    weight [V, H] float32 (the `nn.Embedding` table); attr_indptr [N + 1] int64, attr_indices [nnz] int32, attr_data [nnz]
    float32 (the node-attribute CSR resident on the GPU); col int32 [S_rows * K], val float64 [S_rows * K], filled int32
    [S_rows] or None (every slot filled) as `Graph.gfpush_device` returns them; batch_rows int32 [B] (None: every row).
    Returns [B, H] float32 for samples = 1 and [S, B, H] otherwise (keep: uint8 [S, S_rows * K], the DropNode mask of
    `random_prop_rows`).  Differentiable with respect to `weight`: by default `torch.zeros` and one launch, fp32 atomics.
    A batch row outside [0, S_rows), a column outside [0, N) and an attribute id outside [0, V) are never used as an
    address; they contribute nothing and are counted: validate=True reads the count back (the only host read of this
    function) and raises IndexError.
    `deterministic`: None follows `torch.are_deterministic_algorithms_enabled()`.  When it resolves to True and a gradient
    is wanted, the backward is the deterministic one of DESIGN §7o if `max_entries` (an int >= 1: the capacity of its key
    buffer, an upper bound of sum over the batch's slots of the slot's bag length) is given; without `max_entries` the call
    raises RuntimeError.  It never reads the host: `overflow` (an int32 [1] tensor on weight's device; a private one
    that nobody reads when omitted) gets bit 0 set by the backward if the batch had more entries than `max_entries`, and
    the gradient then lacks the entries past it.  Input dropout (input_droprate > 0 while training) is not supported by that
    backward: ValueError, unless `det_input_dropout=True` (below).  When the mode resolves to False `max_entries` is ignored.
    `seed`: an int, or a contiguous int64 tensor of one element on weight's device: the kernels then read the
    seed, as a uint64, from that address when they run, so a captured call draws the masks of the value that stands there at
    each replay.  With the value v there the forward is bit for bit the call with seed=v.  Any other tensor: TypeError.
    `det_input_dropout=True` lets the deterministic backward run with input dropout: it keeps the slot
    gradient per sample (S times the scratch) and applies every sample's own mask in the gather (mag_drop.py).  It needs
    the mode to resolve to deterministic and `max_entries` (ValueError otherwise), goes with `row_grad` and
    `segment_chunk`, and changes nothing where no mask is drawn (input_droprate = 0, or eval mode).
    `row_grad`: an `optim_rows.RowGrad(weight)`.  The deterministic backward then writes dW into its persistent
    buffer instead of a fresh `torch.zeros`, hands it the sorted key list and returns no gradient for `weight`
    (`weight.grad` stays None): the table is stepped by `ClipAdam.set_row_grad`.  It needs the deterministic mode and
    `max_entries` (ValueError with the atomic mode or without a capacity) and must be the RowGrad of this very `weight`
    (TypeError / ValueError).  The forward is the same.
    An `optim_rows.BitmapRowGrad(weight)` is the same for the ATOMIC backward: it needs the mode to resolve to
    non-deterministic and `max_entries` (ValueError otherwise).  The backward marks the rows the batch's bags name in the
    BitmapRowGrad's bitmap, compacts them into a fresh int64 [min(V, max_entries)] list, zeroes those rows of its buffer and
    runs the atomic launch into it: no `torch.zeros` of [V, H], no host read, input dropout allowed.  The list holds every
    row a slot of the batch names, dropped by DropNode or not.  If the batch names more rows than the list holds, bit 0 of
    `overflow` is set and the list lacks the rows past it.
    `segment_chunk` = C (a power of two in [64, 4096]; None: off) cuts the deterministic backward's sums into chunks of C
    entries (gather_chunk.py): an attribute that sits in many bags of the batch is no longer one serial chain.
    Still no host read and the same bits run to run; with `row_grad` the rows and the key list are the unchunked call's.  It
    needs the mode to resolve to deterministic (ValueError otherwise)."""
    deterministic = _deterministic(deterministic)
    from .gather_chunk import resolve
    segment_chunk = resolve(segment_chunk, deterministic, "mag_prop_rows")
    if max_entries is not None:
        from .mag_det import check_max_entries
        check_max_entries(max_entries)
    if not isinstance(det_input_dropout, bool):
        raise TypeError(f"det_input_dropout must be True or False, got {det_input_dropout!r}")
    if det_input_dropout and (not deterministic or max_entries is None):
        raise ValueError("det_input_dropout=True is the deterministic backward's: it needs deterministic=True (or torch's "
                         "deterministic mode) and max_entries= (DESIGN §7y)")
    if not isinstance(samples, int) or not 1 <= samples <= _native.GP_MAX_SAMPLES:
        raise ValueError(f"samples must be an int in [1, {_native.GP_MAX_SAMPLES}], got {samples!r}")
    _check(weight, torch.float32, "weight")
    if weight.dim() != 2 or weight.shape[0] < 1 or weight.shape[1] < 1:
        raise TypeError("weight must be a 2-D [V, H] table")
    if row_grad is not None:
        from .optim_rows import BitmapRowGrad, RowGrad
        if not isinstance(row_grad, RowGrad):
            raise TypeError(f"row_grad must be an optim_rows.RowGrad, got {type(row_grad).__name__}")
        if isinstance(row_grad, BitmapRowGrad):
            if deterministic:
                raise ValueError("a BitmapRowGrad is the atomic backward's row gradient: deterministic=False (and torch's "
                                 "deterministic mode off); the deterministic backward takes a plain optim_rows.RowGrad")
            if max_entries is None:
                raise ValueError("a BitmapRowGrad needs max_entries=: the capacity of its row list is min(V, max_entries)")
        elif not deterministic or max_entries is None:
            raise ValueError("row_grad needs the deterministic backward: deterministic=True (or torch's deterministic mode) and "
                             "max_entries=; the atomic backward keeps no list of the rows it touched (DESIGN §9)")
        row_grad.check_weight(weight)
    _check(attr_indptr, torch.int64, "attr_indptr")
    _check(attr_indices, torch.int32, "attr_indices")
    _check(attr_data, torch.float32, "attr_data")
    if attr_indptr.numel() < 1 or attr_data.numel() != attr_indices.numel():
        raise ValueError("attr_indptr needs N + 1 entries; attr_indices and attr_data the same length")
    _check(col, torch.int32, "col")
    _check(val, torch.float64, "val")
    K = int(K)
    if not 1 <= K <= _native.GP_MAX_K:
        raise ValueError(f"K must be in [1, {_native.GP_MAX_K}], got {K}")
    if col.numel() % K or val.numel() != col.numel():
        raise ValueError("col and val must hold S_rows * K entries each")
    S_rows = col.numel() // K
    if filled is not None:
        _check(filled, torch.int32, "filled")
        if filled.numel() != S_rows:
            raise ValueError(f"filled must hold one entry per row ({S_rows}), got {filled.numel()}")
    if batch_rows is not None:
        _check(batch_rows, torch.int32, "batch_rows")
    B = S_rows if batch_rows is None else batch_rows.numel()
    for name, p in (("dropnode_rate", dropnode_rate), ("input_droprate", input_droprate)):
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"{name} must lie in [0, 1]")
    if keep is not None:
        _check(keep, torch.uint8, "keep")
        if keep.numel() != samples * col.numel():
            raise ValueError(f"keep must hold samples x {col.numel()} = {samples * col.numel()} entries, got {keep.numel()}")
    for name, t in (("attr_indptr", attr_indptr), ("attr_indices", attr_indices), ("attr_data", attr_data), ("col", col), ("val", val),
                    ("filled", filled), ("batch_rows", batch_rows), ("keep", keep)):
        if t is not None and t.device != weight.device:
            raise TypeError(f"{name} must be on {weight.device}, got {t.device} (no CPU fallback)")
    device_seed = isinstance(seed, torch.Tensor)
    if device_seed and (seed.dtype != torch.int64 or seed.numel() != 1 or not seed.is_contiguous() or seed.device != weight.device):
        raise TypeError(f"seed must be an int, or a contiguous int64 tensor of one element on {weight.device} (DESIGN §7y)")
    masked = bool(training) and float(input_droprate) > 0.0
    if device_seed and not masked and (keep is not None or not training):
        seed = 0                                                       # no mask is hashed: nothing reads the seed
        device_seed = False
    wants_grad = torch.is_grad_enabled() and weight.requires_grad
    det = None
    if deterministic and wants_grad and max_entries is not None:
        from .mag_det import check_overflow
        if masked and not det_input_dropout:
            raise ValueError("the deterministic backward of mag_prop_rows does not support input dropout (DESIGN §9): "
                             "input_droprate must be 0 in training")
        if B * K >= 2 ** 31:
            raise ValueError(f"the deterministic backward of mag_prop_rows takes fewer than 2**31 slots, got {B} x {K}")
        if overflow is not None:
            check_overflow(overflow, weight.device)
        # the per-sample backward: a mask per sample, or a seed that only the entry points of mag_drop_abi.hpp read
        det = (max_entries, overflow if overflow is not None else torch.zeros(1, dtype=torch.int32, device=weight.device), row_grad,
               segment_chunk, masked or device_seed)
    elif deterministic and wants_grad:
        raise RuntimeError("mag_prop_rows has no deterministic backward (fp32 atomics into dW); for a reproducible gradient use the "
                           "composed path with deterministic=True: flatten_rows -> embedding_bag_csr(nodes=..., deterministic=True) "
                           "-> random_prop, or pass max_entries= for the deterministic backward of this op (DESIGN §7o)")
    elif row_grad is not None and wants_grad:                          # a BitmapRowGrad: the atomic backward into its rows
        from .mag_det import check_overflow
        if B * K >= 2 ** 31:
            raise ValueError(f"the row list of mag_prop_rows takes fewer than 2**31 slots, got {B} x {K}")
        if overflow is not None:
            check_overflow(overflow, weight.device)
        det = (min(weight.shape[0], max_entries),
               overflow if overflow is not None else torch.zeros(1, dtype=torch.int32, device=weight.device), row_grad)
    if seed is None:
        seed = _new_seed()
    call = _Call((attr_indptr, attr_indices, attr_data, col, val, filled, batch_rows, keep), S_rows, K, B, samples,
                 float(dropnode_rate), float(input_droprate), bool(training), seed)
    n_bad = torch.zeros(1, dtype=torch.int32, device=weight.device)
    out = _MagRowsFn.apply(weight, call, n_bad, det) if wants_grad else _forward(weight, call, n_bad)
    if validate:
        bad = int(n_bad.item())
        if bad:
            raise IndexError(f"mag_prop_rows: {bad} batch row(s), column(s) or attribute id(s) out of range")
    return out[0] if samples == 1 else out


def valid_mag(model, rows, attr_indptr, attr_indices, attr_data, idx_val, labels, batch_size=100, dropnode_rate=0.5,
              return_counts=False):
    """MAG's `valid` (model_mag.py:145-177) on the GPU: (loss, acc) as 0-dim float32 device tensors.

    model: a MagMLP; rows: the RowMatrix that holds `topk_adj`; the node-attribute CSR as for `mag_prop_rows`; idx_val: the
    validation node ids (every one a seed of `rows`); labels int64 CUDA [N].  The positions of idx_val are looked up once
    (one check, KeyError for a node that is no seed); then per batch `model.emb_rows` in eval mode (only the batch's
    neighbours are embedded, with the weights as they are now), the MLP and `eval_head` into one shared buffer, and one
    `eval_reduce`: nothing synchronises.  The model's training flag is restored.  Same returns as `valid`.  The one-pass
    form is `valid_mag_pass(valid_mag_plan(..., one_pass=True))`."""
    plan = valid_mag_plan(model, rows, attr_indptr, attr_indices, attr_data, idx_val, labels, batch_size)
    loss, acc, counts = valid_mag_pass(plan, dropnode_rate)
    return (loss, acc, counts) if return_counts else (loss, acc)


class ValidMagPlan(NamedTuple):
    """What `valid_mag` prepares once for a validation set: its arguments as checked, the node ids on the device, their
    positions in `rows` and the evaluation buffers.  Nothing in it depends on the weights: `valid_mag_pass` runs over it any
    number of times (the fit loop) and sees the table as it is at that moment.  `one` is None, or the
    evaluate.OnePass of a plan made with one_pass=True (an attribute, not a field)."""
    model: torch.nn.Module
    rows: object
    attr: tuple
    labels: torch.Tensor
    idx: torch.Tensor
    pos: torch.Tensor
    buf: object
    batch_size: int
    one = None


class _OnePassValidMagPlan(ValidMagPlan):
    """A ValidMagPlan whose instances carry `one`."""


def valid_mag_plan(model, rows, attr_indptr, attr_indices, attr_data, idx_val, labels, batch_size=100, *, one_pass=False, fused=False):
    """The checks, the one position lookup (KeyError for a node that is no seed) and the buffers of `valid_mag`.

    one_pass=True: `valid_mag_pass` runs one eval `mag_prop_rows` over all positions, `model.infer` into the
    plan's [n, C] logits and one `eval_tail`; batch_size is a memory bound only (chunks of it go into row slices of the one
    logits buffer, the tail runs once).  Bit for bit the eager composition emb_rows -> infer -> eval_head -> eval_reduce,
    whatever batch_size; `infer`'s bits, NOT promised bit-equal to one_pass=False.  fused= is `infer`'s."""
    from .evaluate import _node_ids, _on_gpu, check_one_pass, eval_buffers, one_pass_buffers
    from .rows import RowMatrix
    if not isinstance(model, torch.nn.Module) or not hasattr(model, "emb_rows"):
        raise TypeError("valid_mag: model must be a MagMLP")
    if not isinstance(rows, RowMatrix):
        raise TypeError("rows must be a RowMatrix")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
        raise TypeError("labels must be an int64 CUDA tensor")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    _on_gpu("valid_mag", model.embeds.weight, labels=labels, attr_indptr=attr_indptr, col=rows.col)
    C = check_one_pass(model, one_pass, fused, "valid_mag")
    dev = rows.col.device
    idx = _node_ids(idx_val, "idx_val", dev)
    n = idx.numel()
    one = one_pass_buffers(n, C, dev, fused)
    pos = rows.batch_positions(idx, check=True) if n else None
    fields = (model, rows, (attr_indptr, attr_indices, attr_data), labels, idx, pos, eval_buffers(n, dev), batch_size)
    if one is None:
        return ValidMagPlan(*fields)
    plan = _OnePassValidMagPlan(*fields)
    plan.one = one
    return plan


def valid_mag_pass(plan, dropnode_rate=0.5, one_pass=None):
    """One validation pass over a ValidMagPlan: (loss, acc, counts) as device tensors.  Nothing synchronises.  one_pass: None
    reads it from the plan; False runs the batches over a one-pass plan too."""
    from .evaluate import _NoSync, _resolve_one_pass, eval_head, eval_reduce, one_pass_body
    model, rows, attr, labels, idx, pos, buf, batch_size = plan
    n = idx.numel()
    one_pass = _resolve_one_pass(plan, one_pass)
    with _NoSync(model):
        if one_pass:
            return one_pass_body(plan, lambda p: model.emb_rows(*attr, rows, batch_rows=p, dropnode_rate=dropnode_rate))
        for start in range(0, n, batch_size):
            end = min(start + batch_size, n)
            aug = model.emb_rows(*attr, rows, batch_rows=pos[start:end], dropnode_rate=dropnode_rate)
            eval_head(model(aug), labels, label_rows=idx[start:end], out=buf, offset=start)
        return eval_reduce(buf)


def predict_mag(graph, attr_indptr, attr_indices, attr_data, model, idx_test, labels, prop_mode, order, alpha=0.2,
                batch_size_logits=10000, return_preds=False, infer=False, fused=False):
    """MAG's `predict` (model_mag.py:192-245) on the GPU: the embedding of every node in eval mode
    (`embedding_bag_csr(nodes=None)`, model_mag.py:197-205), then `predict` on it.  A composition, no kernel of its own;
    the whole body is free of host synchronisation.  Same returns as `predict`."""
    from .embedding import embedding_bag_csr
    from .evaluate import _NoSync, _node_ids, predict
    if not isinstance(model, torch.nn.Module) or not hasattr(model, "embeds"):
        raise TypeError("predict_mag: model must be a MagMLP")
    _check(model.embeds.weight, torch.float32, "model.embeds.weight")
    idx_test = _node_ids(idx_test, "idx_test", model.embeds.weight.device)       # the upload of a host list comes first
    with _NoSync(model):
        emb = embedding_bag_csr(model.embeds.weight, attr_indptr, attr_indices, attr_data, nodes=None, training=False, validate=False)
        return predict(graph, emb, model, idx_test, labels, prop_mode, order, alpha, batch_size_logits, return_preds, infer, fused)
