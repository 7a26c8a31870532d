"""GRAND+'s evaluation on MI355X: `valid` and `predict` resident on the GPU, over the fused head of
csrc/evaluate.hip.

Reference `valid` (model.py:143-166), per mini-batch of `idx_val`: slice the scipy matrix, build and upload three
tensors, `random_prop`, the MLP, `log_softmax`; then `cat`, `nll_loss`, `accuracy` and two `.item()`.  Reference
`predict` (model.py:181-224): propagate in numpy, upload the features 10 000 rows at a time, copy every logit back,
`argmax` and the comparison with the labels on the host.

Here the row positions of all of `idx_val` are looked up once, every batch runs `random_prop_rows(training=False)`, the
model in eval mode and `eval_head` into one shared buffer, and one `eval_reduce` gives the two scalars; `predict` runs
`Graph.propagate_features`, the model over all N rows into one [N, C] device tensor, one `eval_head` with
`rows = label_rows = idx_test` and one `eval_reduce`.  Both return 0-dim device tensors: `.item()` is the caller's
choice, and after the position lookup nothing synchronises with the host (both run that part under
`torch.cuda.set_sync_debug_mode("error")`).  `local_logits` is the reference's `get_local_logits` on the device, over
`model.infer`; `predict(..., infer=True)` uses it.

Labels equal to `ignore_index` are left out of the loss as in `F.nll_loss`; other labels outside [0, C) and indices
outside their array are never used as an address: they are flagged, left out and counted.  The accuracy divides by the
number of rows, ignored ones included, as the reference's `accuracy` divides by `len(labels)`
(utils/data_loader.py:165).  There is no CPU fallback.

Opt-in: `eval_tail` is `eval_head` + `eval_reduce` as one launch with the same bits; `valid_plan(one_pass=True)`
validates in one gather, one `model.infer` and one tail; `ValidGraph` replays a pass and the tracker's update from one
captured graph.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import _native
from ._common import _ptr, _stream


class EvalBuffers(NamedTuple):
    """What `eval_head` fills and `eval_reduce` reads, one entry per evaluated row."""
    nll: torch.Tensor      # float32: -logp[y], 0 for a row that is ignored or bad
    pred: torch.Tensor     # int32: argmax of the row (-1: the row index was outside the logits)
    flag: torch.Tensor     # uint8: _native.GP_EVAL_WRONG / CORRECT / IGNORED / BAD


def eval_buffers(n, device):
    """Buffers for n evaluated rows on `device`."""
    return EvalBuffers(torch.empty(n, dtype=torch.float32, device=device), torch.empty(n, dtype=torch.int32, device=device),
                       torch.empty(n, dtype=torch.uint8, device=device))


def _index(t, name):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
        raise TypeError(f"{name} must be an int64 CUDA tensor")
    return t.reshape(-1).contiguous()


def _check_buffers(out):
    """dtype, layout and common length of (nll, pred, flag); returns the length.  The device is checked by _on_gpu."""
    if not isinstance(out, tuple) or len(out) != 3:
        raise TypeError("out must be the (nll, pred, flag) buffers of eval_buffers()")
    for t, dtype, name in zip(out, (torch.float32, torch.int32, torch.uint8), ("nll", "pred", "flag")):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
            raise TypeError(f"out.{name} must be a contiguous 1-d {dtype} tensor")
    if not out[0].numel() == out[1].numel() == out[2].numel():
        raise ValueError("out.nll, out.pred and out.flag must have the same length")
    return out[0].numel()


def _on_gpu(what, first, **tensors):
    """Every tensor of a call on one GPU, checked last: dtype, shape and size errors are told apart from a CPU tensor."""
    if not first.is_cuda:
        raise TypeError(f"{what} runs on the GPU only: its tensors must be CUDA tensors (no CPU fallback)")
    for name, t in tensors.items():
        if t is not None and t.device != first.device:
            raise TypeError(f"{name} must be on {first.device}, got {t.device} (no CPU fallback)")


def eval_head(logits, labels, *, rows=None, label_rows=None, ignore_index=-100, out=None, offset=0):
    """nll, argmax and a flag for n rows of logits, written at out[offset : offset + n]; returns `out` (EvalBuffers).

    logits: float32 CUDA [R, C], 1 <= C <= 4096.  Evaluated row i reads logits[rows[i]] (rows None: logits[i]) and the
    label labels[label_rows[i]] (label_rows None: labels[i]); labels, rows and label_rows are int64 CUDA tensors.  n is
    the length of rows, else of label_rows, else R.  out None allocates buffers of offset + n rows; successive calls with
    the same `out` and rising offsets fill one buffer for `eval_reduce`.  One launch, no host synchronisation."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a float32 [R, C] CUDA tensor")
    R, C = logits.shape
    if not 1 <= C <= _native.GP_MAX_CLASSES:
        raise ValueError(f"the number of classes must be in [1, {_native.GP_MAX_CLASSES}], got {C}")
    labels = _index(labels, "labels")
    if labels is None:
        raise TypeError("labels must be an int64 CUDA tensor")
    rows = _index(rows, "rows")
    label_rows = _index(label_rows, "label_rows")
    if rows is not None and label_rows is not None and rows.numel() != label_rows.numel():
        raise ValueError(f"rows has {rows.numel()} entries, label_rows {label_rows.numel()}")
    n = rows.numel() if rows is not None else label_rows.numel() if label_rows is not None else R
    if rows is None and n > R:
        raise ValueError(f"label_rows has {n} entries, logits {R} rows (pass rows to pick them)")
    if label_rows is None and n > labels.numel():
        raise ValueError(f"labels has {labels.numel()} entries for {n} rows (pass label_rows to pick them)")
    offset = int(offset)
    if offset < 0:
        raise ValueError(f"offset must be >= 0, got {offset}")
    if out is not None:
        cap = _check_buffers(out)
        if offset + n > cap:
            raise ValueError(f"offset + n = {offset + n} rows do not fit the out buffers of {cap}")
        _on_gpu("eval_head", logits, labels=labels, rows=rows, label_rows=label_rows, nll=out[0], pred=out[1], flag=out[2])
    else:
        _on_gpu("eval_head", logits, labels=labels, rows=rows, label_rows=label_rows)
        out, cap = eval_buffers(offset + n, logits.device), offset + n
    z = logits.contiguous()
    rc = _native.lib().gp_eval_head(z.device.index, z.data_ptr(), R, C, _ptr(rows), labels.data_ptr(), labels.numel(),
                                    _ptr(label_rows), n, int(ignore_index), offset, cap, out[0].data_ptr(), out[1].data_ptr(),
                                    out[2].data_ptr(), _stream(z))
    _native.raise_for_status(rc)
    return EvalBuffers(*out)


def eval_reduce(buffers):
    """(loss, acc, counts) of filled EvalBuffers: loss = sum(nll) / n_valid and acc = n_correct / n_rows as 0-dim float32
    device tensors, counts int64 [4] = n_valid, n_correct, n_ignored, n_bad.  No valid row gives a NaN loss.  Two
    launches, no host synchronisation; bitwise the same however the buffers were filled."""
    n = _check_buffers(buffers)
    nll, _pred, flag = buffers
    _on_gpu("eval_reduce", nll, pred=_pred, flag=flag)
    out = torch.empty(2, dtype=torch.float32, device=nll.device)
    counts = torch.empty(4, dtype=torch.int64, device=nll.device)
    ws = torch.empty(_native.eval_workspace_bytes(), dtype=torch.uint8, device=nll.device)
    rc = _native.lib().gp_eval_reduce(nll.device.index, nll.data_ptr(), flag.data_ptr(), n, ws.data_ptr(), out.data_ptr(),
                                      counts.data_ptr(), _stream(nll))
    _native.raise_for_status(rc)
    return out[0], out[1], counts


def eval_tail_workspace(device):
    """The workspace of `eval_tail` on `device`: the ticket counter, zeroed here once; every call leaves it zero."""
    return torch.zeros(_native.EVAL_TAIL_WORKSPACE_BYTES, dtype=torch.uint8, device=device)


def eval_tail(logits, labels, *, rows=None, label_rows=None, ignore_index=-100, out=None, workspace=None, result=None):
    """`eval_head` over all n rows at offset 0 and `eval_reduce` over them as ONE launch (gp_eval_tail): returns
    (loss, acc, counts, EvalBuffers), every one bit for bit what the two calls give.

    The arguments and host checks are `eval_head`'s (no offset: the buffers are filled from 0, `out` may be longer than n
    and only its first n rows are written and reduced).  workspace: the uint8 tensor of `eval_tail_workspace(device)`, kept
    by the caller between calls on one stream; None allocates and zeroes one.  result: None, or (out2, counts) -- a float32
    [2] and an int64 [4] tensor on the device that the call writes (a plan's static tensors); loss and acc are views of
    out2.  Above _native.EVAL_TAIL_MAX_ROWS rows the two calls run instead (three launches, the same bits).  No host
    synchronisation."""
    if not isinstance(logits, torch.Tensor) or logits.dtype != torch.float32 or logits.dim() != 2:
        raise TypeError("logits must be a float32 [R, C] CUDA tensor")
    R, C = logits.shape
    if not 1 <= C <= _native.GP_MAX_CLASSES:
        raise ValueError(f"the number of classes must be in [1, {_native.GP_MAX_CLASSES}], got {C}")
    labels = _index(labels, "labels")
    if labels is None:
        raise TypeError("labels must be an int64 CUDA tensor")
    rows = _index(rows, "rows")
    label_rows = _index(label_rows, "label_rows")
    if rows is not None and label_rows is not None and rows.numel() != label_rows.numel():
        raise ValueError(f"rows has {rows.numel()} entries, label_rows {label_rows.numel()}")
    n = rows.numel() if rows is not None else label_rows.numel() if label_rows is not None else R
    if rows is None and n > R:
        raise ValueError(f"label_rows has {n} entries, logits {R} rows (pass rows to pick them)")
    if label_rows is None and n > labels.numel():
        raise ValueError(f"labels has {labels.numel()} entries for {n} rows (pass label_rows to pick them)")
    if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or
                                  not workspace.is_contiguous() or workspace.numel() < _native.EVAL_TAIL_WORKSPACE_BYTES):
        raise TypeError(f"workspace must be a contiguous uint8 tensor of at least {_native.EVAL_TAIL_WORKSPACE_BYTES} bytes "
                        "(eval_tail_workspace)")
    if result is not None:
        if not isinstance(result, tuple) or len(result) != 2:
            raise TypeError("result must be (out2, counts): a float32 [2] and an int64 [4] tensor")
        for t, dtype, k, name in zip(result, (torch.float32, torch.int64), (2, 4), ("out2", "counts")):
            if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.shape != (k,) or not t.is_contiguous():
                raise TypeError(f"result.{name} must be a contiguous {dtype} tensor of {k} elements")
    extra = dict(workspace=workspace, out2=result[0] if result else None, counts=result[1] if result else None)
    if out is not None:
        cap = _check_buffers(out)
        if n > cap:
            raise ValueError(f"n = {n} rows do not fit the out buffers of {cap}")
        _on_gpu("eval_tail", logits, labels=labels, rows=rows, label_rows=label_rows, nll=out[0], pred=out[1], flag=out[2], **extra)
    else:
        _on_gpu("eval_tail", logits, labels=labels, rows=rows, label_rows=label_rows, **extra)
        out = eval_buffers(n, logits.device)
    out = EvalBuffers(*out)
    if n > _native.EVAL_TAIL_MAX_ROWS:                    # one workgroup would walk too many slices: the unfused pair
        eval_head(logits, labels, rows=rows, label_rows=label_rows, ignore_index=ignore_index, out=out)
        used = out if out[0].numel() == n else EvalBuffers(out[0][:n], out[1][:n], out[2][:n])
        loss, acc, counts = eval_reduce(used)
        if result is not None:
            result[0][0].copy_(loss)
            result[0][1].copy_(acc)
            result[1].copy_(counts)
            loss, acc, counts = result[0][0], result[0][1], result[1]
        return loss, acc, counts, out
    if workspace is None:
        workspace = eval_tail_workspace(logits.device)
    out2, counts = result if result is not None else (torch.empty(2, dtype=torch.float32, device=logits.device),
                                                      torch.empty(4, dtype=torch.int64, device=logits.device))
    z = logits.contiguous()
    rc = _native.lib().gp_eval_tail(z.device.index, z.data_ptr(), R, C, _ptr(rows), labels.data_ptr(), labels.numel(), _ptr(label_rows),
                                    n, int(ignore_index), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                    workspace.data_ptr(), out2.data_ptr(), counts.data_ptr(), _stream(z))
    _native.raise_for_status(rc)
    return out2[0], out2[1], counts, out


def _node_ids(idx, name, device):
    """A list of node ids (tensor or anything numpy converts) as an int64 tensor on `device`."""
    if isinstance(idx, torch.Tensor):
        if idx.dtype != torch.int64:
            raise TypeError(f"{name} must hold int64 node ids, got {idx.dtype}")
        t = idx
    else:
        a = np.asarray(idx)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"{name} must hold integer node ids, got {a.dtype}")
        t = torch.from_numpy(np.ascontiguousarray(a.reshape(-1), dtype=np.int64))
    return t.reshape(-1).to(device).contiguous()


def _check_common(model, features, labels, what):
    if not isinstance(model, torch.nn.Module):
        raise TypeError(f"{what}: model must be a GrandPlusMLP or MagMLP")
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or not features.is_contiguous():
        raise TypeError("features must be a contiguous float32 [N, F] CUDA tensor")
    if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64:
        raise TypeError("labels must be an int64 CUDA tensor")
    _on_gpu(what, features, labels=labels)


class _NoSync:
    """The body of valid / predict: no gradient, the model in eval mode, host synchronisation an error."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.training = self.model.training
        self.mode = torch.cuda.get_sync_debug_mode()
        self.grad = torch.is_grad_enabled()
        self.model.eval()
        torch.set_grad_enabled(False)
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode(self.mode)
        torch.set_grad_enabled(self.grad)
        self.model.train(self.training)
        return False


def valid(model, rows, features, idx_val, labels, batch_size=10000, dropnode_rate=0.5, return_counts=False, one_pass=False,
          fused=False):
    """The reference's `valid` (model.py:143-166) on the GPU: (loss, acc) as 0-dim float32 device tensors.

    rows: the RowMatrix that holds `topk_adj`; features float32 CUDA [N, F]; idx_val: the validation node ids (every one
    a seed of `rows`); labels int64 CUDA [N], indexed by node id as `labels[idx]` is.  The positions of idx_val in `rows`
    are looked up once (one check, KeyError for a node that is no seed); from there on nothing synchronises.  The
    model's training flag is restored on exit.  return_counts adds the int64 [4] device tensor n_valid, n_correct,
    n_ignored, n_bad (labels outside [0, C) are counted there, not raised).

    model: a GrandPlusMLP, or a MagMLP with `features` = the [N, H] embedding the caller computed in eval mode
    (`model.emb_csr(...)` over all nodes): the MLP is then applied to the propagated embedding, as model_mag.py does.

    one_pass=True: one gather over the whole set, `model.infer` (fused= is its) and one `eval_tail`, see
    `valid_plan`."""
    loss, acc, counts = valid_pass(valid_plan(model, rows, features, idx_val, labels, batch_size, one_pass=one_pass, fused=fused),
                                   dropnode_rate)
    return (loss, acc, counts) if return_counts else (loss, acc)


class OnePass(NamedTuple):
    """What a one-pass plan owns beside the evaluation buffers, allocated once."""
    logits: torch.Tensor       # float32 [n, C]: `infer` writes its chunks into row slices of it
    out2: torch.Tensor         # float32 [2]: loss, acc
    counts: torch.Tensor       # int64 [4]
    workspace: torch.Tensor    # eval_tail's ticket counter
    fused: bool                # `infer`'s fused=


class ValidPlan(NamedTuple):
    """What `valid` prepares once for a validation set: its arguments as checked, the node ids on the device, their
    positions in `rows` and the evaluation buffers.  `valid_pass` runs over it any number of times (the fit loop).
    `one` is None, or the OnePass of a plan made with one_pass=True (an attribute, not a field: the tuple stays what it was)."""
    model: torch.nn.Module
    rows: object
    features: torch.Tensor
    labels: torch.Tensor
    idx: torch.Tensor
    pos: torch.Tensor
    buf: EvalBuffers
    batch_size: int
    one = None


class _OnePassValidPlan(ValidPlan):
    """A ValidPlan whose instances carry `one` (a subclass of a NamedTuple has a __dict__)."""


def n_classes_of(model):
    """The width of the model's logits: the last layer's, or the embedding's for a MagMLP that is its embedding alone."""
    layers = model._layers()
    return int(layers[-1][0].weight.shape[0] if layers else model.embeds.weight.shape[1])


def check_one_pass(model, one_pass, fused, what):
    """The refusals of one_pass= / fused=, before any device call: the number of classes of a one-pass plan, else None."""
    if not isinstance(one_pass, bool) or not isinstance(fused, bool):
        raise TypeError(f"{what}: one_pass and fused must be bools")
    if not one_pass:
        if fused:
            raise ValueError(f"{what}: fused=True needs one_pass=True (the fused kernel is an inference path)")
        return None
    if not hasattr(model, "infer") or not hasattr(model, "_layers"):
        raise TypeError(f"{what}: one_pass=True needs a GrandPlusMLP or MagMLP (it runs model.infer)")
    C = n_classes_of(model)
    if not 1 <= C <= _native.GP_MAX_CLASSES:
        raise ValueError(f"the number of classes must be in [1, {_native.GP_MAX_CLASSES}], got {C}")
    return C


def one_pass_buffers(n, C, device, fused):
    """The OnePass of n rows of C classes, or None for C None."""
    if C is None:
        return None
    return OnePass(torch.empty((n, C), dtype=torch.float32, device=device), torch.empty(2, dtype=torch.float32, device=device),
                   torch.empty(4, dtype=torch.int64, device=device), eval_tail_workspace(device), fused)


def valid_plan(model, rows, features, idx_val, labels, batch_size=10000, *, one_pass=False, fused=False):
    """The checks, the one position lookup (KeyError for a node that is no seed) and the buffers of `valid`.

    one_pass=True: `valid_pass` then runs one `random_prop_rows(training=False)` over all positions, one
    `model.infer` into the plan's [n, C] logits and one `eval_tail`; batch_size is a memory bound only -- for n above it the
    gather and `infer` go chunk by chunk into row slices of the one logits buffer, and the tail still runs once (above
    _native.EVAL_TAIL_MAX_ROWS rows: `eval_head` + `eval_reduce`).  The result is bit for bit the eager composition
    random_prop_rows -> infer -> eval_head -> eval_reduce and does not depend on batch_size.  The rows get `infer`'s bits,
    not the block path's (the trade of `predict(..., infer=True)`): it is NOT promised bit-equal to one_pass=False.
    fused=True is `infer`'s (the same bits) and needs one_pass=True."""
    from .rows import RowMatrix
    if not isinstance(rows, RowMatrix):
        raise TypeError("rows must be a RowMatrix")
    _check_common(model, features, labels, "valid")
    if features.shape[0] != rows.n_nodes or features.device != rows.col.device:
        raise ValueError(f"features must have one row per node ({rows.n_nodes}) on the device of rows ({rows.col.device})")
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be >= 1, got {batch_size}")
    dev = features.device
    C = check_one_pass(model, one_pass, fused, "valid")
    idx = _node_ids(idx_val, "idx_val", dev)
    n = idx.numel()
    one = one_pass_buffers(n, C, dev, fused)
    pos = rows.batch_positions(idx, check=True) if n else None
    fields = (model, rows, features, labels, idx, pos, eval_buffers(n, dev), batch_size)
    if one is None:
        return ValidPlan(*fields)
    plan = _OnePassValidPlan(*fields)
    plan.one = one
    return plan


def one_pass_body(plan, gather):
    """The one-pass validation over a plan with `one` set (inside _NoSync): gather(pos) gives the augmented rows of a chunk."""
    model, labels, idx, pos, buf, batch_size, one = plan.model, plan.labels, plan.idx, plan.pos, plan.buf, plan.batch_size, plan.one
    n = idx.numel()
    for start in range(0, n, batch_size):
        end = min(start + batch_size, n)
        model.infer(gather(pos if end - start == n else pos[start:end]), out=one.logits[start:end], fused=one.fused)
    loss, acc, counts, _ = eval_tail(one.logits, labels, label_rows=idx, out=buf, workspace=one.workspace, result=(one.out2, one.counts))
    return loss, acc, counts


def _resolve_one_pass(plan, one_pass):
    if one_pass is None:
        return plan.one is not None
    if not isinstance(one_pass, bool):
        raise TypeError("one_pass must be None (the plan's) or a bool")
    if one_pass and plan.one is None:
        raise ValueError("one_pass=True needs a plan made with one_pass=True (it owns the logits and the tail's workspace)")
    return one_pass


def valid_pass(plan, dropnode_rate=0.5, one_pass=None):
    """One validation pass over a ValidPlan: (loss, acc, counts) as device tensors.  Nothing synchronises.  one_pass: None
    reads it from the plan; False runs the batches over a one-pass plan too."""
    from .augment import random_prop_rows
    model, rows, features, labels, idx, pos, buf, batch_size = plan
    one_pass = _resolve_one_pass(plan, one_pass)
    with _NoSync(model):
        if one_pass:
            return one_pass_body(plan, lambda p: random_prop_rows(features, rows.col, rows.val, rows.filled, rows.K, batch_rows=p,
                                                                  dropnode_rate=dropnode_rate, training=False))
        for start in range(0, idx.numel(), batch_size):
            end = min(start + batch_size, idx.numel())
            aug = random_prop_rows(features, rows.col, rows.val, rows.filled, rows.K, batch_rows=pos[start:end],
                                   dropnode_rate=dropnode_rate, training=False)
            eval_head(model(aug), labels, label_rows=idx[start:end], out=buf, offset=start)
        return eval_reduce(buf)


class ValidGraph:
    """A validation pass and the tracker's update as one replayed graph.

    plan: a ValidPlan or a mag.ValidMagPlan, one_pass or batched; tracker: None, or the fit.BestTracker that takes the
    pass's loss and accuracy at `state`'s tick (state: the StepState; a tracker without one is a ValueError).  The first
    `run()` executes the body eagerly (it loads code), the second captures it with torch.cuda.graph, every later one is one
    replay; each returns (loss, acc, counts), from the capture on the static tensors of the graph.  With a row_grad tracker
    gp_fit_rows_snapshot is part of the graph.  The body is one stream, a linear chain of launches.  `before` (an attribute,
    None by default) is a callable whose launches run in front of the pass and are captured with it: `fit` sets it to
    `MagTrainStep.flush_table` for a deferred table.

    A replay reads the weights, the BatchNorm running statistics, the step state and the tracker's struct through the
    pointers of the capture: every tensor of model.state_dict() has to stay where it is, which run() checks (RuntimeError
    for a tensor that moved).  The model's training flag, the grad mode and the sync-debug mode are as the pass leaves
    them (_NoSync) on every path.  A capture that raises is re-raised with the name of the call that broke it."""

    def __init__(self, plan, dropnode_rate=0.5, tracker=None, state=None):
        if not isinstance(plan, tuple) or not hasattr(plan, "one") or not hasattr(plan, "model"):
            raise TypeError("ValidGraph takes a ValidPlan (valid_plan) or a ValidMagPlan (mag.valid_mag_plan)")
        # None, or a callable whose launches belong in front of the pass and are captured with it; to be set before the second
        # run().  `fit` sets MagTrainStep.flush_table for a deferred table
        self.before = None
        if not 0.0 <= float(dropnode_rate) <= 1.0:
            raise ValueError(f"dropnode_rate must be in [0, 1], got {dropnode_rate}")
        if tracker is not None:
            if not hasattr(tracker, "update") or not hasattr(tracker, "buf"):
                raise TypeError("tracker must be a fit.BestTracker")
            if state is None or not hasattr(state, "buf"):
                raise ValueError("a tracker needs the StepState whose tick its update reads: pass state=")
        self.plan, self.dropnode_rate, self.tracker, self.state = plan, float(dropnode_rate), tracker, state
        if isinstance(plan, ValidPlan):
            self._pass = valid_pass
        else:
            from .mag import valid_mag_pass
            self._pass = valid_mag_pass
        self.runs = 0
        self._graph = self._result = self._ptrs = self._where = None

    def _body(self):
        if self.before is not None:
            self._where = "before"
            self.before()
        self._where = "valid_pass"
        result = self._pass(self.plan, self.dropnode_rate)
        if self.tracker is not None:
            self._where = "tracker.update"
            self.tracker.update(result[0], result[1], self.state)
        self._where = None
        return result

    def _pointers(self):
        return [(name, t.data_ptr()) for name, t in self.plan.model.state_dict().items()]

    def run(self):
        self.runs += 1
        if self.runs == 1:                                               # a real, eager pass
            return self._body()
        if self._graph is None:
            ptrs = self._pointers()
            graph = torch.cuda.CUDAGraph()
            try:
                with torch.cuda.graph(graph):                            # one side stream; nothing runs until the replay
                    result = self._body()
            except Exception as e:
                where, self._where = self._where, None
                self.runs -= 1
                raise RuntimeError(f"capturing the validation pass broke in {where}: {e}") from e
            self._graph, self._result, self._ptrs = graph, tuple(result), ptrs
        else:
            for (name, was), (_name, now) in zip(self._ptrs, self._pointers()):
                if was != now:
                    raise RuntimeError(f"{name} moved since the validation pass was captured: the graph reads the model's tensors "
                                       "through the pointers of the capture (change them in place)")
        self._graph.replay()
        return self._result


def local_logits(model, attr_mat, batch_size=10000, out=None, fused=False):
    """The reference's `get_local_logits` (model.py:169-178) with the logits staying on the device: the model in eval
    semantics over every row of attr_mat (float32 CUDA [N, F], contiguous), batch_size rows at a time, as one [N, C]
    device tensor (`out`, if given).  A thin wrapper over `model.infer`: the module's training flag is not
    touched, nothing synchronises, and the rows get the same bits whatever the batch size.  fused=True is `infer`'s: the
    last two blocks as one kernel, the same bits."""
    if not isinstance(model, torch.nn.Module) or not hasattr(model, "infer"):
        raise TypeError("local_logits: model must be a GrandPlusMLP or MagMLP")
    return model.infer(attr_mat, out=out, batch_size=batch_size, fused=fused)


def predict(graph, features, model, idx_test, labels, prop_mode, order, alpha=0.2, batch_size_logits=10000, return_preds=False,
            infer=False, fused=False):
    """The reference's `predict` (model.py:181-224) on the GPU: the test accuracy as a 0-dim float32 device tensor, and
    with return_preds also the int32 [len(idx_test)] predictions.

    graph: the Graph of adj + I; features float32 CUDA [N, F]; model: the MLP (`model.mlp` of the reference); idx_test:
    node ids (any order, duplicates allowed); labels int64 CUDA [N].  `Graph.propagate_features`, then the model in eval
    mode over all N rows, batch_size_logits at a time, into one [N, C] device tensor; one head call gathers
    logits[idx_test] and labels[idx_test].  No logit reaches the host.  An id outside [0, N) is counted as a bad row
    (prediction -1), never read.  infer=True runs the model through `local_logits` (the inference GEMM of DESIGN §7j,
    each batch written straight into the [N, C] tensor) in place of the batch loop over the training kernels; with it,
    fused=True runs the model's last two blocks as one kernel (the same bits); fused=True alone is refused."""
    if fused and not infer:
        raise ValueError("predict: fused=True needs infer=True (the fused kernel is an inference path)")
    _check_common(model, features, labels, "predict")
    batch_size_logits = int(batch_size_logits)
    if batch_size_logits < 1:
        raise ValueError(f"batch_size_logits must be >= 1, got {batch_size_logits}")
    dev = features.device
    idx = _node_ids(idx_test, "idx_test", dev)
    N = features.shape[0]
    with _NoSync(model):
        prop = graph.propagate_features(features, prop_mode, order, alpha)
        if infer:
            logits = local_logits(model, prop, batch_size_logits, fused=fused)
        elif N <= batch_size_logits:
            logits = model(prop)
        else:
            logits = None
            for start in range(0, N, batch_size_logits):
                z = model(prop[start:start + batch_size_logits])
                if logits is None:
                    logits = torch.empty((N, z.shape[1]), dtype=torch.float32, device=dev)
                logits[start:start + z.shape[0]].copy_(z)
        buf = eval_head(logits, labels, rows=idx, label_rows=idx)
        _, acc, _ = eval_reduce(buf)
    return (acc, buf.pred) if return_preds else acc
