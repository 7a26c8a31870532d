"""MAG's training step over device-resident step state, replayable from a captured graph.

`MagTrainStep` is `step.TrainStep` with the front end swapped: where that runs `random_prop_rows` over dense features,
this runs `MagMLP.emb_rows` (`mag_prop_rows`, §7k) over the node-attribute CSR and trains the embedding table with the
layers.  The advance, the batch gather, `gp_step_masks` (the DropNode mask is `random_prop_rows`'s layout, which
`mag_prop_rows` takes), the S-sample MLP, the loss, `ClipAdam(capturable=True)`, `step`, `step_sampled`, the graph per batch
shape, `MAX_GRAPHS` and the wrapping of a broken capture are inherited.

The table gradient has two modes.  `deterministic=False`: the atomic backward, one launch, not reproducible -- the fast
mode.  `deterministic=True` (None follows torch's flag): the sort-then-gather backward of mag_det.py, which never asks the
host for a number, so the whole step is captured and a replay is bitwise the eager step.  Its key buffer holds
`max_entries` entries per batch row and slot: None means K * Lmax per batch row, Lmax the longest bag among the nodes that
occur as columns of `rows` (read once here, the constructor's one host read), and then the buffer cannot overflow.

`table_step="exact"` or `"lazy"` (deterministic mode, or the atomic mode with `row_list="bitmap"`, §7u) steps
the embedding table from the backward's row list instead of a dense gradient: no `torch.zeros` of [V, H] per step, no dense read of dW.  "exact" is bit for bit today's
step.  "lazy" updates the touched rows alone and is NOT the reference's dense Adam (model_mag.py:312), under which an
untouched row still moves while its moments decay.  "deferred"  is "exact"'s trajectory with "lazy"'s traffic: the
untouched rows' updates are replayed when a row is next read and by `flush_table()`; between flushes the table shows lagging rows.

`fit.fit` takes a MagTrainStep as it takes a TrainStep: `_valid_plan` / `_valid_pass` are `mag.valid_mag_plan` /
`valid_mag_pass` over the step's attribute CSR and rows.  `dirty_rows=True` (with `table_step="lazy"`) has every backward mark
the rows it hands over in a bitmap, from which the loop's BestTracker copies only the rows that changed since its last snapshot.

`input_dropout=True` takes a model with `input_droprate > 0`: the front end reads the step state's seed from
device memory, so every replay draws a fresh input-dropout mask, and the deterministic table gradient keeps the samples apart
(mag_drop.py).

Left out: an explicit input-dropout mask, several steps in one graph, the validation pass as a captured graph.
"""
from __future__ import annotations

import torch

from . import _native
from ._common import _deterministic
from .step import TrainStep, trained_parameters

__all__ = ["MagTrainStep", "mag_trained_parameters"]


_SEED_WORD = _native.GpStepState.seed.offset // 8      # gp_step_state.seed, as an index into StepState.buf (int64 words)


def mag_trained_parameters(model):
    """The parameters of a MagMLP that a training step gives a gradient: the embedding table, then what
    `trained_parameters` lists for the layers."""
    return [model.embeds.weight] + trained_parameters(model)


def _csr(t, dtype, name):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-D tensor of dtype {dtype}")


class MagTrainStep(TrainStep):
    """One MAG training step (model_mag.py's loop body) as one replayable object.

    model: a MagMLP in train mode, with input_droprate = 0 unless input_dropout=True; optimizer: a
    ClipAdam(capturable=True, state=StepState(device)) over `mag_trained_parameters(model)`; rows: the RowMatrix; attr_indptr int64 [N + 1], attr_indices int32 [nnz],
    attr_data float32 [nnz]: the node-attribute CSR on the GPU; labels, idx_train, idx_unlabel and the keywords up to
    `capture` as for TrainStep.  nlayers = 1 (no `fcs`: the embedding is the logits) is accepted.

    deterministic: None follows torch.are_deterministic_algorithms_enabled(), resolved here once.  True: the table gradient is
    mag_det's (bitwise the same run to run, eager or replayed); False: fp32 atomics.
    max_entries: the capacity of the deterministic backward's key buffer for the WHOLE batch; None: B * K * Lmax per batch
    shape, which cannot overflow.  A tighter value may: the step then runs on with a gradient that lacks the entries past
    it and sets a flag, which `check_entries_flag()` reads.

    table_step: None is the dense table gradient and the dense clip + Adam pass over it.  "exact" / "lazy" need the
    deterministic mode (ValueError otherwise): one optim_rows.RowGrad, shared by every graph of the step, receives the
    backward's rows and `optimizer.set_row_grad(weight, row_grad, table_step)` steps the table from them; `weight.grad` stays
    None.  "exact": every parameter, Adam tensor and loss is bit for bit what None gives (with clipping on, up to the
    rounding of the norm, whose partial sums are cut differently).  "lazy": only the touched rows of the table and of its
    moments change -- NOT the reference's trajectory (dense Adam moves an untouched row while its moments decay); the table's
    group must have weight_decay = 0.
    row_list: None, or "bitmap"  for a `table_step` over the ATOMIC backward: it needs a table_step and a mode
    that resolves to non-deterministic (ValueError otherwise).  One optim_rows.BitmapRowGrad, shared by every graph, lists
    the rows each batch's bags name (a bitmap of V bits, compacted without a sort) in min(V, max_entries) keys; with
    max_entries=None that cannot overflow.  The table gradient is then as reproducible as the atomic backward is -- the row
    list itself is the same run to run -- and with "exact" the step is the dense atomic step up to the order of the atomics.
    dirty_rows: True needs table_step="lazy" (ValueError otherwise, before any device call: under None or "exact" every row of
    the table moves in every step, so there is nothing to skip).  The step's RowGrad then tracks the rows every backward
    hands over (`RowGrad.track_dirty()`, made here, before any capture: the mark is part of every graph of the step), and
    `fit` snapshots the table row by row (`fit.BestTracker(row_grad=)`).
    table_step="deferred" (DESIGN §7za), with either backward: the trajectory of "exact", bit for bit with the deterministic
    backward, at the memory traffic of "lazy"; weight decay is allowed.  The zero-gradient update dense Adam gives an
    untouched row at every step is put off: before the forward the step lists the rows the batch's bags name (the bitmap
    kernels of §7u, min(V, max_entries) keys, the same overflow bit) and replays on them the steps they missed, in order,
    through the dense step's own element update; `flush_table()` does so for every row.  defer_capacity: the steps of
    history kept, a power of two in [4, 65536] (None: 1024; a ValueError with any other table_step); the step flushes by
    itself before a row could lag further.  BETWEEN FLUSHES `model.embeds.weight` AND ITS MOMENTS SHOW LAGGING ROWS: call
    `flush_table()` before reading them (`fit`, `_valid_pass` and `optimizer.state_dict()` do).  dirty_rows=True is refused
    as for "exact": every row moves.
    segment_chunk: None, or C (a power of two in [64, 4096]): the deterministic table gradient sums every
    attribute's segment in chunks of C entries, so that an attribute that sits in many bags of a batch is no longer one
    serial chain.  It needs the deterministic mode (ValueError otherwise) and goes with every table_step, dirty_rows and fit.

    input_dropout: True accepts a model with input_droprate > 0, in every mode above.  The front end is handed the
    address of the step state's seed, which `gp_step_advance` rewrites at every step: the input-dropout mask of step t is
    `mag_prop_rows`' for seed = step_seed(base, t), eager or replayed.  The deterministic table gradient then runs
    `gp_mag_prop_rows_backward_det_drop`, whose scratch is S times as large and, like every buffer of the step, sized from the
    batch shape before the capture.  With a model at input_droprate = 0 the step is bit for bit the step without the keyword.

    With capture=True and the deterministic mode the capture includes `torch.sort`; should a torch build refuse to capture it,
    the capture fails as every broken capture does here: a RuntimeError naming the call (backward), no retry, no fallback."""

    def __init__(self, model, optimizer, rows, attr_indptr, attr_indices, attr_data, labels, idx_train, idx_unlabel, *, samples,
                 dropnode_rate, lam, warmup, tem, conf=None, kind="l2", seed, capture=True, deterministic=None, max_entries=None, table_step=None,
                 row_list=None, dirty_rows=False, segment_chunk=None, input_dropout=False, defer_capacity=None):
        from .mlp import MagMLP
        if not isinstance(model, MagMLP):
            raise ValueError("MagTrainStep takes a MagMLP (a GrandPlusMLP goes to step.TrainStep)")
        if not isinstance(input_dropout, bool):
            raise TypeError(f"input_dropout must be True or False, got {input_dropout!r}")
        if float(model.input_droprate) != 0.0 and not input_dropout:
            raise ValueError("MagTrainStep needs model.input_droprate = 0: input dropout in the step is left out (DESIGN §9) unless "
                             f"input_dropout=True is passed (DESIGN §7y), got {model.input_droprate}")
        self.input_dropout = input_dropout and float(model.input_droprate) > 0.0
        self._check_optimizer_and_rows(optimizer, rows)
        _csr(attr_indptr, torch.int64, "attr_indptr")
        _csr(attr_indices, torch.int32, "attr_indices")
        _csr(attr_data, torch.float32, "attr_data")
        if attr_indptr.numel() != rows.n_nodes + 1 or attr_data.numel() != attr_indices.numel():
            raise ValueError(f"attr_indptr needs one entry per node ({rows.n_nodes}) plus one; attr_indices and attr_data the same length")
        self._check_hyperparameters(model, optimizer, samples, dropnode_rate, kind, tem)
        self.deterministic = _deterministic(deterministic)
        if max_entries is not None:
            from .mag_det import check_max_entries
            check_max_entries(max_entries)
        from .gather_chunk import resolve
        self.segment_chunk = resolve(segment_chunk, self.deterministic, "MagTrainStep")
        if row_list not in (None, "bitmap"):
            raise ValueError(f"row_list must be None or 'bitmap', got {row_list!r}")
        if table_step is not None:
            from .optim_rows import check_mode
            check_mode(table_step)
            if row_list == "bitmap":
                if self.deterministic:
                    raise ValueError("row_list='bitmap' is the atomic backward's row list: it needs deterministic=False (the "
                                     "deterministic backward holds a key list of its own)")
            elif not self.deterministic:
                raise ValueError(f"table_step={table_step!r} needs the deterministic table gradient: deterministic=True (the atomic "
                                 "backward keeps no list of the rows it touched, DESIGN §9)")
        elif row_list == "bitmap":
            raise ValueError("row_list='bitmap' needs a table_step ('exact' or 'lazy'): without one the table takes a dense gradient")
        if dirty_rows and table_step != "lazy":
            raise ValueError(f"dirty_rows=True needs table_step='lazy', got table_step={table_step!r}: under None or 'exact' every "
                             "row of the table moves in every step, so a snapshot has no row to skip")
        if table_step == "deferred":
            from .optim_rows import check_capacity
            defer_capacity = check_capacity(defer_capacity)
        elif defer_capacity is not None:
            raise ValueError(f"defer_capacity belongs to table_step='deferred', got table_step={table_step!r}")
        if not attr_indptr.is_cuda:
            raise ValueError("the step runs on the GPU only: the attribute CSR must be CUDA tensors (no CPU fallback)")
        dev = attr_indptr.device
        for name, t in (("attr_indices", attr_indices), ("attr_data", attr_data), ("rows.col", rows.col),
                        ("model.embeds.weight", model.embeds.weight)):
            if t.device != dev:
                raise ValueError(f"{name} must be on the device of attr_indptr ({dev}), got {t.device}")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.device != dev:
            raise ValueError("labels must be an int64 tensor on the device of the attribute CSR")
        self.attr = (attr_indptr, attr_indices, attr_data)
        self.max_entries = max_entries
        self._setup(model, optimizer, rows, labels, idx_train, idx_unlabel, dev, samples=samples, dropnode_rate=dropnode_rate,
                    lam=lam, warmup=warmup, tem=tem, conf=conf, kind=kind, seed=seed, capture=capture)
        self._entries_flag = torch.zeros(1, dtype=torch.int32, device=dev)   # bit 0: a backward had more entries than its buffer
        self.table_step, self.row_list, self.row_grad = table_step, row_list, None
        self.deferred, self._since_flush = None, 0                   # table_step="deferred": the DeferredRows; steps since a flush
        if table_step is not None:                                   # one RowGrad for every graph of the step
            from .optim_rows import BitmapRowGrad, RowGrad
            self.row_grad = (BitmapRowGrad if row_list == "bitmap" else RowGrad)(model.embeds.weight)
            if table_step == "deferred":                             # the step's flag word takes the unserved-row bit too
                optimizer.set_row_grad(model.embeds.weight, self.row_grad, table_step, capacity=defer_capacity,
                                       flag=self._entries_flag)
                self.deferred = optimizer.deferred_rows(model.embeds.weight)
            else:
                optimizer.set_row_grad(model.embeds.weight, self.row_grad, table_step)
        self.dirty_rows = bool(dirty_rows)
        if self.dirty_rows:
            self.row_grad.track_dirty()                              # before any capture: every graph of the step marks
        # the longest bag among the nodes that occur as columns of rows: the one host read, and only here
        lens = attr_indptr[1:] - attr_indptr[:-1]
        cols = rows.col.long()
        cols = cols[(cols >= 0) & (cols < rows.n_nodes)]
        self.longest_bag = int(lens[cols].max().item()) if cols.numel() else 0

    def _max_entries(self, B):
        if self.max_entries is not None:
            return self.max_entries
        return max(1, B * self.rows.K * self.longest_bag)

    def _front(self, batch_rows):
        self._where = "mag_prop_rows"
        S = self.samples
        # with input dropout the kernels read the state's seed where it stands: the step's, at every replay
        seed = self.state.buf[_SEED_WORD:_SEED_WORD + 1] if self.input_dropout else 0
        if self.deferred is not None:
            self._catch_up(batch_rows)
            self._where = "mag_prop_rows"
        X = self.model.emb_rows(*self.attr, self.rows, batch_rows=batch_rows, samples=S, dropnode_rate=self.dropnode_rate, seed=seed,
                                keep=self._node_keep, deterministic=self.deterministic,
                                max_entries=self._max_entries(batch_rows.numel()), overflow=self._entries_flag,
                                row_grad=self.row_grad, segment_chunk=self.segment_chunk,
                                det_input_dropout=self.input_dropout and self.deterministic)
        return X[None] if S == 1 else X

    # ---- table_step="deferred" 
    def _catch_up(self, batch_rows):
        """Before the forward: the rows of the table that the batch's bags name, listed with the bitmap kernels of §7u
        (min(V, max_entries) keys, the step's overflow bit), are brought through the step before.  With row_list="bitmap" the
        backward takes this list over instead of marking a second time: the same batch and capacity, so the list it makes today."""
        self._where = "gp_row_mark_mag"
        V = self.model.embeds.weight.shape[0]
        rows = self.rows
        keys = self.deferred.list_batch(self.attr[0], self.attr[1], rows.col, rows.filled, rows.col.numel() // rows.K, rows.K,
                                        batch_rows, min(V, self._max_entries(batch_rows.numel())), self._entries_flag)
        self._where = "gp_optim_defer_catch_up"
        self.deferred.catch_up(keys)
        if self.row_list == "bitmap":
            self.row_grad.prelisted = keys

    def flush_table(self):
        """With table_step="deferred": brings every row of the table and of its moments through the current step (one launch
        on the current stream, capturable, no host read); afterwards they hold what table_step="exact" holds.  Between
        flushes `model.embeds.weight` shows lagging rows.  `fit` calls it before every validation and before the best weights
        are restored, `optimizer.state_dict()` before a checkpoint, and `step()` / `step_sampled()` themselves from a host
        count of the steps since the last flush, before the ring of `defer_capacity` steps could be overrun.  With any other
        table_step there is nothing to do."""
        if self.deferred is not None:
            self.deferred.flush()
            self._since_flush = 0

    def _before_step(self):
        if self.deferred is not None:
            if self._since_flush >= self.deferred.capacity:          # a row may lag by `capacity` steps, and no further
                self.flush_table()
            self._since_flush += 1

    def step(self, train_sel, unlabel_sel):
        self._before_step()
        return super().step(train_sel, unlabel_sel)

    def step_sampled(self, sampler, t):
        self._before_step()
        return super().step_sampled(sampler, t)

    # ---- what the fit loop validates with
    _valid_batch = 100             # model_mag.py:372 calls `valid` without a batch size; its default (line 145) is 100

    def _valid_plan(self, idx_val, batch_size, one_pass=False):
        from .mag import valid_mag_plan
        return valid_mag_plan(self.model, self.rows, *self.attr, idx_val, self.labels, batch_size, one_pass=one_pass)

    def _valid_pass(self, plan):
        from .mag import valid_mag_pass
        self.flush_table()                                           # the pass reads the whole table: no row may lag (§7za)
        return valid_mag_pass(plan, self.dropnode_rate)

    def check_entries_flag(self):
        """Raises if a deterministic backward had more entries than `max_entries`, or, with row_list="bitmap", if a batch
        named more rows than min(V, max_entries), or, with table_step="deferred", if a row lagged further than the ring of
        `defer_capacity` steps serves (one device-to-host copy)."""
        flag = int(self._entries_flag.item())
        if flag & 2:
            raise RuntimeError(f"a row of the table lagged more than defer_capacity = {self.deferred.capacity} steps behind the step "
                               "count (or the count moved without DeferredRows.reset()): it was left as it was and is NOT on the "
                               "dense trajectory; call flush_table() at least every defer_capacity steps")
        if flag & 1:
            if self.row_list == "bitmap":
                raise RuntimeError(f"a step's batch named more table rows than max_entries = {self.max_entries}: the row list of "
                                   "that step lacks the rows past it, and the table was not stepped on them (pass a larger "
                                   "max_entries, or None)")
            raise RuntimeError(f"a step's batch had more entries than max_entries = {self.max_entries}: the table gradient of that "
                               "step lacks the entries past it (pass a larger max_entries, or None for B * K * Lmax)")
