"""A GRAND+ training step over device-resident step state, replayable from a captured graph.

Every piece of a step is HIP and free of host synchronisation (`random_prop_rows(samples=S)`, the S-sample MLP blocks,
`grand_plus_loss`, `ClipAdam`).  What kept the step from stream capture were four host numbers: the DropNode seed, the
MLP's dropout seed, the consistency weight min(lam, lam * num_batch / warmup) (model.py:329) and Adam's step count.

  * `StepState` owns one `gp_step_state` in device memory (grandplus_step.h).  `advance()` is one tiny launch that moves
    it to the next step: tick, seed = step_seed(base, tick), weight, and Adam's bias corrections per parameter group.
  * `TrainStep` is the step of model.py:305-334 over it: advance, gather the batch, write the step's dropout masks from the
    seed on the device (`gp_step_masks`), then the existing kernels fed those masks, the loss weighted by the state's
    weight, backward, `ClipAdam(capturable=True)`.  With capture=True the body of each batch shape is captured once with
    `torch.cuda.graph` and replayed; with capture=False the same body runs eagerly every call.  `step()` takes the
    batch from the host; `step_sampled()` has `gp_fit_select` draw it on the device right after the advance, so a replay
    takes no host input (`fit.py`).

`TrainStep` takes a GrandPlusMLP over dense features.  MAG's step (a MagMLP, whose front end is `mag_prop_rows` and whose
embedding table is trained) is `mag_step.MagTrainStep`, a subclass that swaps the front end of the body (`_front`) and
inherits the rest.

Left out: several optimisers, `validate=True` of the loss, and schedulers that change
`lr` between replays -- `lr` is a value of the capture; rebuild the TrainStep after changing it.
"""
from __future__ import annotations

import collections
import ctypes

import numpy as np
import torch

from . import _native
from ._common import _M64, _cuda_device, _stream, step_seed  # noqa: F401  (step_seed: public here)

__all__ = ["StepState", "TrainStep", "StepResult", "trained_parameters", "step_seed", "step_weight"]

MAX_GRAPHS = 4            # batch shapes that keep a captured graph; a further shape runs eagerly

StepResult = collections.namedtuple("StepResult", ["loss", "sup", "con", "n_conf", "n_correct", "grad_norm"])
_S = _native.GpStepState


def step_weight(lam, warmup, t):
    """gp_step_state.weight of step t >= 1 on the host: the float32 of min(lam, lam * num_batch / warmup) (model.py:329)
    with num_batch = t - 1, formed in double."""
    lam = float(lam)
    return np.float32(min(lam, lam * (t - 1) / float(warmup)))


def trained_parameters(model):
    """The parameters of a GrandPlusMLP that a training step gives a gradient: every layer's Linear and, with use_bn,
    its BatchNorm.  (Without use_bn the module still holds `bns`, as the reference does; they are never trained, and a
    capturable ClipAdam refuses a parameter without a gradient.)"""
    out = []
    for fc, bn, *_ in model._layers():
        out += list(fc.parameters()) + (list(bn.parameters()) if bn is not None else [])
    return out


class StepState:
    """One gp_step_state in device memory: tick, seed, weight, step_size[8], rsqrt_bc2[8].

    `advance(optimizer)` begins the next step on the device; nothing is read back.  `weight` is a 0-dim float32 view of
    the struct's weight, for use in the loss.  `read()` copies the struct to the host (tests and checkpoints only)."""

    def __init__(self, device, base_seed=0, lam=0.0, warmup=1.0):
        self.device = device = _cuda_device(device, "StepState")
        self.configure(base_seed, lam, warmup)
        self.buf = torch.zeros(ctypes.sizeof(_S) // 8, dtype=torch.int64, device=device)
        self.weight = self.buf.view(torch.float32)[_S.weight.offset // 4]

    def configure(self, base_seed, lam, warmup):
        """Sets what advance() derives a step from: the base seed and the weight schedule.  They are arguments of the
        launch, not device memory; `tick` is left as it is."""
        lam, warmup = float(lam), float(warmup)
        if not np.isfinite(lam) or not np.isfinite(warmup) or not warmup > 0:
            raise ValueError(f"lam must be finite and warmup finite and > 0, got lam={lam}, warmup={warmup}")
        self.base_seed, self.lam, self.warmup = int(base_seed) & _M64, lam, warmup

    def correction_ptrs(self, group):
        """Device addresses of step_size[group] and rsqrt_bc2[group]."""
        base = self.buf.data_ptr()
        return base + _S.step_size.offset + 4 * group, base + _S.rsqrt_bc2.offset + 4 * group

    def advance(self, optimizer=None):
        """tick += 1 and everything that follows from it, in one launch on the current stream.  optimizer: the ClipAdam
        whose groups' lr and betas give the bias corrections (None: no group)."""
        groups = optimizer.param_groups if optimizer is not None else []
        n = len(groups)
        if n > _native.GP_STEP_MAX_GROUPS:
            raise ValueError(f"at most {_native.GP_STEP_MAX_GROUPS} parameter groups, got {n}")
        arr = ctypes.c_double * max(n, 1)
        lr = arr(*[float(g["lr"]) for g in groups])
        b1 = arr(*[float(g["betas"][0]) for g in groups])
        b2 = arr(*[float(g["betas"][1]) for g in groups])
        rc = _native.lib().gp_step_advance(self.device.index, self.buf.data_ptr(), ctypes.c_uint64(self.base_seed), self.lam,
                                           self.warmup, n, lr, b1, b2, _stream(self.buf))
        _native.raise_for_status(rc)

    def read(self):
        """The struct as a host object with tick, seed, weight, step_size, rsqrt_bc2 (one device-to-host copy)."""
        s = _S.from_buffer_copy(self.buf.cpu().numpy().tobytes())
        return collections.namedtuple("StepStateImage", "tick seed weight step_size rsqrt_bc2")(
            int(s.tick), int(s.seed), np.float32(s.weight), np.array(s.step_size, np.float32), np.array(s.rsqrt_bc2, np.float32))

    def set_tick(self, tick):
        """Sets the number of steps begun (a checkpoint's step count); the next advance() derives the rest from it."""
        tick = int(tick)
        if tick < 0:
            raise ValueError(f"tick must be >= 0, got {tick}")
        self.buf[:1].copy_(torch.tensor([tick], dtype=torch.int64))


def rows_segment(keep, batch_rows, filled, K, S, p):
    """The DropNode mask of random_prop_rows(samples=S, keep=keep): keep uint8 [S, S_rows * K]."""
    return _native.GpStepSegment(keep=keep.data_ptr(), keep_stride=keep.numel() // S, batch_rows=batch_rows.data_ptr(),
                                 filled=filled.data_ptr() if filled is not None else None, kind=_native.GP_STEP_SEG_ROWS,
                                 n_samples=S, n_batch=batch_rows.numel(), K=K, width=0, layer=0, p=float(p), pad=0)


def layer_segment(keep, layer, p):
    """The dropout mask of MLP layer `layer`: keep uint8 [S, B, F]."""
    S, B, F = keep.shape
    return _native.GpStepSegment(keep=keep.data_ptr(), keep_stride=0, batch_rows=None, filled=None,
                                 kind=_native.GP_STEP_SEG_LAYER, n_samples=S, n_batch=B, K=0, width=F, layer=layer,
                                 p=float(p), pad=0)


def step_masks(state, segments):
    """One launch, on the current stream, that writes every segment's mask from the seed in `state` (gp_step_masks)."""
    segments = list(segments)
    tab = (_native.GpStepSegment * max(len(segments), 1))(*segments)
    rc = _native.lib().gp_step_masks(state.device.index, state.buf.data_ptr(), tab, len(segments), _stream(state.buf))
    _native.raise_for_status(rc)


def _selection(sel, n_pool, what):
    if isinstance(sel, torch.Tensor) and sel.is_cuda:
        raise TypeError(f"{what} is a host selection (a numpy array or a CPU tensor)")
    a = sel.numpy() if isinstance(sel, torch.Tensor) else np.asarray(sel)
    a = np.ascontiguousarray(a.reshape(-1), dtype=np.int64)
    if a.size and (int(a.min()) < 0 or int(a.max()) >= n_pool):
        raise IndexError(f"{what} holds an index outside [0, {n_pool})")
    return a


class TrainStep:
    """One GRAND+ training step (model.py:305-334) as one replayable object.

    model: a GrandPlusMLP in train mode; optimizer: a ClipAdam(capturable=True, state=StepState(device)) over
    `trained_parameters(model)` -- the step runs over that state, and `seed`, `lam` and `warmup` given here are set on it
    (`StepState.configure`); rows: the RowMatrix; features float32 CUDA [N, F], not requiring grad (model.py:322 detaches); labels int64 CUDA [N];
    idx_train / idx_unlabel: the node ids of the two pools.  Their row positions are looked up once here
    (`batch_positions(check=True)`: an unknown id is a KeyError) and stay on the device with labels[idx_train].

    `step(train_sel, unlabel_sel)` takes selections INTO the pools (numpy arrays or CPU tensors; what
    iterate_minibatches_listinputs and sample_unlabel produce), range-checks them on the host (IndexError before the
    device is touched) and runs: advance -> gather rows and labels -> gp_step_masks -> random_prop_rows(samples=S, keep) ->
    model(X, keep) -> grand_plus_loss -> (sup + weight * con).backward() -> optimizer.step().  It returns a StepResult of
    0-dim device tensors (loss, sup, con, n_conf, n_correct, grad_norm), valid until the next call.

    capture=True: the first call of a batch shape (B, n_labeled) runs eagerly (a real step; it loads code and creates
    the optimiser state), the second captures the body with torch.cuda.graph and replays it, every later one is one
    replay.  At most MAX_GRAPHS shapes keep a graph; a further shape runs eagerly.  A capture that raises is re-raised
    with the name of the call that broke it; there is no retry and no fallback.  capture=False runs the same body
    eagerly every call.  `lr` and the betas are values of the capture."""

    def __init__(self, model, optimizer, rows, features, labels, idx_train, idx_unlabel, *, samples, dropnode_rate, lam,
                 warmup, tem, conf=None, kind="l2", seed, capture=True):
        from .mlp import GrandPlusMLP
        if not isinstance(model, GrandPlusMLP):
            raise ValueError("TrainStep takes a GrandPlusMLP (a MagMLP goes to mag_step.MagTrainStep: DESIGN §7o)")
        self._check_optimizer_and_rows(optimizer, rows)
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or \
                not features.is_contiguous():
            raise ValueError("features must be a contiguous float32 [N, F] tensor")
        if features.requires_grad:
            raise ValueError("features must not require grad: the step trains the MLP alone (model.py:322 detaches)")
        self._check_hyperparameters(model, optimizer, samples, dropnode_rate, kind, tem)
        if not features.is_cuda:
            raise ValueError("the step runs on the GPU only: features must be a CUDA tensor (no CPU fallback)")
        if not isinstance(labels, torch.Tensor) or labels.dtype != torch.int64 or labels.device != features.device:
            raise ValueError("labels must be an int64 tensor on the device of features")
        dev = features.device
        if features.shape[0] != rows.n_nodes or rows.col.device != dev:
            raise ValueError(f"features must have one row per node ({rows.n_nodes}) on the device of rows ({rows.col.device})")
        self.features = features
        self._setup(model, optimizer, rows, labels, idx_train, idx_unlabel, dev, samples=samples, dropnode_rate=dropnode_rate,
                    lam=lam, warmup=warmup, tem=tem, conf=conf, kind=kind, seed=seed, capture=capture)

    # ---- the refusals and the state that every step shares (mag_step.MagTrainStep calls them too)
    @staticmethod
    def _check_optimizer_and_rows(optimizer, rows):
        from .optim import ClipAdam
        from .rows import RowMatrix
        if not isinstance(optimizer, ClipAdam) or not optimizer.capturable:
            raise ValueError("TrainStep takes a ClipAdam(capturable=True)")
        if not isinstance(rows, RowMatrix):
            raise ValueError("rows must be a RowMatrix")

    @staticmethod
    def _check_hyperparameters(model, optimizer, samples, dropnode_rate, kind, tem):
        if not isinstance(samples, int) or not 1 <= samples <= _native.GP_MAX_SAMPLES:
            raise ValueError(f"samples must be an int in [1, {_native.GP_MAX_SAMPLES}], got {samples!r}")
        if not 0.0 <= float(dropnode_rate) <= 1.0:
            raise ValueError(f"dropnode_rate must be in [0, 1], got {dropnode_rate}")
        if kind not in ("kl", "l2"):
            raise ValueError(f"kind must be 'kl' or 'l2', got {kind!r}")
        if not float(tem) > 0.0:
            raise ValueError(f"tem must be > 0, got {tem!r}")
        if len(model._layers()) > _native.GP_STEP_MAX_LAYERS:
            raise ValueError(f"at most {_native.GP_STEP_MAX_LAYERS} layers, got {len(model._layers())}")
        if len(optimizer.param_groups) > _native.GP_STEP_MAX_GROUPS:
            raise ValueError(f"at most {_native.GP_STEP_MAX_GROUPS} parameter groups, got {len(optimizer.param_groups)}")

    def _setup(self, model, optimizer, rows, labels, idx_train, idx_unlabel, dev, *, samples, dropnode_rate, lam, warmup, tem,
               conf, kind, seed, capture):
        self.model, self.optimizer, self.rows, self.device = model, optimizer, rows, dev
        self.samples, self.dropnode_rate, self.tem, self.conf, self.kind = samples, float(dropnode_rate), float(tem), conf, kind
        self.capture = bool(capture)
        idx_train = torch.as_tensor(np.asarray(idx_train).reshape(-1), dtype=torch.int64)
        idx_unlabel = torch.as_tensor(np.asarray(idx_unlabel).reshape(-1), dtype=torch.int64)
        self.n_train, self.n_unlabel = idx_train.numel(), idx_unlabel.numel()
        # positions of both pools, labelled first: a selection into the unlabelled pool is offset by n_train
        self._pos = rows.batch_positions(torch.cat([idx_train, idx_unlabel]), check=True)
        self._pool_labels = labels[idx_train.to(dev)].contiguous()
        self.state = optimizer.step_state                          # the optimiser's: its tick is Adam's step count
        if self.state.device != dev:
            raise ValueError(f"the optimiser's StepState is on {self.state.device}, the step's tensors on {dev}")
        self.state.configure(seed, lam, warmup)
        self._node_keep = torch.zeros((samples, rows.col.numel()), dtype=torch.uint8, device=dev) \
            if self.dropnode_rate > 0 else None
        self._shapes = {}              # (B, n_labeled) -> None after the eager call, then its _Graph
        self._sampled = {}             # the same for step_sampled, keyed by what its capture freezes
        self.labels = labels
        self._sel_flag = torch.zeros(1, dtype=torch.int32, device=dev)      # bit 0: a step_sampled ran with a wrong shape
        self._where = None

    # ---- one step's launches: what a graph captures
    def _body(self, sel, n_l, sampler=None):
        m, S, st = self.model, self.samples, self.state
        layers = m._layers()
        self._where = "optimizer.zero_grad"
        self.optimizer.zero_grad(set_to_none=True)
        self._where = "gp_step_advance"
        st.advance(self.optimizer)
        if sampler is not None:                                      # step_sampled: the device draws the new tick's selection
            self._where = "gp_fit_select"
            from .fit import fit_select
            fit_select(st, sampler, n_l, sel, self._sel_flag)
        self._where = "index_select"
        batch_rows = self._pos.index_select(0, sel)
        y = self._pool_labels.index_select(0, sel[:n_l]) if n_l else None
        B = batch_rows.numel()
        self._where = "gp_step_masks"
        segments = []
        if self._node_keep is not None:
            segments.append(rows_segment(self._node_keep, batch_rows, self.rows.filled, self.rows.K, S, self.dropnode_rate))
        keeps = []
        for l, (fc, _bn, _relu, _norm, _detach, p) in enumerate(layers):
            keeps.append(torch.empty((S, B, fc.weight.shape[1]), dtype=torch.uint8, device=sel.device) if p > 0 else None)
            if keeps[-1] is not None:
                segments.append(layer_segment(keeps[-1], l, p))
        step_masks(st, segments)
        X = self._front(batch_rows)
        from .objective import grand_plus_loss
        self._where = "model"
        z = m(X, seed=0, keep=keeps)
        self._where = "grand_plus_loss"
        _, parts = grand_plus_loss(z, y, n_l, 0.0, tem=self.tem, conf=self.conf, kind=self.kind)
        loss = parts["sup"] + st.weight * parts["con"]
        self._where = "backward"
        loss.backward()
        self._where = "optimizer.step"
        norm = self.optimizer.step()
        self._where = None
        return StepResult(loss.detach(), parts["sup"].detach(), parts["con"].detach(), parts["n_conf"], parts["n_correct"], norm)

    def _front(self, batch_rows):
        """The front end of the body: the S augmented inputs [S, B, F] of the batch, under the DropNode mask that
        gp_step_masks has just written.  The one part of the body a subclass swaps."""
        self._where = "random_prop_rows"
        from .augment import random_prop_rows
        X = random_prop_rows(self.features, self.rows.col, self.rows.val, self.rows.filled, self.rows.K, batch_rows=batch_rows,
                             dropnode_rate=self.dropnode_rate, training=True, seed=0, keep=self._node_keep, samples=self.samples)
        return X[None] if self.samples == 1 else X

    def step(self, train_sel, unlabel_sel):
        if not self.model.training:
            raise RuntimeError("TrainStep.step() needs the model in train mode: call model.train() (eval / train are the caller's)")
        a = _selection(train_sel, self.n_train, "train_sel")
        b = _selection(unlabel_sel, self.n_unlabel, "unlabel_sel")
        n_l, B = a.size, a.size + b.size
        if B < 1:
            raise IndexError("the batch is empty")
        host = torch.from_numpy(np.concatenate([a, b + self.n_train]))
        key = (B, n_l)
        if not self.capture or (key not in self._shapes and len(self._shapes) >= MAX_GRAPHS):
            return self._body(host.pin_memory().to(self.device, non_blocking=True), n_l)
        if key not in self._shapes:                                  # the first call of a shape: a real, eager step
            self._shapes[key] = None
            return self._body(host.pin_memory().to(self.device, non_blocking=True), n_l)
        if self._shapes[key] is None:
            self._shapes[key] = self._capture(B, n_l)
        sel, graph, result = self._shapes[key]
        # a pinned block goes back to torch's host allocator only after this copy has run, so the next step may start early
        sel.copy_(host.pin_memory(), non_blocking=True)
        graph.replay()
        return result

    # ---- what the fit loop validates with (fit.FitLoop); mag_step.MagTrainStep swaps both
    def _valid_plan(self, idx_val, batch_size, one_pass=False):
        from .evaluate import valid_plan
        return valid_plan(self.model, self.rows, self.features, idx_val, self.labels, batch_size, one_pass=one_pass)

    def _valid_pass(self, plan):
        from .evaluate import valid_pass
        return valid_pass(plan, self.dropnode_rate)

    _valid_batch = None            # the validation batch size `fit` uses when it is given none: None is the sampler's

    # ---- the step with the selection drawn on the device
    def check_sampler(self, sampler):
        if (sampler.n_train, sampler.n_unlabel) != (self.n_train, self.n_unlabel):
            raise ValueError(f"the sampler draws from pools of {sampler.n_train} and {sampler.n_unlabel} nodes, "
                             f"the step holds {self.n_train} and {self.n_unlabel}")

    def check_selection_flag(self):
        """Raises if a step_sampled ran with a batch shape that was not its step's (one device-to-host copy)."""
        if int(self._sel_flag.item()) & 1:
            raise RuntimeError("a step_sampled(sampler, t) ran with the batch shape of another step: t was not the tick of "
                               "the step state (the selection stayed inside the pools, but the labelled batch was not the step's)")

    def step_sampled(self, sampler, t):
        """step() with the selection of fit.Sampler drawn on the device: advance -> gp_fit_select -> the rest of the body.
        t: the step this call runs, the state's tick + 1; the host needs it for the batch shape alone, `sampler.shape(t)`.
        Bitwise `step(*sampler.selection(t, step_seed(base, t)))`; a replay takes no host input at all.  Graphs are kept per
        shape under the same MAX_GRAPHS limit as step()'s, apart from them."""
        if not self.model.training:
            raise RuntimeError("TrainStep.step_sampled() needs the model in train mode: call model.train() (eval / train are the caller's)")
        self.check_sampler(sampler)
        n_l, u = sampler.shape(t)
        B = n_l + u
        key = (B, n_l, sampler.batch_size, sampler.unlabel_batch, sampler.base_seed)    # the values a capture freezes
        if not self.capture or (key not in self._sampled and len(self._sampled) >= MAX_GRAPHS):
            return self._body(torch.empty(B, dtype=torch.int64, device=self.device), n_l, sampler)
        if key not in self._sampled:                                 # the first call of a shape: a real, eager step
            self._sampled[key] = None
            return self._body(torch.empty(B, dtype=torch.int64, device=self.device), n_l, sampler)
        if self._sampled[key] is None:
            self._sampled[key] = self._capture(B, n_l, sampler)
        _sel, graph, result = self._sampled[key]
        graph.replay()
        return result

    def _capture(self, B, n_l, sampler=None):
        dev = self.device
        sel = torch.zeros(B, dtype=torch.int64, device=dev)         # static: a replay reads the selection from here
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph):                            # one side stream; nothing runs until the replay
                result = self._body(sel, n_l, sampler)
        except Exception as e:
            where, self._where = self._where, None
            raise RuntimeError(f"capturing the training step broke in {where}: {e}") from e
        return sel, graph, result
