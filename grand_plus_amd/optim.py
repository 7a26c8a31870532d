"""Gradient clipping and Adam on MI355X, over the fused HIP kernels of csrc/optim.hip.

Reference, at the end of every training step (`model.py:116-120, 333-334`, same in `model_mag.py`):

    grad_norm = clip_grad_norm(model.parameters(), args.clip_norm);  optimizer.step()        # torch.optim.Adam

Here that is two launches for the whole model -- one float64 sum of squares over every gradient, one kernel that forms
the clip coefficient and applies Adam -- with no host synchronisation: `ClipAdam.step()` returns the norm as a 0-dim
device tensor and reads nothing back.

Documented difference from the reference: `ClipAdam.step()` leaves `p.grad` unscaled (the coefficient is applied while
the update reads the gradient; the reference never looks at the gradients after the step).  `clip_grad_norm` is the
standalone form and does scale them in place.  float32 CUDA parameters only: there is no CPU fallback.
"""
from __future__ import annotations

import math

import torch

from . import _native
from ._common import _stream
from .optim_rows import DeferredRows, RowGrad, check_capacity, check_mode, clip_adam_rows, sqnorm

__all__ = ["ClipAdam", "clip_grad_norm"]


def _check_tensor(t, what):
    if not isinstance(t, torch.Tensor) or t.is_sparse:
        raise TypeError(f"{what} must be a dense tensor (sparse gradients are not supported)")
    # the kernels read every pointer as a dense float*: dtype and layout come first, so that they are refused on any device
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32, got {t.dtype} (no CPU fallback, no other precision)")
    if not t.is_contiguous():
        raise TypeError(f"{what} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)} "
                        f"(no CPU fallback, no strided path)")
    if not t.is_cuda:
        raise TypeError(f"{what} must be a CUDA tensor: the optimiser runs on the GPU only (no CPU fallback)")


def _no_gradients(params):
    """The norm of no gradients: 0 as a 0-dim float32 tensor on the device of the first parameter, if there is one."""
    dev = params[0].device if params else None
    return torch.zeros((), dtype=torch.float32, device=dev)


def _table(entries):
    """The host array of gp_optim_tensor for (param, grad, exp_avg, exp_avg_sq) tuples (None = NULL)."""
    tab = (_native.GpOptimTensor * max(len(entries), 1))()
    for e, (p, g, m, v) in zip(tab, entries):
        e.param = p.data_ptr() if p is not None else None
        e.grad = g.data_ptr()
        e.exp_avg = m.data_ptr() if m is not None else None
        e.exp_avg_sq = v.data_ptr() if v is not None else None
        e.numel = g.numel()
    return tab


def _buffers(dev):
    """(workspace, norm scalar) from torch's caching allocator."""
    return (torch.empty(_native.optim_workspace_bytes(), dtype=torch.uint8, device=dev),
            torch.empty((), dtype=torch.float32, device=dev))


def _call(dev, like, entries, flags, ws, norm, max_norm=0.0, lr=0.0, betas=(0.0, 0.0), eps=0.0, weight_decay=0.0,
          step_size=0.0, rsqrt_bc2=0.0):
    rc = _native.lib().gp_clip_adam_step(dev.index, _table(entries), len(entries), flags, max_norm, lr, betas[0], betas[1],
                                         eps, weight_decay, step_size, rsqrt_bc2, ws.data_ptr(), norm.data_ptr(), _stream(like))
    _native.raise_for_status(rc)


def _call_dev(dev, like, entries, flags, ws, norm, d_step_size, d_rsqrt_bc2, max_norm, lr, betas, eps, weight_decay):
    """_call with the two bias corrections read on the device (gp_clip_adam_step_dev): addresses inside a gp_step_state."""
    rc = _native.lib().gp_clip_adam_step_dev(dev.index, _table(entries), len(entries), flags, max_norm, lr, betas[0], betas[1],
                                             eps, weight_decay, d_step_size, d_rsqrt_bc2, ws.data_ptr(), norm.data_ptr(),
                                             _stream(like))
    _native.raise_for_status(rc)


def clip_grad_norm(params, max_norm):
    """Drop-in for the reference's `clip_grad_norm(params, max_norm)` (model.py:116-120): the 2-norm of all gradients as a
    0-dim float32 device tensor; with max_norm > 0 the gradients are scaled in place by min(max_norm / (norm + 1e-6), 1)
    (torch's `clip_grad_norm_`), otherwise they are left alone.  Parameters without a gradient are skipped; with no
    gradient at all the result is 0 on the first parameter's device and nothing is launched."""
    params = [params] if isinstance(params, torch.Tensor) else list(params)
    grads = [p.grad for p in params if p.grad is not None]
    if not grads:
        return _no_gradients(params)
    for g in grads:
        _check_tensor(g, "a gradient")
        if g.device != grads[0].device:
            raise TypeError("all gradients must be on one device")
    dev = grads[0].device
    ws, norm = _buffers(dev)
    _call(dev, grads[0], [(None, g, None, None) for g in grads], _native.GP_OPTIM_CLIP_ONLY, ws, norm, max_norm=float(max_norm))
    return norm


class ClipAdam(torch.optim.Optimizer):
    """`clip_grad_norm_(all parameters, clip_norm)` followed by `torch.optim.Adam.step()`, as one pair of launches.

    Arguments, their range checks and the state (`step`, `exp_avg`, `exp_avg_sq`) are torch.optim.Adam's, so a checkpoint
    of either loads into the other; `step` is kept as a Python number here.  clip_norm <= 0 means no clipping
    (model.py:119-120).  One norm is taken over the gradients of ALL parameter groups; the hyper-parameters are per group.
    `step()` returns that norm, before clipping, as a 0-dim float32 device tensor (a closure is called for its gradients;
    its loss is not returned).  `p.grad` is left unscaled.  Parameters whose `.grad` is None are skipped and get no state;
    if none has a gradient, `step()` returns 0 on the first parameter's device and launches nothing.
    Every parameter that has a gradient must be a contiguous float32 CUDA tensor, all on one device: `step()` raises
    TypeError otherwise, before anything is launched or any state changes (the constructor accepts a model that is still
    on the CPU).  The same holds for `exp_avg` and `exp_avg_sq` of a loaded checkpoint.

    capturable=True, state=<step.StepState> keeps the step count on the device, so that `step()` is a fixed
    sequence of launches with fixed arguments and can be replayed from a captured graph.  The count is `tick` of the
    StepState given here as `state` (capturable=True without one is a TypeError: a required argument is missing); the
    caller advances it once per step (`state.advance(optimizer)`), and `step()` reads lr / (1 - beta1^t) and
    1 / sqrt(1 - beta2^t) from it on the device.  One count serves every parameter, so `step()` raises ValueError, before
    any launch, for a parameter without a gradient, for parameters whose loaded `step` values differ from one another and
    for more than 8 parameter groups.  `state_dict()` reports `step` as the number torch.optim.Adam would hold (one host
    read of `tick`); `load_state_dict()` sets `tick` from it.  `lr` and the betas are read when the state advances: under a
    captured graph they are the values of the capture.

    `set_row_grad(param, row_grad, mode)` steps one [V, H] embedding table from a row list instead of a dense
    `.grad`: see there.  mode "lazy" is NOT the reference's dense Adam.  mode "deferred"  is, bit for bit, at
    "lazy"'s memory traffic: it needs capturable=True, and `flush_rows()` brings its lagging rows up to date (`state_dict()`
    calls it first; `load_state_dict()` makes every row current through the loaded step).
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, clip_norm=0.0, *,
                 amsgrad=False, maximize=False, capturable=False, state=None):
        if amsgrad or maximize:
            raise ValueError("ClipAdam does not implement amsgrad or maximize")
        if capturable and state is None:
            raise TypeError("ClipAdam(capturable=True) is missing its StepState: pass state=StepState(device, seed, lam, warmup)")
        if state is not None and not capturable:
            raise ValueError("state= is the step count of ClipAdam(capturable=True); without capturable the count is a host number")
        self.capturable = bool(capturable)
        self.step_state = state
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise ValueError("ClipAdam takes lr and betas as Python numbers, not Tensors")
        if not math.isfinite(float(clip_norm)):
            raise ValueError(f"Invalid clip_norm value: {clip_norm}")
        # torch.optim.Adam's own constructor checks the ranges (its messages) and names the keys of a parameter group
        probe = torch.optim.Adam([torch.nn.Parameter(torch.empty(0))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.clip_norm = float(clip_norm)
        self._row_grads = {}                                         # parameter -> (RowGrad, mode): set_row_grad
        self._deferred = {}                                          # parameter -> DeferredRows, for mode "deferred"
        super().__init__(params, dict(probe.defaults))

    def set_row_grad(self, param, row_grad, mode, capacity=None, flag=None):
        """Steps `param`, a [V, H] embedding table of this optimiser, from `row_grad` (an optim_rows.RowGrad(param), filled by
        the deterministic backward of `mag_prop_rows(..., row_grad=row_grad)`) instead of `param.grad`, which stays None.
        The parameter counts as having a gradient: the one norm of `step()` includes its touched rows, and its state
        (`step`, dense `exp_avg` and `exp_avg_sq`) and checkpoints are torch.optim.Adam's, unchanged.

        mode "exact": every element gets the update the dense path gives it, bit for bit; an untouched row takes g = 0.0f.
        mode "lazy": only the touched rows of the parameter and of its moments are read and written; every other row keeps
        its bits.  This is NOT the reference's trajectory: under dense torch.optim.Adam (model_mag.py:312) an untouched row
        still moves while its moments decay.  The group's weight_decay must be 0 in this mode (ValueError, here and in
        `step()`): a decay applied to the touched rows alone is nobody's semantics.
        mode "deferred" (DESIGN §7za): the trajectory of "exact", bit for bit, at the memory traffic of "lazy".  The
        zero-gradient update of an untouched row is put off and replayed, step by step through the same element update,
        when the row is next read (`deferred_rows(param).catch_up(keys)`, before the forward) and by `flush_rows()`.
        Weight decay is allowed.  It needs capturable=True (ValueError otherwise): the step number is read on the device.
        capacity: the steps of history kept, a power of two in [4, 65536] (None: 1024); `flush_rows()` is due at least that
        often.  flag: an int32 [1] tensor whose bit 1 a row that could not be served sets (None: a private one).
        BETWEEN FLUSHES THE TABLE AND ITS MOMENTS SHOW LAGGING ROWS; `state_dict()` flushes first.

        A `step()` before any backward has filled the RowGrad is a RuntimeError."""
        if not isinstance(row_grad, RowGrad):
            raise TypeError(f"row_grad must be an optim_rows.RowGrad, got {type(row_grad).__name__}")
        check_mode(mode)
        if mode == "deferred":
            if not self.capturable:
                raise ValueError("mode 'deferred' reads the step count on the device: it needs ClipAdam(capturable=True, state=...)")
            capacity = check_capacity(capacity)
        elif capacity is not None or flag is not None:
            raise ValueError(f"capacity= and flag= belong to mode 'deferred', got mode {mode!r}")
        group = next((g for g in self.param_groups if any(p is param for p in g["params"])), None)
        if group is None:
            raise ValueError("set_row_grad: param is not a parameter of this optimiser")
        row_grad.check_weight(param)
        if mode == "lazy" and float(group["weight_decay"]) != 0.0:
            raise ValueError(f"mode 'lazy' takes weight_decay = 0, the parameter's group has {group['weight_decay']}: a decay "
                             "applied to the touched rows alone is nobody's semantics")
        self._deferred.pop(param, None)
        if mode == "deferred":
            self._deferred[param] = DeferredRows(self, param, self.param_groups.index(group), capacity, flag)
        self._row_grads[param] = (row_grad, mode)

    def deferred_rows(self, param):
        """The optim_rows.DeferredRows of a parameter set to mode "deferred" (KeyError otherwise)."""
        return self._deferred[param]

    def flush_rows(self):
        """Brings every row of every table in mode "deferred" through the current step (one launch per table, capturable, no
        host read): afterwards the tables and their moments hold what the dense step holds.  Nothing to do without one."""
        for deferred in self._deferred.values():
            deferred.flush()

    def load_state_dict(self, state_dict):
        if self.capturable:
            steps = {self._number(s["step"]) for s in state_dict["state"].values() if "step" in s}
            if len(steps) > 1:
                raise ValueError(f"a capturable ClipAdam keeps one step count for all parameters: the checkpoint holds {sorted(steps)}")
        super().load_state_dict(state_dict)
        for s in self.state.values():                                # torch.optim.Adam keeps `step` as a tensor
            if "step" in s:
                s["step"] = self._number(s["step"])
        if self.capturable:
            self.step_state.set_tick(steps.pop() if steps else 0)
            for deferred in self._deferred.values():                 # the loaded table is current through the loaded tick
                deferred.reset()

    def state_dict(self):
        self.flush_rows()                                            # a checkpoint holds no lagging row
        out = super().state_dict()
        if self.capturable and out["state"]:
            # in self.state `step` is what a checkpoint brought (the same for all, 0 without one) and never moves
            t = self.step_state.read().tick
            out["state"] = {k: {**s, "step": t} if "step" in s else s for k, s in out["state"].items()}
        return out

    @staticmethod
    def _number(step):
        return int(step.item() if isinstance(step, torch.Tensor) else step)

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            with torch.enable_grad():
                closure()
        todo, calls, dev = [], {}, None                              # calls: (group index, step count) -> entries
        rows = []                                                    # (group index, parameter, RowGrad, mode): set_row_grad
        if self.capturable:
            self._check_capturable()
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise ValueError("ClipAdam does not implement amsgrad, maximize or decoupled_weight_decay")
            for p in group["params"]:
                g = p.grad
                rg, mode = self._row_grads.get(p, (None, None))
                if rg is not None:                                   # the gradient is the RowGrad's rows
                    if g is not None:
                        raise ValueError("a parameter with a row gradient (set_row_grad) also has a dense .grad")
                    if mode == "lazy" and float(group["weight_decay"]) != 0.0:
                        raise ValueError(f"mode 'lazy' takes weight_decay = 0, the parameter's group has {group['weight_decay']}")
                    if not rg.filled():
                        raise RuntimeError("ClipAdam.step(): no backward has filled the parameter's RowGrad yet (run the "
                                           "deterministic backward of mag_prop_rows(..., row_grad=...) first)")
                    g = rg.values
                elif g is None:
                    continue
                _check_tensor(g, "a gradient")
                _check_tensor(p, "a parameter")
                if dev is None:
                    dev = p.device
                if p.device != dev or g.device != dev:
                    raise TypeError("all parameters and gradients must be on one device")
                loaded = self.state.get(p) or {}                     # state of an earlier step or of a checkpoint
                for key in ("exp_avg", "exp_avg_sq") if loaded else ():
                    s = loaded[key]
                    _check_tensor(s, key)
                    if s.device != dev or s.shape != p.shape:
                        raise TypeError(f"{key} must have its parameter's device and shape, got {tuple(s.shape)} on {s.device}")
                if rg is not None:
                    rows.append((gi, p, rg, mode))
                else:
                    todo.append((gi, p, g))
        if self.capturable:
            return self._step_capturable(todo, dev, rows)
        row_calls = []
        for gi, p, rg, mode in rows:
            state = self._init_state(p)
            state["step"] = self._number(state["step"]) + 1
            row_calls.append((gi, state["step"], p, rg, mode))
        for gi, p, g in todo:                                        # every check has passed: now the state may change
            state = self._init_state(p)
            t = state["step"] = self._number(state["step"]) + 1
            calls.setdefault((gi, t), []).append((p, g, state["exp_avg"], state["exp_avg_sq"]))
        if dev is None:
            return _no_gradients([p for group in self.param_groups for p in group["params"]])
        ws, norm = _buffers(dev)
        like = next(iter(calls.values()))[0][0] if calls else row_calls[0][2]
        flags = self._norm_first(dev, like, calls, [rg for _, _, _, rg, _ in row_calls], ws, norm)
        for (gi, t), entries in calls.items():
            group = self.param_groups[gi]
            lr, (beta1, beta2) = float(group["lr"]), group["betas"]
            _call(dev, like, entries, flags, ws, norm, max_norm=self.clip_norm, lr=lr, betas=(float(beta1), float(beta2)),
                  eps=float(group["eps"]), weight_decay=float(group["weight_decay"]),
                  step_size=lr / (1.0 - beta1 ** t), rsqrt_bc2=1.0 / math.sqrt(1.0 - beta2 ** t))
        for gi, t, p, rg, mode in row_calls:
            group = self.param_groups[gi]
            lr, (beta1, beta2) = float(group["lr"]), group["betas"]
            self._rows_update(gi, p, rg, mode, ws, norm, step_size=lr / (1.0 - beta1 ** t),
                              rsqrt_bc2=1.0 / math.sqrt(1.0 - beta2 ** t))
        return norm

    def _init_state(self, p):
        """The Adam state of p, created on its first step as torch.optim.Adam creates it (a capturable optimiser leaves `step`
        at what a checkpoint brought: its count is the state's tick)."""
        state = self.state[p]
        if len(state) == 0:
            state["step"] = 0
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return state

    def _rows_update(self, gi, p, rg, mode, ws, norm, **corrections):
        """The table's update from its RowGrad with the hyper-parameters of group gi; corrections: step_size and rsqrt_bc2 as
        numbers, or d_step_size and d_rsqrt_bc2 as device addresses."""
        group = self.param_groups[gi]
        beta1, beta2 = group["betas"]
        clip_adam_rows(rg, mode, self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"], ws, norm, max_norm=self.clip_norm,
                       lr=float(group["lr"]), betas=(float(beta1), float(beta2)), eps=float(group["eps"]),
                       weight_decay=float(group["weight_decay"]), **corrections)

    @staticmethod
    def _norm_first(dev, like, calls, row_grads, ws, norm):
        """The norm launches that come before the updates, and the flags of the dense updates after them.  Without a row
        gradient: today's sequence (one norm-only launch when several calls share the norm).  With one: the dense
        gradients' norm-only launch, if there is any dense gradient, then every RowGrad's rows added into the same
        workspace; the updates then find the norm ready."""
        if not row_grads:
            if len(calls) > 1:                                       # one norm over everything, then an update per group
                _call(dev, like, [e for entries in calls.values() for e in entries], _native.GP_OPTIM_NORM_ONLY, ws, norm)
                return _native.GP_OPTIM_NORM_READY
            return 0
        first = True
        if calls:
            _call(dev, like, [e for entries in calls.values() for e in entries], _native.GP_OPTIM_NORM_ONLY, ws, norm)
            first = False
        for rg in row_grads:
            sqnorm(rg, not first, ws)
            first = False
        return _native.GP_OPTIM_NORM_READY

    def _check_capturable(self):
        """What one device-resident step count cannot serve: ValueError before anything is launched or any state changes."""
        if len(self.param_groups) > _native.GP_STEP_MAX_GROUPS:
            raise ValueError(f"ClipAdam(capturable=True) takes at most {_native.GP_STEP_MAX_GROUPS} parameter groups, "
                             f"got {len(self.param_groups)}")
        steps = set()
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None and p not in self._row_grads:
                    raise ValueError("ClipAdam(capturable=True) steps every parameter with one step count: a parameter has no "
                                     "gradient (give the optimiser only the parameters that are trained)")
                steps.add(self._number((self.state.get(p) or {}).get("step", 0)))
        if len(steps) > 1:
            raise ValueError(f"ClipAdam(capturable=True) keeps one step count for all parameters: the loaded values are {sorted(steps)}")

    def _step_capturable(self, todo, dev, rows=()):
        """The launches of step() with the bias corrections of group gi read from the optimiser's gp_step_state."""
        calls = {}
        for _gi, p, _rg, _mode in rows:
            self._init_state(p)
        for gi, p, g in todo:
            state = self._init_state(p)
            calls.setdefault(gi, []).append((p, g, state["exp_avg"], state["exp_avg_sq"]))
        if dev is None:
            return _no_gradients([p for group in self.param_groups for p in group["params"]])
        if self.step_state.device != dev:
            raise TypeError(f"the StepState is on {self.step_state.device}, the parameters on {dev}")
        ws, norm = _buffers(dev)
        like = next(iter(calls.values()))[0][0] if calls else rows[0][1]
        flags = self._norm_first(dev, like, calls, [rg for _, _, rg, _ in rows], ws, norm)
        for gi, entries in calls.items():
            group = self.param_groups[gi]
            beta1, beta2 = group["betas"]
            d_step_size, d_rsqrt_bc2 = self.step_state.correction_ptrs(gi)
            _call_dev(dev, like, entries, flags, ws, norm, d_step_size, d_rsqrt_bc2, max_norm=self.clip_norm, lr=float(group["lr"]),
                      betas=(float(beta1), float(beta2)), eps=float(group["eps"]), weight_decay=float(group["weight_decay"]))
        for gi, p, rg, mode in rows:
            d_step_size, d_rsqrt_bc2 = self.step_state.correction_ptrs(gi)
            if mode == "deferred":
                self._deferred[p].step(rg, ws, norm, self.clip_norm, d_step_size, d_rsqrt_bc2)
            else:
                self._rows_update(gi, p, rg, mode, ws, norm, d_step_size=d_step_size, d_rsqrt_bc2=d_rsqrt_bc2)
        return norm
