"""GRAND+'s training objective after the MLP on MI355X, over the fused HIP kernels of csrc/objective.hip.

Reference, per step with S = `--sample` augmentations (`model.py:321-331`, `model_mag.py:354-366`):

    logp[s] = log_softmax(z[s]);  loss = (1/S) sum_s nll_loss(logp[s][:n_l], y) + w * consis_loss(logp[:, n_l:], tem, conf)

with `consis_loss` of `model.py:123-139`.  Here that is one forward launch, one reduce and one backward launch, with
no host synchronisation: `parts` holds 0-dim device tensors and nothing is read back (unless `validate=True`).

Two documented differences from the reference, which agree wherever p does not underflow in fp32:
  * sharp_p = softmax(log(avg_p) / tem) is formed in the log domain, so avg_p ** (1/tem) never underflows to 0/0;
  * kl uses logp where the reference uses log(exp(logp)).
A mean over an empty set (no confident row, no labelled row) is NaN in the value and adds no gradient, as
`torch.mean` of an empty tensor does.  Labels equal to `ignore_index` are left out as in `F.nll_loss`; other labels
outside [0, C) are never used as an index: they are left out and counted in parts["n_bad_labels"].
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._common import _ptr, _stream

_KINDS = {"kl": _native.GP_LOSS_KL, "l2": _native.GP_LOSS_L2}


def _loss_call(z, labels, n_labeled, weight, tem, conf, kind, ignore_index, logp_in):
    S, B, C = z.shape
    out = torch.empty(3, dtype=torch.float32, device=z.device)
    counts = torch.empty(4, dtype=torch.int32, device=z.device)
    ws = torch.empty(max(_native.grand_loss_workspace_bytes(B), 8), dtype=torch.uint8, device=z.device)
    rc = _native.lib().gp_grand_loss(
        z.device.index, z.data_ptr(), S, B, C, _ptr(labels), n_labeled, ignore_index,
        float(weight), float(tem), float(conf), kind, int(logp_in), ws.data_ptr(), out.data_ptr(), counts.data_ptr(), _stream(z))
    _native.raise_for_status(rc)
    return out, counts


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, labels, n_labeled, weight, tem, conf, kind, ignore_index, logp_in):
        out, counts = _loss_call(z, labels, n_labeled, weight, tem, conf, kind, ignore_index, logp_in)
        ctx.save_for_backward(z, labels, counts)
        ctx.args = (n_labeled, weight, tem, conf, kind, ignore_index, logp_in)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(counts)
        return out[0], out[1], out[2], counts

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, g_sup, g_con, _g_counts):
        z, labels, counts = ctx.saved_tensors
        n_labeled, weight, tem, conf, kind, ignore_index, logp_in = ctx.args
        S, B, C = z.shape
        if g_loss is None:
            g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
        g_loss, g_sup, g_con = (g.float().contiguous() if g is not None else None for g in (g_loss, g_sup, g_con))
        dz = torch.empty_like(z)
        rc = _native.lib().gp_grand_loss_backward(
            z.device.index, z.data_ptr(), S, B, C, _ptr(labels), n_labeled,
            ignore_index, float(weight), float(tem), float(conf), kind, int(logp_in), g_loss.data_ptr(),
            _ptr(g_sup), _ptr(g_con), counts.data_ptr(), dz.data_ptr(), _stream(z))
        _native.raise_for_status(rc)
        return dz, None, None, None, None, None, None, None, None


def grand_plus_loss(logits, labels, n_labeled, weight, *, tem=0.1, conf=None, kind="l2", ignore_index=-100,
                    validate=False, inputs_are_log_probs=False):
    """The GRAND+ objective of one training step: (loss, parts).

    logits: float32 CUDA [S, B, C] tensor, or a sequence of S [B, C] tensors (stacked; the gradient flows back through the
    stack).  Rows b < n_labeled carry `labels[b]` (int64 CUDA tensor, at least n_labeled entries; None when n_labeled = 0),
    in the order of `batch_index = concat(train_index, unlabel_index_batch)` (model.py:309).  `weight` is the caller's
    min(lam, lam * num_batch / warmup) (model.py:329); conf=None means 2 / C (model.py:328); kind "kl" or "l2" is
    args.loss.  With inputs_are_log_probs the logits are taken as log-probabilities (no log_softmax) and the gradient is
    with respect to them.

    parts: 0-dim device tensors "sup" (L_sup), "con" (L_con, unweighted), "n_conf", "n_valid", "n_correct" (the last
    sample's correct labelled rows, what model.py:333's accuracy counts) and "n_bad_labels".  validate=True reads
    n_bad_labels back (one host synchronisation) and raises IndexError when a label is outside [0, C).
    """
    if kind not in _KINDS:
        raise ValueError(f"kind must be 'kl' or 'l2', got {kind!r}")
    z = logits if isinstance(logits, torch.Tensor) else torch.stack(list(logits))
    if not z.is_cuda:
        raise TypeError("grand_plus_loss runs on the GPU only: logits must be CUDA tensors (no CPU fallback)")
    if z.dtype != torch.float32 or z.dim() != 3:
        raise TypeError("logits must be float32 [S, B, C] (or S tensors [B, C])")
    z = z.contiguous()
    S, B, C = z.shape
    if not 1 <= S <= _native.GP_MAX_SAMPLES:
        raise ValueError(f"the number of samples must be in [1, {_native.GP_MAX_SAMPLES}], got {S}")
    n_labeled = int(n_labeled)
    if not 0 <= n_labeled <= B:
        raise ValueError(f"n_labeled must be in [0, {B}], got {n_labeled}")
    if n_labeled > 0:
        if not isinstance(labels, torch.Tensor) or not labels.is_cuda or labels.dtype != torch.int64:
            raise TypeError("labels must be an int64 CUDA tensor")
        if labels.numel() < n_labeled:
            raise ValueError(f"labels has {labels.numel()} entries, n_labeled is {n_labeled}")
        labels = labels.reshape(-1)[:n_labeled].contiguous()
    else:
        labels = None
    if not float(tem) > 0.0:
        raise ValueError(f"tem must be > 0, got {tem!r}")
    conf = 2.0 / C if conf is None else float(conf)
    args = (n_labeled, float(weight), float(tem), conf, _KINDS[kind], int(ignore_index), bool(inputs_are_log_probs))
    if torch.is_grad_enabled() and z.requires_grad:
        loss, l_sup, l_con, counts = _LossFn.apply(z, labels, *args)
    else:
        out, counts = _loss_call(z, labels, *args)
        loss, l_sup, l_con = out[0], out[1], out[2]
    parts = {"sup": l_sup, "con": l_con, "n_conf": counts[0], "n_valid": counts[1], "n_correct": counts[2],
             "n_bad_labels": counts[3]}
    if validate:
        n_bad = int(counts[3].item())
        if n_bad:
            raise IndexError(f"{n_bad} label(s) outside [0, {C}) (other than ignore_index {ignore_index})")
    return loss, parts


def consis_loss(logps, tem, conf, loss="l2"):
    """Drop-in for the reference's `consis_loss(args, logps, tem, conf)` (model.py:123-139) with args.loss = `loss`:
    logps is a sequence of S [B, C] log-probability tensors (or an [S, B, C] tensor).  Returns a 0-dim device tensor."""
    _, parts = grand_plus_loss(logps, None, 0, 1.0, tem=tem, conf=conf, kind=loss, inputs_are_log_probs=True)
    return parts["con"]
