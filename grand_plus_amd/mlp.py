"""GRAND+'s MLP on MI355X: all S samples of a training step through each layer in one set of HIP launches.

Reference `MLP.forward` (model.py:48-66, model_mag.py:57-67), called once per sample there.  Every layer is the block

    block(x) = Linear( dropout_p( BN( node_norm( relu?(x) ) ) ) ),      node_norm(u) = u / (1e-12 + |u|_2)

run by `gp_mlp_block_forward` / `gp_mlp_block_backward` of csrc/mlp.hip over x [S, B, F] (what
`random_prop*(samples=S)` returns).  BatchNorm in training takes each sample's own batch statistics and updates the
running statistics once per sample in sample order, exactly as S calls of `bn(x)`.

  * `GrandPlusMLP` -- model.py's layout (layer 0: no ReLU, node_norm with `.detach()`, `bns[0]`, `input_droprate`);
  * `MagMLP`       -- model_mag.py's layout (`embeds`, then "ReLU, node_norm, BN, hidden_droprate, fc" per layer).

Both keep the reference's submodules (`fcs`, `bns`, `embeds`), so a `state_dict` loads in either direction.  Dropout of
layer l, sample s, entry b * F + f uses the counter hash on `layer_seed(seed, l, s)` (grandplus.h), or an explicit uint8
keep mask per layer.  Calls without grad (eval, `torch.no_grad`) run the forward kernels only.  There is no fallback:
`reference_forward` is the torch formulation kept for comparison and benchmarks, never taken silently.

`infer` is the eval-only forward over any number of rows: `gp_mlp_infer_block` of csrc/mlp_infer.hip per
layer, on a GEMM tiled for millions of rows; it is opt-in and leaves `forward` as it is.  `infer(fused=True)` runs the
last two blocks as one kernel, `gp_mlp_infer_chain2` of csrc/mlp_chain.hip: the hidden activations stay in
LDS, and the result has the bits of the unfused path.
"""
from __future__ import annotations

import ctypes

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import _native
from ._common import _M64, _new_seed, _ptr, _stream, layer_seed  # noqa: F401  (layer_seed: public here)


class _Cfg:
    """The non-tensor arguments of one block call."""
    __slots__ = ("flags", "bn", "p", "seed", "layer", "keep")

    def __init__(self, flags, bn, p, seed, layer, keep):
        self.flags, self.bn, self.p, self.seed, self.layer, self.keep = flags, bn, p, seed, layer, keep


def _forward(x, weight, bias, gamma, beta, c, save_a):
    S, B, F = x.shape
    N = weight.shape[0]
    # tests/test_gpu_mlp_block.py names these allocations by their order (out, saved, a, workspace): keep its list in step
    out = torch.empty((S, B, N), dtype=torch.float32, device=x.device)
    saved = None
    if c.flags & (_native.GP_MLP_NORM | _native.GP_MLP_BN):
        saved = torch.empty(_native.mlp_saved_floats(S, B, F), dtype=torch.float32, device=x.device)
    a = torch.empty_like(x) if save_a else None
    ws = torch.empty(_native.mlp_forward_workspace_bytes(S), dtype=torch.uint8, device=x.device)
    bn = c.bn
    rm = bn.running_mean if bn is not None else None
    rv = bn.running_var if bn is not None else None
    nbt = bn.num_batches_tracked if bn is not None and c.flags & _native.GP_MLP_TRAINING else None
    rc = _native.lib().gp_mlp_block_forward(
        x.device.index, x.data_ptr(), S, B, F, N, weight.data_ptr(), _ptr(bias), c.flags, _ptr(gamma), _ptr(beta),
        _ptr(rm), _ptr(rv), _ptr(nbt), float(bn.eps) if bn is not None else 1e-5,
        float(bn.momentum) if bn is not None else 0.1, float(c.p), ctypes.c_uint64(c.seed), c.layer, _ptr(c.keep),
        out.data_ptr(), _ptr(saved), _ptr(a), ws.data_ptr(), _stream(x))
    _native.raise_for_status(rc)
    return out, saved, a


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, c):
        out, saved, a = _forward(x, weight, bias, gamma, beta, c, save_a=ctx.needs_input_grad[1])
        ctx.save_for_backward(x, weight, gamma, saved, a)
        ctx.c = c
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, weight, gamma, saved, a = ctx.saved_tensors
        c = ctx.c
        S, B, F = x.shape
        N = weight.shape[0]
        gy = gy.contiguous()
        nx, nw, nb, ng, nbe = ctx.needs_input_grad[:5]
        # ... and these (gx, gw, gb, gg, gbe, workspace)
        new = lambda need, shape: torch.empty(shape, dtype=torch.float32, device=x.device) if need else None  # noqa: E731
        gx, gw, gb = new(nx, x.shape), new(nw, weight.shape), new(nb, (N,))
        gg = new(ng and gamma is not None, (F,))
        gbe = new(nbe, (F,))
        ws = torch.empty(_native.mlp_backward_workspace_bytes(S, B, F), dtype=torch.uint8, device=x.device)
        rc = _native.lib().gp_mlp_block_backward(
            x.device.index, x.data_ptr(), S, B, F, N, weight.data_ptr(), c.flags, _ptr(gamma), float(c.p),
            ctypes.c_uint64(c.seed), c.layer, _ptr(c.keep), _ptr(saved), _ptr(a), gy.data_ptr(), _ptr(gx), _ptr(gw),
            _ptr(gb), _ptr(gg), _ptr(gbe), ws.data_ptr(), _stream(x))
        _native.raise_for_status(rc)
        return gx, gw, gb, gg, gbe, None


def _check_bn(bn):
    if bn.momentum is None:
        raise ValueError("BatchNorm1d with momentum=None (cumulative average) is not supported; the reference uses 0.1")
    if not bn.track_running_stats or bn.running_mean is None:
        raise ValueError("BatchNorm1d without running statistics is not supported (the reference tracks them)")


def _check_layout(X, ranks, shapes, contiguous):
    """What the kernels assume of an input they take by raw pointer: a float32 tensor of one of `ranks`, contiguous."""
    if not isinstance(X, torch.Tensor):
        raise ValueError("X must be a tensor")
    if X.dtype != torch.float32:
        raise ValueError(f"X must be float32, got {X.dtype}")
    if X.dim() not in ranks:
        raise ValueError(f"X must be {shapes}, got {tuple(X.shape)}")
    if not X.is_contiguous():
        raise ValueError(contiguous)


def _check_samples(S, B):
    if not 1 <= S <= _native.GP_MAX_SAMPLES:
        raise ValueError(f"the number of samples must be in [1, {_native.GP_MAX_SAMPLES}], got {S}")
    if B < 1:
        raise ValueError("X has no rows")


def _check_cuda(X):
    if not X.is_cuda:
        raise ValueError("the MLP runs on the GPU only: X must be a CUDA tensor (no CPU fallback)")


def block(x, fc, bn, *, relu, node_norm, training, dropout, seed, layer, keep=None):
    """One block on x [S, B, F] (contiguous float32 CUDA): Linear(dropout(BN(node_norm(relu?(x))))).  bn None = no
    BatchNorm.  Differentiable with respect to x, fc's and bn's parameters; running statistics update in training.
    Anything else for x is a ValueError before the first launch (the kernels take x by raw pointer); the CPU-tensor
    check comes last, as in _check_input."""
    _check_layout(x, (3,), "[S, B, F]", "X must be contiguous (what random_prop*(samples=S) returns)")
    S, B, F = x.shape
    _check_samples(S, B)
    flags = (_native.GP_MLP_RELU if relu else 0) | (_native.GP_MLP_NORM if node_norm else 0) | \
            (_native.GP_MLP_BN if bn is not None else 0) | (_native.GP_MLP_TRAINING if training else 0)
    if fc.weight.shape[1] != F:
        raise ValueError(f"the layer takes {fc.weight.shape[1]} features, the input has {F}")
    for name, t in (("weight", fc.weight), ("bias", fc.bias)) + ((("bn weight", bn.weight), ("bn bias", bn.bias),
                                                                   ("running_mean", bn.running_mean),
                                                                   ("running_var", bn.running_var)) if bn is not None else ()):
        if t is not None and (t.dtype != torch.float32 or t.device != x.device or not t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32 tensor on {x.device}")
    if bn is not None:
        _check_bn(bn)
        if bn.num_features != F:
            raise ValueError(f"BatchNorm1d has {bn.num_features} features, the input has {F}")
        if training and B < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, F]}")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.uint8 or keep.device != x.device or not keep.is_contiguous():
            raise ValueError("keep must be a contiguous uint8 tensor on the input's device")
        if keep.numel() != S * B * F:
            raise ValueError(f"keep must hold S x B x F = {S * B * F} entries, got {keep.numel()}")
    _check_cuda(x)
    c = _Cfg(flags, bn, float(dropout), int(seed) & _M64, int(layer), keep if training and dropout > 0 else None)
    gamma = bn.weight if bn is not None else None
    beta = bn.bias if bn is not None else None
    params = (x, fc.weight, fc.bias, gamma, beta)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in params):
        return _BlockFn.apply(x, fc.weight, fc.bias, gamma, beta, c)
    return _forward(x, fc.weight, fc.bias, gamma, beta, c, save_a=False)[0]


def _check_input(X, layers, training):
    """Every host check before the first launch: shape, dtype, layout, sample count, BatchNorm's batch size, device."""
    _check_layout(X, (2, 3), "[B, F] or [S, B, F]", "X must be contiguous (what random_prop*(samples=S) returns)")
    x = X[None] if X.dim() == 2 else X
    S, B, _ = x.shape
    _check_samples(S, B)
    for _fc, bn, *_ in layers:
        if bn is not None:
            _check_bn(bn)
            if training and B < 2:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {[B, bn.num_features]}")
    _check_cuda(X)
    if layers and layers[0][0].weight.device != X.device:
        raise ValueError(f"X is on {X.device}, the parameters on {layers[0][0].weight.device}")
    return x


def _keeps(keep, n):
    if keep is None:
        return [None] * n
    keep = list(keep)
    if len(keep) != n:
        raise ValueError(f"keep needs one mask (or None) per layer: {n}, got {len(keep)}")
    return keep


def _run(module, X, seed, keep, layers):
    """layers: (fc, bn or None, relu, node_norm, detach, dropout) per layer."""
    x = _check_input(X, layers, module.training)
    seed = _new_seed() if seed is None else int(seed)
    keeps = _keeps(keep, len(layers))
    for l, ((fc, bn, relu, norm, detach, p), k) in enumerate(zip(layers, keeps)):
        if detach:
            x = x.detach()
        x = block(x, fc, bn, relu=relu, node_norm=norm, training=module.training, dropout=p, seed=seed, layer=l, keep=k)
    return x[0] if X.dim() == 2 else x


def _torch_block(x, fc, bn, relu, norm, detach, p, training):
    import torch.nn.functional as F
    if relu:
        x = F.relu(x)
    if norm:
        x = x / (1e-12 + torch.norm(x, p=2, dim=-1, keepdim=True))
        if detach:
            x = x.detach()
    if bn is not None:
        x = bn(x)
    x = F.dropout(x, p, training=training)
    return fc(x)


def _check_infer(X, out, batch_size, layers, fused=False):
    """Every host check of `infer` before the first launch; the CPU-tensor check comes last, as in _check_input."""
    if not isinstance(X, torch.Tensor):
        raise ValueError("X must be a tensor")
    if X.dtype != torch.float32:
        raise ValueError(f"X must be float32, got {X.dtype}")
    if X.dim() != 2:
        raise ValueError(f"infer takes X [B, F] (one sample, any number of rows), got {tuple(X.shape)}")
    if not X.is_contiguous():
        raise ValueError("X must be contiguous")
    B, F = X.shape
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError(f"batch_size must be >= 1 or None, got {batch_size}")
    C = F
    for fc, bn, *_ in layers:
        if fc.weight.shape[1] != C:
            raise ValueError(f"the layer takes {fc.weight.shape[1]} features, its input has {C}")
        if bn is not None:
            _check_bn(bn)
            if bn.num_features != C:
                raise ValueError(f"BatchNorm1d has {bn.num_features} features, its input has {C}")
        for name, t in (("weight", fc.weight), ("bias", fc.bias)) + ((("bn weight", bn.weight), ("bn bias", bn.bias),
                                                                       ("running_mean", bn.running_mean),
                                                                       ("running_var", bn.running_var)) if bn is not None else ()):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous float32 tensor")
        C = fc.weight.shape[0]
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 tensor")
        if tuple(out.shape) != (B, C):
            raise ValueError(f"out must be [B, C] = {(B, C)}, got {tuple(out.shape)}")
        if out.device != X.device:
            raise ValueError(f"out must be on X's device {X.device}, got {out.device}")
    if fused:                                                # the limits of gp_mlp_infer_chain2 (grandplus_infer_chain.h)
        if len(layers) < 2:
            raise ValueError(f"infer(fused=True) fuses the last two blocks: the model has {len(layers)}, fewer than two blocks")
        hidden = layers[-1][0].weight.shape[1]
        if hidden > _native.GP_MLP_CHAIN_MAX_HIDDEN:
            raise ValueError(f"infer(fused=True) keeps the hidden tile in LDS: hidden size {hidden} is above the limit of "
                             f"{_native.GP_MLP_CHAIN_MAX_HIDDEN}")
        if C > _native.GP_MLP_CHAIN_MAX_OUT:
            raise ValueError(f"infer(fused=True): {C} classes are above the limit of {_native.GP_MLP_CHAIN_MAX_OUT}")
    if not X.is_cuda:
        raise ValueError("the MLP runs on the GPU only: X must be a CUDA tensor (no CPU fallback)")
    if layers and layers[0][0].weight.device != X.device:
        raise ValueError(f"X is on {X.device}, the parameters on {layers[0][0].weight.device}")
    return C


def _block_args(fc, bn, relu, norm):
    """A block's arguments as gp_mlp_infer_block and gp_mlp_infer_chain2 take them: weight, bias, flags, BatchNorm, eps."""
    flags = (_native.GP_MLP_RELU if relu else 0) | (_native.GP_MLP_NORM if norm else 0) | \
            (_native.GP_MLP_BN if bn is not None else 0)
    return (fc.weight.data_ptr(), _ptr(fc.bias), flags,
            _ptr(bn.weight) if bn is not None else None, _ptr(bn.bias) if bn is not None else None,
            _ptr(bn.running_mean) if bn is not None else None, _ptr(bn.running_var) if bn is not None else None,
            float(bn.eps) if bn is not None else 1e-5)


def _infer_block(x, fc, bn, relu, norm, out, ws):
    """One eval block on x [n, F] into out [n, N] (gp_mlp_infer_block); ws: the caller's scratch."""
    rc = _native.lib().gp_mlp_infer_block(
        x.device.index, x.data_ptr(), x.shape[0], x.shape[1], fc.weight.shape[0], *_block_args(fc, bn, relu, norm),
        out.data_ptr(), _ptr(ws), _stream(x))
    _native.raise_for_status(rc)


def _infer_chain2(x, first, second, out, ws):
    """Two eval blocks on x [n, F] into out [n, C] as one kernel (gp_mlp_infer_chain2); ws: the caller's scratch."""
    rc = _native.lib().gp_mlp_infer_chain2(
        x.device.index, x.data_ptr(), x.shape[0], x.shape[1], first[0].weight.shape[0], second[0].weight.shape[0],
        *_block_args(*first[:4]), *_block_args(*second[:4]), out.data_ptr(), _ptr(ws), _stream(x))
    _native.raise_for_status(rc)


class _MLPBase:
    def reset_param(self):
        for lin in self.fcs:
            lin.reset_parameters()

    def normalize(self, embedding):
        return embedding / (1e-12 + torch.norm(embedding, p=2, dim=-1, keepdim=True))

    def forward(self, X, seed=None, keep=None):
        """X [S, B, F] or [B, F] float32 CUDA, contiguous -> [S, B, C] or [B, C].  seed: the dropout seed of this call
        (None = a fresh one); keep: one uint8 [S, B, F_l] mask (or None) per layer in place of the hash."""
        return _run(self, X, seed, keep, self._layers())

    @torch.no_grad()
    def infer(self, X, out=None, batch_size=None, fused=False):
        """The model in eval semantics over any number of rows: X [B, F] float32 CUDA, contiguous (a row
        slice is fine) -> [B, C].  Running statistics, no dropout, whatever `self.training` says: the flag, the running
        statistics and num_batches_tracked are neither read nor written, and the result never requires grad.
        batch_size bounds the hidden activations: rows go through the layers that many at a time (None: all at once),
        the last layer writing straight into its row slice of the result; every row gets the same bits either way.
        out: a contiguous float32 [B, C] on X's device, written and returned.  One gp_mlp_infer_block per layer and
        chunk; no host synchronisation.
        fused=True: the last two blocks of a chunk are one gp_mlp_infer_chain2 call, their hidden activations
        stay in LDS and no [rows, hidden] tensor is allocated for them; earlier blocks run as above.  The bits are those of
        fused=False.  It needs at least two blocks, a last hidden size <= 1024 and <= 64 classes (ValueError)."""
        layers = self._layers()
        C = _check_infer(X, out, batch_size, layers, fused)
        B = X.shape[0]
        if not layers:                                       # a MagMLP that is its embedding alone
            return X if out is None else out.copy_(X)
        if out is None:
            out = torch.empty((B, C), dtype=torch.float32, device=X.device)
        step = B if batch_size is None else min(int(batch_size), B)
        if B == 0:
            return out
        single = layers[:-2] if fused else layers            # the blocks that go one gp_mlp_infer_block each
        need = any(norm or bn is not None for _fc, bn, _relu, norm, *_ in single)
        ws = torch.empty(_native.mlp_infer_workspace_bytes(step, max(fc.weight.shape[1] for fc, *_ in single)),
                         dtype=torch.uint8, device=X.device) if need else None
        if fused:
            (fc1, *_), (fc2, *_) = layers[-2:]
            ws2 = torch.empty(_native.mlp_infer_chain_workspace_bytes(step, fc1.weight.shape[1], fc2.weight.shape[1]),
                              dtype=torch.uint8, device=X.device)
        for start in range(0, B, step):
            x = X[start:start + step]
            for l, (fc, bn, relu, norm, _detach, _p) in enumerate(single):
                y = out[start:start + step] if l == len(layers) - 1 else \
                    torch.empty((x.shape[0], fc.weight.shape[0]), dtype=torch.float32, device=X.device)
                _infer_block(x, fc, bn, relu, norm, y, ws)
                x = y
            if fused:
                _infer_chain2(x, layers[-2], layers[-1], out[start:start + step], ws2)
        return out

    def reference_forward(self, X):
        """The reference's MLP.forward on one [B, F] sample with torch ops and this module's parameters (torch's own
        dropout RNG): what the benchmark compares against, called once per sample as model.py:321-325 does."""
        x = X
        for fc, bn, relu, norm, detach, p in self._layers():
            x = _torch_block(x, fc, bn, relu, norm, detach, p, self.training)
        return x


class GrandPlusMLP(_MLPBase, nn.Module):
    """model.py's `MLP` (model.py:17-66) over the HIP block kernels; same constructor, submodules and state_dict."""

    def __init__(self, num_features, num_classes, hidden_size, nlayers, use_bn, input_dropout, hidden_dropout, node_norm):
        nn.Module.__init__(self)
        if nlayers == 1:
            fcs = [nn.Linear(num_features, num_classes, bias=True)]
            bns = [nn.BatchNorm1d(num_features)]
        else:
            fcs = [nn.Linear(num_features, hidden_size, bias=True)]
            bns = [nn.BatchNorm1d(num_features)]
            for _ in range(nlayers - 2):
                fcs.append(nn.Linear(hidden_size, hidden_size, bias=True))
                bns.append(nn.BatchNorm1d(hidden_size))
            bns.append(nn.BatchNorm1d(hidden_size))
            fcs.append(nn.Linear(hidden_size, num_classes, bias=True))
        self.fcs = nn.ModuleList(fcs)
        self.bns = nn.ModuleList(bns)
        self.input_droprate = input_dropout
        self.hidden_droprate = hidden_dropout
        self.use_bn = use_bn
        self.node_norm = node_norm
        self.reset_param()

    def _layers(self):
        out = []
        for i, (fc, bn) in enumerate(zip(self.fcs, self.bns)):
            out.append((fc, bn if self.use_bn else None, i > 0, bool(self.node_norm), i == 0 and bool(self.node_norm),
                        self.input_droprate if i == 0 else self.hidden_droprate))
        return out


class MagMLP(_MLPBase, nn.Module):
    """model_mag.py's `MLP` (model_mag.py:17-67): the embedding-bag layer `emb` over embedding.py's kernels, then
    "ReLU, node_norm, BN, hidden_droprate, fc" per layer.  The gradient reaches X (and through `emb` the table)."""

    def __init__(self, num_features, num_classes, hidden_size, nlayers, use_bn, input_dropout, hidden_dropout, node_norm):
        nn.Module.__init__(self)
        if nlayers == 1:
            self.embeds = nn.Embedding(num_features, num_classes)
            self.fcs = nn.ModuleList([])
            self.bns = nn.ModuleList([])
        else:
            fcs, bns = [], []
            self.embeds = nn.Embedding(num_features, hidden_size)
            for _ in range(nlayers - 2):
                fcs.append(nn.Linear(hidden_size, hidden_size, bias=True))
                bns.append(nn.BatchNorm1d(hidden_size))
            bns.append(nn.BatchNorm1d(hidden_size))
            fcs.append(nn.Linear(hidden_size, num_classes, bias=True))
            self.fcs = nn.ModuleList(fcs)
            self.bns = nn.ModuleList(bns)
        self.input_droprate = input_dropout
        self.hidden_droprate = hidden_dropout
        self.use_bn = use_bn
        self.node_norm = node_norm
        self.reset_param()

    def emb(self, attr_idx, node_idx, attr_data, seed=None, keep=None, deterministic=None, segment_chunk=None):
        """MLP.emb (model_mag.py:48-55) through embedding.embedding_bag (the reference's COO arguments); `deterministic`
        and `segment_chunk` are passed through."""
        from .embedding import embedding_bag
        return embedding_bag(self.embeds.weight, attr_idx, node_idx, attr_data, self.input_droprate, self.training,
                             seed, keep, deterministic=deterministic, segment_chunk=segment_chunk)

    def emb_csr(self, attr_indptr, attr_indices, attr_data, nodes=None, seed=None, keep=None, deterministic=None,
                segment_chunk=None):
        """MLP.emb over the bags of `nodes` in a GPU-resident node-attribute CSR (embedding.embedding_bag_csr);
        `deterministic` and `segment_chunk` are passed through."""
        from .embedding import embedding_bag_csr
        return embedding_bag_csr(self.embeds.weight, attr_indptr, attr_indices, attr_data, nodes, self.input_droprate,
                                 self.training, seed, keep, deterministic=deterministic, segment_chunk=segment_chunk)

    def emb_rows(self, attr_indptr, attr_indices, attr_data, rows, batch_rows=None, samples=1, dropnode_rate=0.5, seed=None,
                 keep=None, deterministic=None, max_entries=None, overflow=None, row_grad=None, segment_chunk=None,
                 det_input_dropout=False):
        """MLP.emb of every neighbour of a batch of `rows` (a RowMatrix) and random_prop over them as one op
        (mag.mag_prop_rows): [B, H], or [S, B, H] for samples = S > 1, ready for `forward`.  `deterministic`,
        `max_entries` and `overflow` are passed through (the deterministic table gradient), and so is
        `row_grad` (an optim_rows.RowGrad of `embeds.weight`: the table's gradient as a row list) and
        `segment_chunk` (the deterministic gradient's hub segments in chunks).  `seed` may be an int64 [1] device
        tensor and `det_input_dropout=True` lets the deterministic gradient run with `input_droprate > 0`."""
        from .mag import mag_prop_rows
        from .rows import RowMatrix
        if not isinstance(rows, RowMatrix):
            raise TypeError("rows must be a RowMatrix")
        return mag_prop_rows(self.embeds.weight, attr_indptr, attr_indices, attr_data, rows.col, rows.val, rows.filled, rows.K,
                             batch_rows, samples=samples, dropnode_rate=dropnode_rate, input_droprate=self.input_droprate,
                             training=self.training, seed=seed, keep=keep, deterministic=deterministic, max_entries=max_entries,
                             overflow=overflow, row_grad=row_grad, segment_chunk=segment_chunk, det_input_dropout=det_input_dropout)

    def _layers(self):
        return [(fc, bn if self.use_bn else None, True, bool(self.node_norm), False, self.hidden_droprate)
                for fc, bn in zip(self.fcs, self.bns)]

    def forward(self, X, seed=None, keep=None):
        if not len(self.fcs):
            _check_input(X, [], self.training)
            return X
        return _run(self, X, seed, keep, self._layers())
