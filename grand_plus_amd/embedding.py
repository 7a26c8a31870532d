"""MAG's sparse first layer (`MLP.emb`, reference model_mag.py:48-55) on MI355X -- DESIGN.md §7d.

    feat_embeds = dropout(W[attr_idx], input_droprate)                      (model_mag.py:49-50)
    out = scatter_sum(feat_embeds * attr_data[:, None], node_idx)
          / (scatter_sum(attr_data[:, None], node_idx) + 1e-10)              (model_mag.py:51-54)

over the HIP kernels of csrc/augment.hip (forward: one gather kernel; backward: fp32 atomic adds into a
dense, zeroed dW, as `nn.Embedding(sparse=False)` gives the reference's Adam).  Two input forms:

  * `embedding_bag`      -- the reference's own arguments (COO of `features[neighbor_idx].nonzero()`);
  * `embedding_bag_csr`  -- the node-attribute matrix resident on the GPU, bags named by node id: the
                            per-step scipy slicing, `.nonzero()`, upload and host-side lookup of
                            model_mag.py:339-347 disappear.

Both key the dropout of element (j, h) as (seed, j*H + h), j = the entry's position in the batch's entry
order, so the two forms give bitwise-equal outputs for the same seed.  `flatten_rows` turns the GFPush rows
of a batch into the (neighbour nodes, scores, segment ids) the two consumers take.

Gradients flow to `weight` only (attr_data and scores are constants, as in the reference).  The backward's
fp32 atomic sums depend on arrival order: `weight.grad` is not bitwise reproducible from run to run unless
`deterministic=True`, which sorts the batch's entries by attribute id and sums each row of dW in a fixed order with
plain stores (csrc/scatter_det.hip).  The flag chooses the backward alone: the forward is the same bit for
bit.  None follows `torch.are_deterministic_algorithms_enabled()`.
"""
from __future__ import annotations

import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _native
from ._common import _check, _deterministic, _dev_index, _new_seed, _ptr, _stream


class _Layout:
    """Bag layout of one call: offsets (+ optional nodes / entry bases) over (attr_idx, attr_data)."""

    def __init__(self, offsets, n_src, nodes, base, n_rows, attr_idx, attr_data):
        self.offsets, self.n_src, self.nodes, self.base, self.n_rows = offsets, n_src, nodes, base, n_rows
        self.attr_idx, self.attr_data = attr_idx, attr_data

    def tensors(self):
        return (self.offsets, self.nodes, self.base, self.attr_idx, self.attr_data)

    def args(self):
        return (_ptr(self.offsets), self.n_src, _ptr(self.nodes), _ptr(self.base), self.n_rows,
                self.attr_idx.data_ptr(), self.attr_idx.element_size(), self.attr_data.data_ptr())


def _forward(weight, L, p, training, seed, keep, n_bad):
    V, H = weight.shape
    out = torch.empty((L.n_rows, H), dtype=torch.float32, device=weight.device)
    rc = _native.lib().gp_embedding_bag(
        _dev_index(weight), weight.data_ptr(), V, H, *L.args(), float(p), int(bool(training)), ctypes.c_uint64(seed),
        _ptr(keep), out.data_ptr(), n_bad.data_ptr(), _stream(weight))
    _native.raise_for_status(rc)
    return out


def _backward(weight_shape, grad_out, L, p, training, seed, keep):
    V, H = weight_shape
    g = grad_out.contiguous()
    dW = torch.zeros((V, H), dtype=torch.float32, device=g.device)
    rc = _native.lib().gp_embedding_bag_backward(
        _dev_index(g), g.data_ptr(), V, H, *L.args(), float(p), int(bool(training)), ctypes.c_uint64(seed),
        _ptr(keep), dW.data_ptr(), None, _stream(g))
    _native.raise_for_status(rc)
    return dW


def _det_order(L, n_entries, V):
    """The sorted order the deterministic backward takes: (order, keys, rows).  Entry j < n_entries, in the batch's entry
    order, lies in output row m = the first row whose bag ends after j (an empty bag ends where it starts: skipped) at
    storage position t; its key is its attribute id, or the sentinel V when the id lies outside [0, V) or the entry
    outside its bag, so that it sorts last.  A stable sort by key: order = the entry numbers j, keys ascending, rows =
    m of each sorted entry.  Device ops only: nothing here reads the host."""
    nnz = L.attr_idx.numel()
    if L.nodes is None:
        inside = None
        starts = first = L.offsets[:-1]                                  # storage position = entry number
        ends = L.offsets[1:]
    else:
        inside = (L.nodes >= 0) & (L.nodes < L.n_src)
        src = L.nodes.clamp(0, max(L.n_src - 1, 0))
        starts = L.offsets[src]                                          # storage position of the bag's first entry
        first = L.base                                                   # its entry number
        ends = first + torch.where(inside, L.offsets[src + 1] - starts, torch.zeros_like(starts))
    j = torch.arange(n_entries, dtype=torch.int64, device=L.attr_idx.device)
    m = torch.searchsorted(ends, j, right=True)
    live = m < L.n_rows
    m = m.clamp(max=L.n_rows - 1)
    t = starts[m] + (j - first[m])
    live &= (j >= first[m]) & (t >= 0) & (t < nnz)
    if inside is not None:
        live &= inside[m]
    a = L.attr_idx[t.clamp(0, nnz - 1)].long()
    keys, order = torch.sort(torch.where(live & (a >= 0) & (a < V), a, V), stable=True)
    return order, keys, m[order]


def _backward_det(weight_shape, grad_out, L, n_entries, p, training, seed, keep, segment_chunk=None):
    """_backward without atomics (csrc/scatter_det.hip): the entries ordered by attribute id (_det_order), one
    gather kernel that sums each row of dW in that order.  segment_chunk = C: the chunked gather of DESIGN §7w over the
    same order, two kernels and a scratch."""
    V, H = weight_shape
    g = grad_out.contiguous()
    dW = torch.zeros((V, H), dtype=torch.float32, device=g.device)
    if L.n_rows == 0 or n_entries == 0 or L.attr_idx.numel() == 0:
        return dW
    order, keys, rows = _det_order(L, n_entries, V)
    inv_den = torch.empty(_native.scatter_bag_workspace_bytes(L.n_rows) // 4, dtype=torch.float32, device=g.device)
    args = (_dev_index(g), g.data_ptr(), V, H, *L.args(), float(p), int(bool(training)), ctypes.c_uint64(seed),
            _ptr(keep), dW.data_ptr(), None, order.data_ptr(), keys.data_ptr(), rows.data_ptr(), order.numel(),
            inv_den.data_ptr())
    if segment_chunk is None:
        rc = _native.lib().gp_embedding_bag_backward_det(*args, _stream(g))
    else:
        from . import gather_chunk
        scratch, nbytes = gather_chunk.scratch(order.numel(), segment_chunk, H, g.device)
        rc = _native.lib().gp_embedding_bag_backward_det_chunked(*args, segment_chunk, scratch.data_ptr(), nbytes, _stream(g))
    _native.raise_for_status(rc)
    return dW


class _BagFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, L, p, training, seed, keep, n_bad, det_entries=None, segment_chunk=None):
        ctx.save_for_backward(*L.tensors(), keep)
        ctx.args = (weight.shape, L.n_src, L.n_rows, p, training, seed)
        ctx.det_entries = det_entries                                   # None: the atomic backward; else the entry count
        ctx.segment_chunk = segment_chunk                               # the deterministic backward's chunk
        return _forward(weight, L, p, training, seed, keep, n_bad)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        offsets, nodes, base, attr_idx, attr_data, keep = ctx.saved_tensors
        shape, n_src, n_rows, p, training, seed = ctx.args
        L = _Layout(offsets, n_src, nodes, base, n_rows, attr_idx, attr_data)
        if ctx.det_entries is None:
            dW = _backward(shape, grad_out, L, p, training, seed, keep)
        else:
            dW = _backward_det(shape, grad_out, L, ctx.det_entries, p, training, seed, keep, ctx.segment_chunk)
        return dW, None, None, None, None, None, None, None, None


def _run(weight, L, n_entries, input_droprate, training, seed, keep, validate, det_entries=None, segment_chunk=None):
    """det_entries: None for the atomic backward, else a callable that gives the number of entries the deterministic
    backward sorts (called only when the gradient is wanted).  segment_chunk: that backward's chunk, or None."""
    _check(weight, torch.float32, "weight")
    if weight.dim() != 2:
        raise TypeError("weight must be a 2-D [V, H] table")
    if not 0.0 <= float(input_droprate) <= 1.0:
        raise ValueError("input_droprate must lie in [0, 1]")
    if keep is not None:
        _check(keep, torch.uint8, "keep")
        if training and keep.numel() != n_entries() * weight.shape[1]:
            raise ValueError("keep must hold one byte per (entry, column): [nnz * H]")
    if seed is None:
        seed = _new_seed()
    n_bad = torch.zeros(1, dtype=torch.int32, device=weight.device)
    if torch.is_grad_enabled() and weight.requires_grad:
        out = _BagFn.apply(weight, L, float(input_droprate), bool(training), seed, keep, n_bad,
                           det_entries() if det_entries is not None else None, segment_chunk)
    else:
        out = _forward(weight, L, input_droprate, training, seed, keep, n_bad)
    if validate:
        bad = int(n_bad.item())
        if bad:
            raise IndexError(f"embedding_bag: {bad} attribute id(s) outside [0, {weight.shape[0]}) or node id(s) out of range")
    return out


def embedding_bag(weight, attr_idx, node_idx, attr_data, input_droprate=0.0, training=True, seed=None, keep=None,
                  validate=True, deterministic=None, n_out=None, segment_chunk=None):
    """Drop-in for `MLP.emb(attr_idx, node_idx, attr_data)` (model_mag.py:48-55) on CUDA tensors.

    weight [V, H] float32 (the `nn.Embedding` table, on the GPU); attr_idx [nnz] int64; node_idx [nnz] int64
    sorted ascending (the row order of scipy's `.nonzero()`); attr_data [nnz] float32.  Returns
    [node_idx[-1] + 1, H] float32; rows with an empty bag are zeros.  `keep` [nnz * H] uint8 replaces the
    internal dropout RNG (parity tests).  validate=True raises IndexError when an id lies outside [0, V)
    (one host synchronisation); with validate=False such ids are skipped, never read or written.
    `deterministic` (None = torch.are_deterministic_algorithms_enabled()) chooses the backward: see the module docstring.
    `n_out` (optional) is the number of output rows; given, it saves the host read of node_idx[-1] (as random_prop's).
    `segment_chunk` = C (a power of two in [64, 4096]; None: off) cuts the deterministic backward's sums into chunks of C
    entries (gather_chunk.py): a hub attribute is no longer one serial chain.  ValueError with the atomic backward.
    """
    deterministic = _deterministic(deterministic)
    from .gather_chunk import resolve
    segment_chunk = resolve(segment_chunk, deterministic, "embedding_bag")
    _check(attr_idx, torch.int64, "attr_idx")
    _check(node_idx, torch.int64, "node_idx")
    _check(attr_data, torch.float32, "attr_data")
    nnz = attr_idx.numel()
    if node_idx.numel() != nnz or attr_data.numel() != nnz:
        raise ValueError("attr_idx, node_idx and attr_data must have the same number of entries")
    if nnz == 0:
        _check(weight, torch.float32, "weight")
        return weight.new_zeros((0, weight.shape[1]))
    if n_out is None:
        n_out = int(node_idx[-1].item()) + 1                             # model_mag.py:51 dim_size
    elif int(n_out) < 1:
        raise ValueError("n_out must be >= 1")
    n_out = int(n_out)
    offsets = torch.searchsorted(node_idx, torch.arange(n_out + 1, dtype=torch.int64, device=node_idx.device))
    L = _Layout(offsets, n_out, None, None, n_out, attr_idx, attr_data)
    return _run(weight, L, lambda: nnz, input_droprate, training, seed, keep, validate, (lambda: nnz) if deterministic else None,
                segment_chunk)


def embedding_bag_csr(weight, attr_indptr, attr_indices, attr_data, nodes=None, input_droprate=0.0, training=True,
                      seed=None, keep=None, validate=True, deterministic=None, segment_chunk=None):
    """`MLP.emb` over the bags of `nodes` in a node-attribute CSR resident on the GPU.

    attr_indptr [N + 1] int64, attr_indices [nnz] int32, attr_data [nnz] float32 (the scipy CSR's arrays);
    nodes [B] int64 (None = every node: `predict`'s emb pass, model_mag.py:197-205).  Returns [B, H] float32,
    row m built from the bag of node nodes[m].  Equals `embedding_bag` on `features[nodes].nonzero()`
    bitwise for the same seed (same entry order, same dropout keys).  Replaces the slicing, `.nonzero()`,
    upload and host-side lookup of model_mag.py:339-347.
    `deterministic` (None = torch.are_deterministic_algorithms_enabled()) chooses the backward: see the module docstring.
    With `nodes` given the number of entries of the batch is data-dependent, and the deterministic backward needs it as
    a host number to size its sort: that one count is read back here, in the forward call (one host synchronisation;
    only when the gradient is wanted).  With nodes=None the count is `attr_indices.numel()`: no host read.
    `segment_chunk`: as `embedding_bag`'s.
    """
    deterministic = _deterministic(deterministic)
    from .gather_chunk import resolve
    segment_chunk = resolve(segment_chunk, deterministic, "embedding_bag_csr")
    _check(attr_indptr, torch.int64, "attr_indptr")
    _check(attr_indices, torch.int32, "attr_indices")
    _check(attr_data, torch.float32, "attr_data")
    N = attr_indptr.numel() - 1
    if N < 0 or attr_data.numel() != attr_indices.numel():
        raise ValueError("attr_indptr needs N + 1 entries; attr_indices and attr_data the same length")
    if nodes is None:
        L = _Layout(attr_indptr, N, None, None, N, attr_indices, attr_data)
        n_entries = lambda: int(attr_indptr[-1].item())                 # noqa: E731  (j = storage position)
        det_entries = attr_indices.numel                                # every stored entry is sorted: no host read
    else:
        _check(nodes, torch.int64, "nodes")
        inside = (nodes >= 0) & (nodes < N)
        nc = nodes.clamp(0, max(N - 1, 0))
        lens = torch.where(inside, attr_indptr[nc + 1] - attr_indptr[nc], torch.zeros_like(nc)) if N > 0 else torch.zeros_like(nodes)
        base = torch.cumsum(lens, 0) - lens                            # entry order: the bags one after another
        L = _Layout(attr_indptr, N, nodes, base, nodes.numel(), attr_indices, attr_data)
        n_entries = det_entries = lambda: int(lens.sum().item())       # noqa: E731
    return _run(weight, L, n_entries, input_droprate, training, seed, keep, validate, det_entries if deterministic else None,
                segment_chunk)


def flatten_rows(col, val, filled, K, batch_rows):
    """The GFPush rows of one batch as the reference's COO (model_mag.py:339-343), without leaving the GPU.

    col int32 [S*K], val float64 [S*K], filled int32 [S] (`Graph.gfpush_device`), batch_rows int32 / int64 [B]
    (positions of the batch's seeds in the seed list).  Returns (neighbor_nodes int64, scores float32,
    mat_idx int64) in row-major batch order; within a row, slot order (value descending), where the
    reference's `topk_adj.tocsr()` sorts columns ascending -- only the fp32 summation order and which mask
    element lands on which entry differ.  The output length is data-dependent: one count is read back.
    """
    _check(col, torch.int32, "col")
    _check(val, torch.float64, "val")
    _check(filled, torch.int32, "filled")
    if not isinstance(batch_rows, torch.Tensor) or not batch_rows.is_cuda or batch_rows.dtype not in (torch.int32, torch.int64):
        raise TypeError("batch_rows must be an int32 or int64 CUDA tensor")
    K = int(K)
    rows = batch_rows.long()
    B = rows.numel()
    live = torch.arange(K, device=col.device)[None, :] < filled[rows].clamp(max=K)[:, None]
    neighbor_nodes = col.view(-1, K)[rows][live].long()
    scores = val.view(-1, K)[rows][live].to(torch.float32)             # torch.tensor(mat_scores, float32), model_mag.py:343
    mat_idx = torch.arange(B, device=col.device)[:, None].expand(B, K)[live]
    return neighbor_nodes, scores, mat_idx
