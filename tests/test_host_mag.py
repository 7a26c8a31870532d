"""CPU tests of the backward / embedding-bag entries: bad arguments are refused before any device
work, and the Python wrappers refuse CPU tensors (no CPU fallback)."""
import ctypes

import pytest

from grand_plus_amd import _native

NULL = None


def _lib():
    return _native.lib()


def test_random_prop_backward_entries_check_arguments_before_the_device():
    L = _lib()
    p, s = ctypes.c_void_p(16), ctypes.c_void_p(0)
    seed = ctypes.c_uint64(1)
    # coo: gp_random_prop_coo_backward(device, grad_out, n_out, F, scores, idx, n_entries, rate, training, seed, keep, grad_feats, stream)
    assert L.gp_random_prop_coo_backward(0, p, 4, 0, p, p, 8, 0.5, 1, seed, NULL, p, s) == _native.GP_ERR_INVALID_ARG   # F < 1
    assert L.gp_random_prop_coo_backward(0, p, 4, 8, p, p, -1, 0.5, 1, seed, NULL, p, s) == _native.GP_ERR_INVALID_ARG  # n_entries < 0
    assert L.gp_random_prop_coo_backward(0, p, 4, 8, p, p, 8, 1.5, 1, seed, NULL, p, s) == _native.GP_ERR_INVALID_ARG   # rate > 1
    assert L.gp_random_prop_coo_backward(0, NULL, 4, 8, p, p, 8, 0.5, 1, seed, NULL, p, s) == _native.GP_ERR_NULL
    assert L.gp_random_prop_coo_backward(0, p, 4, 8, p, p, 8, 0.5, 1, seed, NULL, NULL, s) == _native.GP_ERR_NULL
    assert L.gp_random_prop_coo_backward(0, NULL, 0, 8, NULL, NULL, 0, 0.5, 1, seed, NULL, NULL, s) == _native.GP_OK  # nothing to do
    # rows: (device, grad_out, n_batch, F, col, val, filled, K, batch_rows, rate, training, seed, keep, grad_x, n_nodes, stream)
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, p, p, p, 0, p, 0.5, 1, seed, NULL, p, 10, s) == _native.GP_ERR_INVALID_ARG     # K < 1
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, p, p, p, 1025, p, 0.5, 1, seed, NULL, p, 10, s) == _native.GP_ERR_INVALID_ARG  # K > 1024
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, p, p, p, 16, p, -0.1, 1, seed, NULL, p, 10, s) == _native.GP_ERR_INVALID_ARG
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, p, p, p, 16, p, 0.5, 1, seed, NULL, p, 0, s) == _native.GP_ERR_INVALID_ARG     # no nodes
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, NULL, p, p, 16, p, 0.5, 1, seed, NULL, p, 10, s) == _native.GP_ERR_NULL
    assert L.gp_random_prop_rows_backward(0, p, 4, 8, p, p, p, 16, p, 0.5, 1, seed, NULL, NULL, 10, s) == _native.GP_ERR_NULL
    assert "gp_random_prop_rows_backward" in L.gp_last_error().decode()


@pytest.mark.parametrize("name", ["gp_embedding_bag", "gp_embedding_bag_backward"])
def test_embedding_bag_entries_check_arguments_before_the_device(name):
    f = getattr(_lib(), name)
    p, s = ctypes.c_void_p(16), ctypes.c_void_p(0)
    seed = ctypes.c_uint64(1)

    def call(table=p, V=100, H=64, offsets=p, n_src=10, nodes=NULL, base=NULL, n_rows=10, idx=p, idx_bytes=8, data=p,
             rate=0.5, dst=p):
        # the forward takes (weight, ..., out); the backward (grad_out, ..., grad_weight): the table pointer and
        # the destination are the two that must not be NULL in either
        first, last = (table, dst) if name == "gp_embedding_bag" else (dst, table)
        return f(0, first, V, H, offsets, n_src, nodes, base, n_rows, idx, idx_bytes, data, rate, 1, seed, NULL, last, NULL, s)

    assert call(H=0) == _native.GP_ERR_INVALID_ARG
    assert call(V=-1) == _native.GP_ERR_INVALID_ARG
    assert call(n_rows=-1) == _native.GP_ERR_INVALID_ARG
    assert call(n_src=-1) == _native.GP_ERR_INVALID_ARG
    assert call(idx_bytes=2) == _native.GP_ERR_INVALID_ARG
    assert call(rate=1.5) == _native.GP_ERR_INVALID_ARG
    assert call(rate=float("nan")) == _native.GP_ERR_INVALID_ARG
    assert call(offsets=NULL) == _native.GP_ERR_NULL
    assert call(idx=NULL) == _native.GP_ERR_NULL
    assert call(data=NULL) == _native.GP_ERR_NULL
    assert call(table=NULL) == _native.GP_ERR_NULL
    assert call(dst=NULL) == _native.GP_ERR_NULL
    assert name in _lib().gp_last_error().decode()
    assert call(n_rows=0, offsets=NULL, idx=NULL, data=NULL, table=NULL, dst=NULL) == _native.GP_OK   # nothing to do


def test_python_wrappers_refuse_cpu_tensors():
    import torch
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr, flatten_rows
    W = torch.randn(10, 4, requires_grad=True)
    idx = torch.tensor([0, 3, 5]); node = torch.tensor([0, 0, 1]); d = torch.ones(3)
    with pytest.raises(TypeError):
        embedding_bag(W, idx, node, d)
    with pytest.raises(TypeError):
        embedding_bag_csr(W, torch.tensor([0, 2, 3]), idx.int(), d)
    with pytest.raises(TypeError):
        flatten_rows(torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.float64), torch.zeros(2, dtype=torch.int32),
                     4, torch.zeros(1, dtype=torch.int32))
    from grand_plus_amd.augment import random_prop, random_prop_rows
    feats = torch.randn(3, 4, requires_grad=True)
    with pytest.raises(TypeError):
        random_prop(feats, torch.ones(3), torch.tensor([0, 0, 1]), 0.5)
    with pytest.raises(TypeError):
        random_prop_rows(feats, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), None, 2)
