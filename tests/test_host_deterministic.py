"""CPU tests of the deterministic scatter backwards: the two entry points refuse bad arguments before any
device call, the `deterministic` keyword refuses anything but None or a bool before any CUDA work, the sorted orders are
what the contract says, and the float32 order pin the GPU test relies on tells a left-to-right sum from a correctly
rounded one."""
import ctypes

import numpy as np
import pytest
import torch

from grand_plus_amd import _native

P = ctypes.c_void_p(16)
SEED = ctypes.c_uint64(1)
E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK


def _rows(g=P, B=4, F=8, col=P, val=P, filled=P, K=16, rows=P, S=2, rate=0.5, keep=None, stride=64, gx=P, n_nodes=10,
          order=P, keys=P, n_sorted=64, inv=P):
    return _native.lib().gp_random_prop_rows_backward_det(0, g, B, F, col, val, filled, K, rows, S, rate, 1, SEED, keep, stride, gx,
                                                          n_nodes, order, keys, n_sorted, inv, None)


def test_rows_entry_refuses_before_any_device_call():
    """No device pointer here is real: every call has to stop at its argument checks."""
    assert _rows(K=0) == E and _rows(K=1025) == E
    assert "gp_random_prop_rows_backward_det" in _native.lib().gp_last_error().decode()
    assert _rows(S=0) == E and _rows(S=17) == E
    assert _rows(rate=-0.1) == E and _rows(rate=1.5) == E and _rows(rate=float("nan")) == E
    assert _rows(B=-1) == E and _rows(F=0) == E and _rows(n_nodes=0) == E and _rows(n_sorted=-1) == E
    assert _rows(keep=P, stride=0) == E
    for name in ("g", "col", "val", "gx", "order", "keys", "inv"):
        assert _rows(**{name: None}) == N, name
    assert "gp_random_prop_rows_backward_det" in _native.lib().gp_last_error().decode()
    assert _rows(B=0, g=None, gx=None) == OK and _rows(n_sorted=0, order=None, keys=None) == OK    # nothing to do


def _bag(g=P, V=100, H=64, offsets=P, n_src=10, nodes=None, base=None, n_rows=10, idx=P, idx_bytes=8, data=P, rate=0.5,
         dW=P, order=P, keys=P, srows=P, n_sorted=64, inv=P):
    return _native.lib().gp_embedding_bag_backward_det(0, g, V, H, offsets, n_src, nodes, base, n_rows, idx, idx_bytes, data, rate, 1,
                                                       SEED, None, dW, None, order, keys, srows, n_sorted, inv, None)


def test_bag_entry_refuses_before_any_device_call():
    assert _bag(H=0) == E and _bag(V=-1) == E and _bag(n_rows=-1) == E and _bag(n_src=-1) == E and _bag(n_sorted=-1) == E
    assert _bag(idx_bytes=2) == E and _bag(idx_bytes=0) == E
    assert _bag(rate=1.5) == E and _bag(rate=-0.5) == E and _bag(rate=float("nan")) == E
    assert "gp_embedding_bag_backward_det" in _native.lib().gp_last_error().decode()
    for name in ("g", "offsets", "idx", "data", "dW", "order", "keys", "srows", "inv"):
        assert _bag(**{name: None}) == N, name
    assert "gp_embedding_bag_backward_det" in _native.lib().gp_last_error().decode()
    assert _bag(n_rows=0, g=None, offsets=None, idx=None, data=None, dW=None, order=None, keys=None, srows=None, inv=None) == OK


def test_deterministic_must_be_none_or_a_bool(monkeypatch):
    """Refused first: before the tensors are looked at, the library is loaded or any CUDA work starts."""
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    from grand_plus_amd.mlp import MagMLP
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    monkeypatch.setattr(torch.cuda, "_lazy_init", lambda: pytest.fail("CUDA was initialised"))
    W = torch.zeros((4, 2), requires_grad=True)
    i64, f32 = torch.zeros(3, dtype=torch.int64), torch.ones(3)
    m = MagMLP(4, 2, 2, 2, False, 0.0, 0.0, False)
    for bad in ("yes", 1, 0, 1.0, "True"):
        with pytest.raises(TypeError, match="deterministic must be None, True or False"):
            random_prop_rows(W, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), None, 2, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic must be None, True or False"):
            embedding_bag(W, i64, i64, f32, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic must be None, True or False"):
            embedding_bag_csr(W, i64, i64.int(), f32, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic must be None, True or False"):
            m.emb(i64, i64, f32, deterministic=bad)
        with pytest.raises(TypeError, match="deterministic must be None, True or False"):
            m.emb_csr(i64, i64.int(), f32, deterministic=bad)
    for good in (None, True, False):                                     # accepted: the next refusal is the CPU tensor's
        with pytest.raises(TypeError, match="CUDA tensor"):
            embedding_bag(W, i64, i64, f32, deterministic=good)


def test_none_follows_torchs_global_flag():
    from grand_plus_amd._common import _deterministic
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        assert _deterministic(None) is True and _deterministic(False) is False
        torch.use_deterministic_algorithms(False)
        assert _deterministic(None) is False and _deterministic(True) is True
    finally:
        torch.use_deterministic_algorithms(was)


def test_sorted_orders_are_the_contracts():
    """The index plumbing on CPU tensors against a brute-force enumeration: stable by destination, unfilled / out-of-range /
    out-of-bag entries at the sentinel, a batch row named twice contributes twice."""
    from grand_plus_amd.augment import _rows_det_order
    from grand_plus_amd.embedding import _det_order, _Layout
    g = torch.Generator().manual_seed(0)
    K, N = 4, 8
    col = torch.randint(-1, N + 1, (6 * K,), generator=g, dtype=torch.int32)
    filled = torch.tensor([4, 0, 2, 5, 1, 3], dtype=torch.int32)
    rows = torch.tensor([5, 0, 0, 3], dtype=torch.int32)
    order, keys = _rows_det_order(col, filled, K, rows, N)
    want = sorted(((int(col[r * K + k]) if k < min(int(filled[r]), K) and 0 <= int(col[r * K + k]) < N else N, b * K + k)
                   for b, r in enumerate(rows.tolist()) for k in range(K)))
    assert [w[1] for w in want] == order.tolist() and [w[0] for w in want] == keys.tolist()
    order, keys = _rows_det_order(col, None, K, None, N)                 # every slot of every row
    assert keys.tolist() == sorted(keys.tolist()) and sorted(order.tolist()) == list(range(6 * K))
    n, V = 30, 11
    lens = torch.randint(0, 5, (n,), generator=g)
    ip = torch.zeros(n + 1, dtype=torch.int64); ip[1:] = lens.cumsum(0)
    ix = torch.randint(-1, V + 1, (int(ip[-1]),), generator=g, dtype=torch.int32)
    nodes = torch.tensor([3, 3, -1, 29, n, 0, 7, 7, 12])
    inside = (nodes >= 0) & (nodes < n)
    nc = nodes.clamp(0, n - 1)
    ln = torch.where(inside, ip[nc + 1] - ip[nc], torch.zeros_like(nc))
    L = _Layout(ip, n, nodes, ln.cumsum(0) - ln, nodes.numel(), ix, None)
    order, keys, srows = _det_order(L, int(ln.sum()), V)
    want, j = [], 0
    for m, nd in enumerate(nodes.tolist()):
        for t in range(int(ip[nd]), int(ip[nd + 1])) if 0 <= nd < n else ():
            want.append((int(ix[t]) if 0 <= int(ix[t]) < V else V, j, m)); j += 1
    want.sort()
    assert [w[1] for w in want] == order.tolist() and [w[0] for w in want] == keys.tolist() and [w[2] for w in want] == srows.tolist()
    L = _Layout(ip, n, None, None, n, ix, None)                         # nodes=None: entry number = storage position
    order, keys, srows = _det_order(L, ix.numel(), V)
    want = sorted((int(ix[t]) if 0 <= int(ix[t]) < V else V, t, int(np.searchsorted(ip.numpy(), t, side="right")) - 1) for t in range(ix.numel()))
    assert [w[1] for w in want] == order.tolist() and [w[2] for w in want] == srows.tolist()


@pytest.mark.parametrize("L", [3, 65])
def test_the_order_pin_tells_orders_apart(L):
    """The GPU pin's expectation: over g = [2^25, 1, -2^25, 1, ...] a float32 left-to-right sum loses every 1 that meets
    2^25, so it differs from the correctly rounded sum."""
    from test_gpu_deterministic_backward import PATTERN, _left_to_right
    g = np.array([PATTERN[b % 4] for b in range(L)], np.float32)[:, None]
    forward = _left_to_right(g)[0]
    exact = np.float32(g.astype(np.float64).sum())
    assert forward.dtype == np.float32 and forward == {3: 0.0, 65: 2.0 ** 25}[L]
    assert exact == {3: 1.0, 65: 2.0 ** 25 + 32}[L] and forward != exact
