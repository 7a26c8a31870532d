"""The deterministic backwards of random_prop_rows and the embedding bag (csrc/scatter_det.hip): the order
contract pinned bit for bit against a numpy float32 left-to-right loop, the gradients against float64 (`close`:
|d| <= 1e-5 * sum|terms| + 1e-7, every destination at most 128 contributions so that the sequential-sum error
(L + 4) * 2^-24 stays below 1e-5; the hub cases, L = 4 097, under the derived bound (L + 4) * 2^-24 * sum|terms| + 1e-7:
recursive summation, unit round-off 2^-24, at most four roundings per term), the edges of the 64-position windows,
run-to-run equality, no host synchronisation, a MAG-shaped step replayed through the optimiser, and the default path
unchanged."""
import numpy as np
import pytest

from augment_cases import close, ref_grad, rows_case, rows_to_coo
from test_gpu_embedding import _attr_csr, _bags, _csr_tensors, emb_ref

pytestmark = pytest.mark.gpu

PATTERN = [2.0 ** 25, 1.0, -2.0 ** 25, 1.0]              # a float32 left-to-right sum loses each 1 that meets 2^25


def _left_to_right(G):
    """float32 sum over axis 0 of G [L, F], one row after another from 0.0f: the order contract's sum."""
    acc = np.zeros(G.shape[1], np.float32)
    for row in np.asarray(G, np.float32):
        acc = (acc + row).astype(np.float32)
    return acc


def _bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _hash_keep(seed, entries, p):
    """csrc/gp_common.hpp's keep decision of (seed, entry) in numpy: uint8, 1 = kept."""
    with np.errstate(over="ignore"):
        x = np.uint64(seed) + entries.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).astype(np.uint8)


def _rows_grad(X, col, val, filled, K, rows, G, **kw):
    """features.grad of random_prop_rows under upstream gradient G (CPU tensors in, CUDA gradient and output out)."""
    from grand_plus_amd.augment import random_prop_rows
    x = X.cuda().requires_grad_(True)
    out = random_prop_rows(x, col.reshape(-1).cuda(), val.reshape(-1).cuda(), None if filled is None else filled.cuda(), K,
                           batch_rows=None if rows is None else rows.cuda(), **kw)
    out.backward(G.cuda())
    return x.grad, out.detach()


# ---------------------------------------------------------------------------------------------- the order contract
@pytest.mark.parametrize("B", [3, 65])
def test_rows_order_is_ascending_batch_position(B):
    import torch
    N, F = 20, 3
    col = torch.full((B, 1), 7, dtype=torch.int32)
    val = torch.ones((B, 1), dtype=torch.float64)                        # coef = 1 / (1 + 1e-12) is exactly 1.0f
    filled = torch.ones(B, dtype=torch.int32)
    G = torch.tensor([PATTERN[b % 4] for b in range(B)], dtype=torch.float32)[:, None] * torch.tensor([1.0, -1.0, 0.5])
    want = _left_to_right(G.numpy())
    assert not np.array_equal(want, G.double().sum(0).float().numpy())   # the orders are told apart
    grad, _ = _rows_grad(torch.zeros((N, F)), col, val, filled, 1, None, G, training=False, deterministic=True)
    assert _bits(grad[7].cpu(), torch.from_numpy(want))
    grad[7] = 0
    assert torch.count_nonzero(grad) == 0
    # the same entries named through batch_rows in reverse: the order is the batch position's, not the resident row's
    rows = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    grad, _ = _rows_grad(torch.zeros((N, F)), col, val, filled, 1, rows, G, training=False, deterministic=True)
    assert _bits(grad[7].cpu(), torch.from_numpy(want))


@pytest.mark.parametrize("n_bags", [3, 65])
def test_bag_order_is_ascending_entry_position(n_bags):
    import torch
    from grand_plus_amd.embedding import embedding_bag
    V, H = 30, 3
    attr = torch.full((n_bags,), 11, dtype=torch.int64).cuda()
    node = torch.arange(n_bags, dtype=torch.int64).cuda()
    d = torch.ones(n_bags).cuda()                                        # inv = 1 / (1 + 1e-10) is exactly 1.0f
    G = torch.tensor([PATTERN[b % 4] for b in range(n_bags)], dtype=torch.float32)[:, None] * torch.tensor([1.0, -1.0, 0.5])
    want = _left_to_right(G.numpy())
    assert not np.array_equal(want, G.double().sum(0).float().numpy())
    W = torch.zeros((V, H), device="cuda", requires_grad=True)
    embedding_bag(W, attr, node, d, training=False, deterministic=True).backward(G.cuda())
    assert _bits(W.grad[11].cpu(), torch.from_numpy(want))
    W.grad[11] = 0
    assert torch.count_nonzero(W.grad) == 0


# ---------------------------------------------------------------------------------------------- against float64
def _rows_inputs(F, S, seed):
    import torch
    col, val, filled, X, g = rows_case(seed=seed, F=F, empty_row=3, second_duplicate=True)
    S_rows, K = col.shape
    rows = torch.cat([torch.tensor([5, 11, 3, 5]), torch.randperm(S_rows, generator=g)[:56]]).to(torch.int32)   # row 5 twice
    rows = torch.flip(rows, [0])                                                                                   # ... in reverse
    G = torch.randn((S, rows.numel(), F), generator=g)
    return col, val, filled, X, g, rows, G


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("F", [1, 7, 64, 65, 130])
def test_rows_backward_matches_float64(F, S):
    """Eval, and training with an explicit mask (p = 0.5, 0, 1) and with a seed (the mask the forward draws, rebuilt here
    from the hash; the forward under that explicit mask is the seeded forward bit for bit).  Every destination has at most
    61 contributions (node 7: once per batch row, twice in row 5, which the batch names twice)."""
    import torch
    col, val, filled, X, g, rows, G = _rows_inputs(F, S, seed=10 * F + S)
    S_rows, K = col.shape
    samples, Gs = (S, G) if S > 1 else (1, G[0])
    seed = 0xC0FFEE + F
    from grand_plus_amd.augment import sample_seed
    hashed = np.stack([_hash_keep(sample_seed(seed, s), np.arange(S_rows * K), 0.5) for s in range(S)])
    for training, p, keep, sd in ((False, 0.5, None, None), (True, 0.5, "mask", None), (True, 0.0, "mask", None),
                                  (True, 1.0, "mask", None), (True, 0.5, None, seed)):
        if sd is not None:
            keep_t = torch.from_numpy(hashed)
        else:
            keep_t = (torch.rand((S, S_rows, K), generator=g) >= p).to(torch.uint8) if training else torch.ones((S, S_rows, K), dtype=torch.uint8)
        idx, cols, scores, kp = rows_to_coo(col, val, filled, K, rows, keep_t)
        ref, terms = ref_grad(X, scores, idx, p, training, kp if S > 1 else kp[0], Gs, cols=cols)
        kw = dict(dropnode_rate=p, training=training, samples=samples)
        if keep == "mask":
            kw["keep"] = keep_t.reshape(-1).cuda()
        if sd is not None:
            kw["seed"] = sd
        grad, out = _rows_grad(X, col, val, filled, K, rows, Gs, deterministic=True, **kw)
        close(grad, ref, terms)
        assert float(grad[7].abs().sum()) > 0 or (training and p == 1.0)
        if sd is not None:                                               # the rebuilt mask is the forward's
            kw.pop("seed")
            _, explicit = _rows_grad(X, col, val, filled, K, rows, Gs, deterministic=True, keep=keep_t.reshape(-1).cuda(), **kw)
            assert _bits(out, explicit)
        if training and p == 1.0:
            assert torch.count_nonzero(grad) == 0


def test_rows_column_ids_outside_the_graph_are_skipped():
    """One slot with column -1 and one with column N: counted in the denominator (as the atomic backward counts them),
    never written.  Straight through the backward (the forward would read them)."""
    import torch
    from grand_plus_amd.augment import _rows_backward, _rows_backward_det
    F, K = 65, 32
    col, val, filled, X, g = rows_case(seed=4, S_rows=40, K=K, N=300, F=F, empty_row=2)
    N = X.shape[0]
    filled[6] = filled[9] = K
    col[6, 4], col[9, 0] = -1, N
    rows = torch.arange(40, dtype=torch.int32)
    G = torch.randn((40, F), generator=g)
    idx, cols, scores, kp = rows_to_coo(col, val, filled, K, rows, torch.ones((1, 40, K), dtype=torch.uint8))
    cols = torch.where((cols < 0) | (cols >= N), torch.full_like(cols, N), cols)          # a phantom node N takes them
    ref, terms = ref_grad(torch.cat([X, torch.zeros((1, F))]), scores, idx, 0.0, False, kp[0], G, cols=cols)
    args = (G.cuda(), col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda(), K, rows.cuda(), 40, N, None, 0.0, False, 0, None)
    got = _rows_backward_det(*args)
    close(got, ref[:N], terms[:N])
    close(_rows_backward(*args), ref[:N], terms[:N])


def _bag_check(W, attr_idx, node_idx, attr_data, p, training, keep, G, **kw):
    """test_gpu_embedding._check_layer for a chosen backward; ids outside [0, V) go to a phantom zero row V of the
    reference (in the denominator, nothing to add, no gradient)."""
    import torch
    from grand_plus_amd.embedding import embedding_bag
    V = W.shape[0]
    a_ref = torch.where((attr_idx < 0) | (attr_idx >= V), torch.full_like(attr_idx, V), attr_idx)
    W64 = torch.cat([W.double().cpu(), torch.zeros((1, W.shape[1]), dtype=torch.float64)])
    ws = W64.clone().requires_grad_(True)
    ref = emb_ref(ws, a_ref, node_idx, attr_data, p, training, keep)
    (ref * G.double()).sum().backward()
    wa = W64.abs().clone().requires_grad_(True)
    (emb_ref(wa, a_ref, node_idx, attr_data, p, training, keep) * G.double().abs()).sum().backward()
    Wc = W.detach().clone().requires_grad_(True)
    out = embedding_bag(Wc, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), input_droprate=p, training=training,
                        keep=keep.reshape(-1).cuda() if keep is not None else None, **kw)
    out.backward(G.cuda())
    close(Wc.grad, ws.grad[:V], wa.grad[:V])
    return Wc.grad, out.detach()


@pytest.mark.parametrize("H", [1, 7, 64, 65, 100])
@pytest.mark.parametrize("training,p", [(False, 0.0), (True, 0.5), (True, 0.0)])
def test_bag_backward_matches_float64(H, training, p):
    """_bags: repeated ids inside and across bags, zero weights, empty bags, a 150-entry bag; V = 500, about 600 entries:
    every id has far fewer than 128 contributions.  Two ids outside [0, V): skipped (validate=False), never written."""
    import torch
    V = 500
    attr_idx, node_idx, attr_data, g = _bags(V, 80, seed=3 * H + int(10 * p) + training)
    attr_idx[7], attr_idx[40] = -1, V
    W = torch.randn((V, H), generator=g).cuda()
    keep = (torch.rand((attr_idx.numel(), H), generator=g) >= p).to(torch.uint8)
    G = torch.randn((int(node_idx[-1]) + 1, H), generator=g)
    grad, out = _bag_check(W, attr_idx, node_idx, attr_data, p, training, keep, G, validate=False, deterministic=True)
    _, out_atomic = _bag_check(W, attr_idx, node_idx, attr_data, p, training, keep, G, validate=False, deterministic=False)
    assert _bits(out, out_atomic)                                        # the flag does not change the forward by a bit


def test_bag_ids_outside_the_table_are_counted_and_never_written():
    """The C entry point on a gradient inside guard rows, as test_gpu_embedding.test_out_of_range_ids holds the atomic one."""
    import ctypes
    import torch
    from grand_plus_amd import _native
    from grand_plus_amd.embedding import _det_order, _Layout
    V, H = 50, 64
    attr_idx = torch.tensor([3, V, 4, -1, 5, V + 100]).cuda()
    data = torch.ones(6).cuda()
    offsets = torch.tensor([0, 2, 5, 5, 6]).cuda()
    L = _Layout(offsets, 4, None, None, 4, attr_idx, data)
    order, keys, rows = _det_order(L, 6, V)
    assert keys.tolist() == [3, 4, 5, V, V, V] and order.tolist() == [0, 2, 4, 1, 3, 5]
    gbuf = torch.zeros((V + 4, H), device="cuda")
    G = torch.ones((4, H), device="cuda")
    n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    inv = torch.empty(_native.scatter_bag_workspace_bytes(4) // 4, device="cuda")
    _native.raise_for_status(_native.lib().gp_embedding_bag_backward_det(
        0, G.data_ptr(), V, H, *L.args(), 0.0, 0, ctypes.c_uint64(0), None, gbuf[2:V + 2].data_ptr(), n_bad.data_ptr(),
        order.data_ptr(), keys.data_ptr(), rows.data_ptr(), 6, inv.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert int(n_bad.item()) == 3
    assert torch.count_nonzero(gbuf[:2]) == 0 and torch.count_nonzero(gbuf[V + 2:]) == 0
    assert torch.count_nonzero(gbuf[2:V + 2].sum(1)) == 3                # rows 3, 4, 5 only
    torch.testing.assert_close(gbuf[2 + 3], torch.full((H,), 0.5, device="cuda"), rtol=1e-6, atol=0)
    torch.testing.assert_close(gbuf[2 + 4], torch.full((H,), 1 / 3, device="cuda"), rtol=1e-6, atol=0)


def _close_hub(got, ref, terms, L):
    got, ref, terms = got.double().cpu(), ref.double().cpu(), terms.double().cpu()
    bad = (got - ref).abs() > (L + 4) * 2.0 ** -24 * terms + 1e-7
    assert not bool(bad.any()), f"{int(bad.sum())} elements off; max |d| {float((got - ref).abs().max()):.3e}"


def _hub_rows():
    import torch
    B, F, N = 4097, 65, 20
    g = torch.Generator().manual_seed(1)
    col = torch.full((B, 1), 7, dtype=torch.int32)
    val = torch.rand((B, 1), generator=g, dtype=torch.float64) + 0.1
    filled = torch.ones(B, dtype=torch.int32)
    X = torch.randn((N, F), generator=g)
    G = torch.randn((B, F), generator=g)
    return col, val, filled, X, G


def _hub_bags():
    import torch
    n, H, V = 4097, 7, 130
    g = torch.Generator().manual_seed(2)
    node_idx = torch.repeat_interleave(torch.arange(n), 2)               # two entries per bag: the hub id 13 and another
    attr_idx = torch.stack([torch.full((n,), 13), 20 + torch.arange(n) % 100], 1).reshape(-1)
    attr_data = torch.rand((2 * n,), generator=g) + 0.05
    W = torch.randn((V, H), generator=g)
    G = torch.randn((n, H), generator=g)
    return W, attr_idx, node_idx, attr_data, G


def test_hub_destinations_hold_the_derived_bound_and_repeat_bit_for_bit():
    """One destination with L = 4 097 contributions, five backwards from the same inputs."""
    import torch
    from grand_plus_amd.embedding import embedding_bag
    col, val, filled, X, G = _hub_rows()
    B = col.shape[0]
    idx, cols, scores, kp = rows_to_coo(col, val, filled, 1, torch.arange(B), torch.ones((1, B, 1), dtype=torch.uint8))
    ref, terms = ref_grad(X, scores, idx, 0.0, False, kp[0], G, cols=cols)
    grads = [_rows_grad(X, col, val, filled, 1, None, G, training=False, deterministic=True)[0] for _ in range(5)]
    _close_hub(grads[0], ref, terms, B)
    assert all(_bits(grads[0], x) for x in grads[1:])
    W, attr_idx, node_idx, attr_data, G = _hub_bags()
    n = G.shape[0]
    assert int((attr_idx == 13).sum()) == n and int(torch.bincount(attr_idx).max()) == n
    ws = W.double().clone().requires_grad_(True)
    (emb_ref(ws, attr_idx, node_idx, attr_data, 0.0, False, None) * G.double()).sum().backward()
    wa = W.double().abs().requires_grad_(True)
    (emb_ref(wa, attr_idx, node_idx, attr_data, 0.0, False, None) * G.double().abs()).sum().backward()
    grads = []
    for _ in range(5):
        Wc = W.cuda().requires_grad_(True)
        embedding_bag(Wc, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), training=False, deterministic=True).backward(G.cuda())
        grads.append(Wc.grad)
    _close_hub(grads[0], ws.grad, wa.grad, n)
    assert all(_bits(grads[0], x) for x in grads[1:])


# ---------------------------------------------------------------------------------------------- window edges
# sorted positions: key 0 at 0..62 (63 long), key 1 at 63 (starts at position 63), key 2 at 64..127 (64 long, starts at 64,
# ends at a window's end), key 3 at 128..192 (65 long, runs past its window), key 4 at 193..255 (63 long, ends at a window's
# end), key 5 at 256..265: the last segment, running into the sentinel tail
SEGMENTS = [63, 1, 64, 65, 63, 10]


def _edge_entries(seed, n_dead):
    """Destination of each entry (-1: an entry that does not exist), shuffled, and an upstream gradient row per entry."""
    import torch
    g = torch.Generator().manual_seed(seed)
    dest = torch.cat([torch.full((n,), k) for k, n in enumerate(SEGMENTS)] + [torch.full((n_dead,), -1)])
    dest = dest[torch.randperm(dest.numel(), generator=g)]
    G = torch.randn((dest.numel(), 70), generator=g) * 10.0 ** torch.randint(-3, 4, (dest.numel(), 1), generator=g)
    return dest, G


def _edge_expected(dest, G, n_dest):
    want = np.zeros((n_dest, G.shape[1]), np.float32)
    for k in range(len(SEGMENTS)):
        want[k] = _left_to_right(G.numpy()[(dest == k).numpy()])
    return want


def test_rows_window_edges_bit_for_bit():
    import torch
    dest, G = _edge_entries(5, n_dead=40)
    B, N = dest.numel(), 9
    col = dest.clamp(min=0).to(torch.int32)[:, None]
    filled = (dest >= 0).to(torch.int32)                                 # the dead entries are unfilled slots
    val = torch.ones((B, 1), dtype=torch.float64)
    grad, _ = _rows_grad(torch.zeros((N, G.shape[1])), col, val, filled, 1, None, G, training=False, deterministic=True)
    assert _bits(grad.cpu(), torch.from_numpy(_edge_expected(dest, G, N)))
    # every slot unfilled: an all-sentinel order, an exactly zero gradient; and an empty batch
    grad, _ = _rows_grad(torch.zeros((N, 70)), col, val, torch.zeros(B, dtype=torch.int32), 1, None, G, training=False, deterministic=True)
    assert torch.count_nonzero(grad) == 0
    grad, out = _rows_grad(torch.zeros((N, 70)), col, val, filled, 1, torch.zeros(0, dtype=torch.int32), G[:0], training=False,
                           deterministic=True)
    assert out.shape == (0, 70) and grad.shape == (N, 70) and torch.count_nonzero(grad) == 0


def test_bag_window_edges_bit_for_bit():
    import torch
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    V = 9
    dest, G = _edge_entries(6, n_dead=40)
    n = dest.numel()
    attr = torch.where(dest >= 0, dest, torch.full_like(dest, V + 3))    # the dead entries carry an id outside the table
    W = torch.zeros((V, G.shape[1]), device="cuda", requires_grad=True)
    embedding_bag(W, attr.cuda(), torch.arange(n).cuda(), torch.ones(n).cuda(), training=False, validate=False,
                  deterministic=True).backward(G.cuda())
    assert _bits(W.grad.cpu(), torch.from_numpy(_edge_expected(dest, G, V)))
    # every id outside the table: an all-sentinel order; then no bags at all, and bags that are all empty
    W.grad = None
    embedding_bag(W, torch.full((n,), V).cuda(), torch.arange(n).cuda(), torch.ones(n).cuda(), training=False, validate=False,
                  deterministic=True).backward(G.cuda())
    assert torch.count_nonzero(W.grad) == 0
    ip = torch.tensor([0, 0, 0, 3]).cuda()
    ix, dt = torch.tensor([1, 2, 3], dtype=torch.int32).cuda(), torch.ones(3).cuda()
    for nodes in (torch.zeros(0, dtype=torch.int64), torch.tensor([0, 1, 1])):
        W.grad = None
        out = embedding_bag_csr(W, ip, ix, dt, nodes=nodes.cuda(), training=False, deterministic=True)
        out.backward(torch.ones_like(out))
        assert out.shape == (nodes.numel(), G.shape[1]) and W.grad.shape == W.shape and torch.count_nonzero(W.grad) == 0


# ---------------------------------------------------------------------------------------------- determinism, the flag
def test_coo_and_csr_forms_give_the_same_gradient_bit_for_bit():
    """embedding_bag on features[nodes].nonzero() and embedding_bag_csr(nodes): the same entry order and the same keys, so
    the same dW under deterministic=True, int64 ids against int32 ids; both within `close` of float64."""
    import torch
    from grand_plus_amd.embedding import embedding_bag_csr
    N, V, H = 600, 300, 65
    A = _attr_csr(N, V, seed=2, density=0.03)
    A[100] = 0; A.eliminate_zeros()
    ip, ix, dt = _csr_tensors(A)
    g = torch.Generator().manual_seed(0)
    W = torch.randn((V, H), generator=g).cuda()
    nodes = torch.tensor([5, 100, 5, 599, 17, 100, 0] + list(range(200, 500, 3)), dtype=torch.int64)
    sub = A[nodes.numpy()]
    node_idx, attr_idx = sub.nonzero()
    node_idx, attr_idx = torch.from_numpy(node_idx.astype(np.int64)), torch.from_numpy(attr_idx.astype(np.int64))
    assert int(torch.bincount(attr_idx).max()) <= 128
    n_out = int(node_idx[-1]) + 1
    G = torch.randn((nodes.numel(), H), generator=g)
    keep = (torch.rand((attr_idx.numel(), H), generator=g) >= 0.5).to(torch.uint8)
    coo, _ = _bag_check(W, attr_idx, node_idx, torch.from_numpy(sub.data), 0.5, True, keep, G[:n_out], deterministic=True)
    Wc = W.clone().requires_grad_(True)
    embedding_bag_csr(Wc, ip, ix, dt, nodes=nodes.cuda(), input_droprate=0.5, training=True, keep=keep.reshape(-1).cuda(),
                      deterministic=True).backward(G.cuda())             # rows past n_out are empty bags
    assert _bits(coo, Wc.grad)


def test_none_follows_torchs_deterministic_mode():
    import torch
    from grand_plus_amd.embedding import embedding_bag
    col, val, filled, X, g, rows, G = _rows_inputs(64, 2, seed=8)
    K = col.shape[1]
    kw = dict(dropnode_rate=0.5, training=True, seed=5, samples=2)
    on, out_on = _rows_grad(X, col, val, filled, K, rows, G, deterministic=True, **kw)
    off, out_off = _rows_grad(X, col, val, filled, K, rows, G, deterministic=False, **kw)
    attr_idx, node_idx, attr_data, gb = _bags(500, 80, seed=1)
    W = torch.randn((500, 64), generator=gb).cuda()
    Gb = torch.randn((int(node_idx[-1]) + 1, 64), generator=gb).cuda()

    def bag(**kw):
        Wc = W.clone().requires_grad_(True)
        embedding_bag(Wc, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), 0.5, True, seed=9, **kw).backward(Gb)
        return Wc.grad

    bag_on = bag(deterministic=True)
    was = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(True)
        follows, out_follows = _rows_grad(X, col, val, filled, K, rows, G, **kw)
        bag_follows = bag()
    finally:
        torch.use_deterministic_algorithms(was)
    assert _bits(follows, on) and _bits(bag_follows, bag_on)
    assert _bits(out_on, out_off) and _bits(out_on, out_follows)         # the forward never changes
    assert off.shape == on.shape


def test_default_path_is_still_the_atomic_backward_and_matches_float64():
    """deterministic=False and the default outside deterministic mode: today's kernels, today's tolerance."""
    import torch
    assert not torch.are_deterministic_algorithms_enabled()
    col, val, filled, X, g, rows, G = _rows_inputs(65, 2, seed=12)
    S_rows, K = col.shape
    keep_t = (torch.rand((2, S_rows, K), generator=g) >= 0.5).to(torch.uint8)
    idx, cols, scores, kp = rows_to_coo(col, val, filled, K, rows, keep_t)
    ref, terms = ref_grad(X, scores, idx, 0.5, True, kp, G, cols=cols)
    for kw in (dict(), dict(deterministic=False)):
        grad, _ = _rows_grad(X, col, val, filled, K, rows, G, dropnode_rate=0.5, training=True, samples=2,
                             keep=keep_t.reshape(-1).cuda(), **kw)
        close(grad, ref, terms)
    attr_idx, node_idx, attr_data, gb = _bags(500, 80, seed=4)
    W = torch.randn((500, 65), generator=gb).cuda()
    keep = (torch.rand((attr_idx.numel(), 65), generator=gb) >= 0.5).to(torch.uint8)
    Gb = torch.randn((int(node_idx[-1]) + 1, 65), generator=gb)
    for kw in (dict(), dict(deterministic=False)):
        _bag_check(W, attr_idx, node_idx, attr_data, 0.5, True, keep, Gb, **kw)


def test_no_host_synchronisation():
    """Forward and backward under torch's sync debug mode: the rows form, embedding_bag (with the caller's n_out and
    validate=False, which are its two host reads) and embedding_bag_csr(nodes=None)."""
    import torch
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    col, val, filled, X, g, rows, G = _rows_inputs(64, 2, seed=3)
    K = col.shape[1]
    x = X.cuda().requires_grad_(True)
    cc, vc, fc, rc, Gc = col.reshape(-1).cuda(), val.reshape(-1).cuda(), filled.cuda(), rows.cuda(), G.cuda()
    attr_idx, node_idx, attr_data, gb = _bags(500, 80, seed=1)
    n_out = int(node_idx[-1]) + 1
    W = torch.randn((500, 64), generator=gb).cuda().requires_grad_(True)
    ai, ni, ad = attr_idx.cuda(), node_idx.cuda(), attr_data.cuda()
    Gb = torch.randn((n_out, 64), generator=gb).cuda()
    A = _attr_csr(300, 500, seed=3, density=0.02)
    ip, ix, dt = _csr_tensors(A)
    Ga = torch.randn((300, 64), generator=gb).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        random_prop_rows(x, cc, vc, fc, K, batch_rows=rc, dropnode_rate=0.5, training=True, seed=1, samples=2,
                         deterministic=True).backward(Gc)
        random_prop_rows(x, cc, vc, None, K, dropnode_rate=0.5, training=True, seed=1, deterministic=True).sum().backward()
        embedding_bag(W, ai, ni, ad, 0.5, True, seed=2, validate=False, deterministic=True, n_out=n_out).backward(Gb)
        embedding_bag_csr(W, ip, ix, dt, input_droprate=0.5, training=True, seed=3, validate=False,
                          deterministic=True).backward(Ga)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert float(x.grad.abs().sum()) > 0 and float(W.grad.abs().sum()) > 0


# ---------------------------------------------------------------------------------------------- end to end
def test_mag_shaped_step_replays_bit_for_bit_through_the_optimiser():
    """test_gpu_embedding.py's MAG-shaped step: gfpush_device -> flatten_rows -> embedding_bag_csr -> random_prop(samples=2)
    -> MagMLP -> grand_plus_loss -> backward -> ClipAdam.step(), run twice from identical state and seeds with
    deterministic=True (and three more backwards): every gradient and every stepped parameter bitwise equal.  The
    table's gradient is held to float64 under `close` where that rule is defined, at the layer: emb_ref in float64 fed the
    gradient that arrived at the layer's output in this step."""
    import copy
    import torch
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop
    from grand_plus_amd.embedding import flatten_rows
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.optim import ClipAdam
    from grand_plus_amd.recipes import make_coef
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 300)
    K, H, C, V, p_node, S = 32, 64, 8, 900, 0.5, 2
    g = Graph(indptr, indices, 0)
    _, col, val, filled = g.gfpush_device(torch.from_numpy(seeds).cuda(), make_coef("ppr", 6, 0.2), 1e-5, K)
    A = _attr_csr(n, V, seed=5, density=0.02)
    ip, ix, dt = _csr_tensors(A)
    torch.manual_seed(0)
    model0 = MagMLP(V, C, H, 2, False, 0.3, 0.2, False).cuda().train()
    batch_rows = torch.arange(0, 40, dtype=torch.int32).cuda()
    n_train = 20
    labels = torch.randint(0, C, (n_train,), generator=torch.Generator().manual_seed(0)).cuda()
    nbr, scores, mat_idx = flatten_rows(col, val, filled, K, batch_rows)

    def step(model, optimise=True):
        grabbed = []
        emb = model.emb_csr(ip, ix, dt, nodes=nbr, seed=11, deterministic=True)
        emb.register_hook(grabbed.append)
        aug = random_prop(emb, scores, mat_idx, p_node, training=True, seed=12, samples=S, n_out=40)
        loss, _ = grand_plus_loss(model(aug, seed=13), labels, n_train, 1.0, tem=0.5, conf=0.0, kind="l2")
        loss.backward()
        grads = [p.grad.clone() for p in model.parameters() if p.grad is not None]       # BatchNorm is off: no gradient there
        if optimise:
            ClipAdam(model.parameters(), lr=1e-2, weight_decay=5e-4, clip_norm=0.1).step()
        return grads, [p.detach().clone() for p in model.parameters()], grabbed[0]

    first, second = step(copy.deepcopy(model0)), step(copy.deepcopy(model0))
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert _bits(a, b)
    assert any(not _bits(p, q.detach()) for p, q in zip(first[1], model0.parameters()))        # the step moved the parameters
    for _ in range(3):
        again = step(copy.deepcopy(model0), optimise=False)
        assert all(_bits(a, b) for a, b in zip(first[0], again[0]))
    # the table's gradient against float64, entry order = the CSR form's = features[nbr].nonzero()
    sub = A[nbr.cpu().numpy()]
    node_idx, attr_idx = sub.nonzero()
    node_idx, attr_idx = torch.from_numpy(node_idx.astype(np.int64)), torch.from_numpy(attr_idx.astype(np.int64))
    assert int(torch.bincount(attr_idx).max()) <= 128
    keep = torch.from_numpy(_hash_keep(11, np.arange(attr_idx.numel() * H), 0.3)).reshape(-1, H)
    n_out = int(node_idx[-1]) + 1
    G_emb = first[2].cpu()[:n_out]
    data = torch.from_numpy(sub.data)
    W0 = model0.embeds.weight.detach().cpu()
    ws = W0.double().clone().requires_grad_(True)
    (emb_ref(ws, attr_idx, node_idx, data, 0.3, True, keep) * G_emb.double()).sum().backward()
    wa = W0.double().abs().requires_grad_(True)
    (emb_ref(wa, attr_idx, node_idx, data, 0.3, True, keep) * G_emb.double().abs()).sum().backward()
    dW = first[0][0]
    assert dW.shape == (V, H) and float(dW.abs().max()) > 0
    close(dW, ws.grad, wa.grad)
