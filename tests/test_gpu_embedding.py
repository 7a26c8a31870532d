"""MAG's embedding-bag layer against a float64 restatement of `MLP.emb` (model_mag.py:48-55) kept in
augment_cases.py: `index_add_` for torch_scatter's scatter-sum, explicit dropout masks, autograd for the reference
gradients.  Tolerance per element: |d| <= 1e-5 * sum|terms| + 1e-7, sum|terms| = the same quantity with every
operand replaced by its magnitude.  Ends with a MAG-shaped training step: gfpush_device -> flatten_rows ->
embedding_bag_csr -> random_prop x 2 -> MLP -> NLL + l2 consistency loss -> backward."""
import ctypes

import numpy as np
import pytest

from augment_cases import close, emb_ref
from oracle.objective_ref import consis_loss_ref

pytestmark = pytest.mark.gpu


def _bags(V, n_out, seed, max_len=12):
    """Sorted node_idx with empty bags in the middle, one long bag, ids repeated within and across bags, some zero weights."""
    import torch
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(0, max_len, (n_out,), generator=g)
    lens[2] = 0; lens[5] = 0; lens[6] = 0; lens[-1] = 3
    lens[10] = 150                                                               # longer than a wave's 64-entry read round
    node_idx = torch.repeat_interleave(torch.arange(n_out), lens)
    nnz = node_idx.numel()
    attr_idx = torch.randint(0, V, (nnz,), generator=g)
    attr_idx[1] = attr_idx[0]                                                   # repeated inside a bag (bag 0 has >= 2 entries or not:
    attr_idx[nnz // 2] = attr_idx[0]                                            # either way repeated across bags)
    attr_data = torch.rand((nnz,), generator=g) + 0.05
    attr_data[::7] = 0.0
    return attr_idx, node_idx, attr_data, g


def _check_layer(W, attr_idx, node_idx, attr_data, p, training, keep, G):
    """GPU forward + weight gradient against the restatement on the gathered unique rows."""
    import torch
    from grand_plus_amd.embedding import embedding_bag
    uniq, inv = torch.unique(attr_idx, return_inverse=True)
    Wsub = W[uniq.cuda()].double().cpu()
    ws = Wsub.clone().requires_grad_(True)
    ref = emb_ref(ws, inv, node_idx, attr_data, p, training, keep)
    (ref * G.double()).sum().backward()
    wa = Wsub.abs().clone().requires_grad_(True)
    terms = emb_ref(wa, inv, node_idx, attr_data, p, training, keep)
    (terms * G.double().abs()).sum().backward()
    Wc = W.detach().requires_grad_(True)
    out = embedding_bag(Wc, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), input_droprate=p, training=training,
                        keep=keep.reshape(-1).cuda() if keep is not None else None)
    assert out.shape == ref.shape and out.grad_fn is not None
    close(out, ref.detach(), terms.detach())
    out.backward(G.cuda())
    close(Wc.grad[uniq.cuda()], ws.grad, wa.grad)
    rest = torch.ones(W.shape[0], dtype=torch.bool, device="cuda"); rest[uniq.cuda()] = False
    assert torch.count_nonzero(Wc.grad[rest]) == 0                              # rows no bag names are untouched
    return out


@pytest.mark.parametrize("H", [7, 64, 100])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("training", [False, True])
def test_embedding_bag_forward_and_weight_gradient(H, p, training):
    import torch
    V = 500
    attr_idx, node_idx, attr_data, g = _bags(V, 80, seed=H + int(10 * p) + training)
    W = torch.randn((V, H), generator=g).cuda()
    keep = (torch.rand((attr_idx.numel(), H), generator=g) >= p).to(torch.uint8)
    G = torch.randn((int(node_idx[-1]) + 1, H), generator=g)
    out = _check_layer(W, attr_idx, node_idx, attr_data, p, training, keep, G)
    assert torch.count_nonzero(out[2]) == 0 and torch.count_nonzero(out[5:7]) == 0          # empty bags are zero rows


def test_embedding_bag_table_above_2gib():
    import torch
    V, H = 8_500_000, 64                                                         # V*H*4 = 2.18 GB > 2 GiB
    assert V * H * 4 > 2**31
    W = torch.empty((V, H), device="cuda").normal_()
    attr_idx, node_idx, attr_data, g = _bags(1000, 40, seed=11)
    attr_idx = V - 1 - attr_idx                                                  # ids near V - 1, offsets above 2^31 bytes
    attr_idx[0] = 0
    keep = (torch.rand((attr_idx.numel(), H), generator=g) >= 0.5).to(torch.uint8)
    G = torch.randn((int(node_idx[-1]) + 1, H), generator=g)
    _check_layer(W, attr_idx, node_idx, attr_data, 0.5, True, keep, G)


def _attr_csr(N, V, seed, density=0.01):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    A = sp.random(N, V, density=density, format="csr", random_state=rng, dtype=np.float64)
    A.data = (A.data + 0.05).astype(np.float32)                                # no explicit zeros: .nonzero() == storage
    A = A.astype(np.float32)
    A.sort_indices()
    return A


def _csr_tensors(A):
    import torch
    return (torch.from_numpy(A.indptr.astype(np.int64)).cuda(), torch.from_numpy(A.indices.astype(np.int32)).cuda(),
            torch.from_numpy(A.data.astype(np.float32)).cuda())


def test_csr_form_equals_coo_form_bitwise():
    import torch
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    N, V, H = 3000, 700, 64
    A = _attr_csr(N, V, seed=2)
    A[100] = 0; A.eliminate_zeros()                                             # an empty bag
    ip, ix, dt = _csr_tensors(A)
    W = torch.randn((V, H), generator=torch.Generator().manual_seed(0)).cuda()
    nodes = torch.tensor([5, 100, 5, 2999, 17, 100, 0] + list(range(200, 1200, 3)), dtype=torch.int64)
    sub = A[nodes.numpy()]
    node_idx, attr_idx = sub.nonzero()                                           # model_mag.py:345
    coo = embedding_bag(W, torch.from_numpy(attr_idx.astype(np.int64)).cuda(), torch.from_numpy(node_idx.astype(np.int64)).cuda(),
                        torch.from_numpy(sub.data).cuda(), input_droprate=0.5, training=True, seed=4242)
    csr = embedding_bag_csr(W, ip, ix, dt, nodes=nodes.cuda(), input_droprate=0.5, training=True, seed=4242)
    assert csr.shape == (nodes.numel(), H)
    assert torch.equal(csr[:coo.shape[0]], coo)
    assert torch.count_nonzero(csr[1]) == 0 and torch.count_nonzero(csr[5]) == 0
    # nodes=None: every node (predict's emb pass, model_mag.py:197-205)
    node_idx, attr_idx = A.nonzero()
    coo = embedding_bag(W, torch.from_numpy(attr_idx.astype(np.int64)).cuda(), torch.from_numpy(node_idx.astype(np.int64)).cuda(),
                        torch.from_numpy(A.data).cuda(), input_droprate=0.3, training=True, seed=7)
    csr = embedding_bag_csr(W, ip, ix, dt, input_droprate=0.3, training=True, seed=7)
    assert csr.shape == (N, H) and torch.equal(csr[:coo.shape[0]], coo)
    with torch.no_grad():
        ev = embedding_bag_csr(W, ip, ix, dt, training=False)
    assert ev.grad_fn is None
    ref = emb_ref(W.double().cpu(), torch.from_numpy(attr_idx.astype(np.int64)), torch.from_numpy(node_idx.astype(np.int64)),
                  torch.from_numpy(A.data), 0.0, False, None)
    terms = emb_ref(W.double().abs().cpu(), torch.from_numpy(attr_idx.astype(np.int64)), torch.from_numpy(node_idx.astype(np.int64)),
                    torch.from_numpy(A.data), 0.0, False, None)
    close(ev[:ref.shape[0]], ref, terms)


def test_out_of_range_ids():
    import torch
    from grand_plus_amd import _native
    from grand_plus_amd.embedding import embedding_bag
    V, H = 50, 64
    W = torch.randn((V, H)).cuda()
    node_idx = torch.tensor([0, 0, 1, 1, 1, 3]).cuda()
    attr_idx = torch.tensor([3, V, 4, -1, 5, V + 100]).cuda()
    data = torch.ones(6).cuda()
    with pytest.raises(IndexError):
        embedding_bag(W, attr_idx, node_idx, data)
    # validate=False: the bad ids are skipped.  The table and its gradient sit inside guard rows (NaN / zero)
    # that a read or write through an id of -1 or >= V would reach.
    buf = torch.full((V + 4, H), float("nan"), device="cuda"); buf[2:V + 2] = W
    out = torch.empty((4, H), device="cuda")
    offsets = torch.tensor([0, 2, 5, 5, 6]).cuda()
    n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    Wv = buf[2:V + 2]
    _native.raise_for_status(_native.lib().gp_embedding_bag(
        0, Wv.data_ptr(), V, H, offsets.data_ptr(), 4, None, None, 4, attr_idx.data_ptr(), 8, data.data_ptr(),
        0.0, 0, ctypes.c_uint64(0), None, out.data_ptr(), n_bad.data_ptr(), s))
    assert int(n_bad.item()) == 3 and not torch.isnan(out).any()
    torch.testing.assert_close(out[0], W[3] / 2, rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(out[1], (W[4] + W[5]) / 3, rtol=1e-6, atol=1e-7)
    assert torch.count_nonzero(out[2:]) == 0
    gbuf = torch.zeros((V + 4, H), device="cuda")
    G = torch.ones((4, H), device="cuda")
    _native.raise_for_status(_native.lib().gp_embedding_bag_backward(
        0, G.data_ptr(), V, H, offsets.data_ptr(), 4, None, None, 4, attr_idx.data_ptr(), 8, data.data_ptr(),
        0.0, 0, ctypes.c_uint64(0), None, gbuf[2:V + 2].data_ptr(), n_bad.data_ptr(), s))
    assert int(n_bad.item()) == 3
    assert torch.count_nonzero(gbuf[:2]) == 0 and torch.count_nonzero(gbuf[V + 2:]) == 0
    assert torch.count_nonzero(gbuf[2:V + 2].sum(1)) == 3                        # rows 3, 4, 5 only
    # the Python wrapper with validate=False: same output, and W.grad untouched outside the named rows
    Wr = W.clone().requires_grad_(True)
    o = embedding_bag(Wr, attr_idx, node_idx, data, validate=False)
    torch.testing.assert_close(o, out, rtol=0, atol=0)
    o.sum().backward()
    assert torch.count_nonzero(Wr.grad.sum(1)) == 3


def test_mag_shaped_training_step_end_to_end():
    import torch
    import torch.nn.functional as Fn
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.augment import random_prop
    from grand_plus_amd.embedding import embedding_bag_csr, flatten_rows
    from grand_plus_amd.recipes import make_coef
    from oracle.random_prop_ref import random_prop_ref
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 300)
    K, H, C, V, p_node, p_in = 32, 64, 8, 900, 0.5, 0.3
    g = Graph(indptr, indices, 0)
    _, col, val, filled = g.gfpush_device(torch.from_numpy(seeds).cuda(), make_coef("ppr", 6, 0.2), 1e-5, K)
    A = _attr_csr(n, V, seed=5, density=0.02)
    ip, ix, dt = _csr_tensors(A)
    gen = torch.Generator().manual_seed(0)
    W0 = torch.randn((V, H), generator=gen) * 0.1
    fc0 = torch.nn.Linear(H, C); fc0.weight.data = torch.randn((C, H), generator=gen) * 0.2; fc0.bias.data.zero_()
    batch_rows = torch.arange(0, 40, dtype=torch.int32).cuda()                  # 20 labelled + 20 unlabelled (run_mag.sh)
    n_train = 20
    labels = torch.randint(0, C, (n_train,), generator=gen)
    nbr, scores, mat_idx = flatten_rows(col, val, filled, K, batch_rows)
    M = nbr.numel()
    nnz = int((ip[nbr + 1] - ip[nbr]).sum())
    keeps = [((torch.rand((nnz, H), generator=gen) >= p_in).to(torch.uint8),
              (torch.rand((M,), generator=gen) >= p_node).to(torch.uint8)) for _ in range(2)]

    # this project's path
    W = W0.cuda().requires_grad_(True)
    fc = torch.nn.Linear(H, C).cuda(); fc.weight.data.copy_(fc0.weight.data); fc.bias.data.copy_(fc0.bias.data)
    outs, loss = [], 0.
    for ke, kn in keeps:                                                         # --sample 2, model_mag.py:354-361
        emb = embedding_bag_csr(W, ip, ix, dt, nodes=nbr, input_droprate=p_in, training=True, keep=ke.reshape(-1).cuda())
        aug = random_prop(emb, scores, mat_idx, p_node, training=True, keep=kn.cuda())
        logp = torch.log_softmax(fc(Fn.relu(aug)), dim=-1)
        outs.append(logp[n_train:])
        loss = loss + Fn.nll_loss(logp[:n_train], labels.cuda())
    loss = loss / 2 + 1.0 * consis_loss_ref(outs, 0.5, 0.0, "l2")
    loss.backward()

    # the restated pure-torch pipeline in float64 under the same masks (reference order: csr rows, nonzero)
    sub = A[nbr.cpu().numpy()]
    node_idx, attr_idx = sub.nonzero()
    node_idx, attr_idx = torch.from_numpy(node_idx.astype(np.int64)), torch.from_numpy(attr_idx.astype(np.int64))
    data = torch.from_numpy(sub.data)
    Wr = W0.double().requires_grad_(True)
    fw, fb = fc0.weight.data.double().requires_grad_(True), fc0.bias.data.double().requires_grad_(True)
    outs_r, loss_r = [], 0.
    for ke, kn in keeps:
        emb = emb_ref(Wr, attr_idx, node_idx, data, p_in, True, ke)
        emb = torch.cat([emb, emb.new_zeros((M - emb.shape[0], H))]) if emb.shape[0] < M else emb
        aug = random_prop_ref(emb, scores.cpu().double(), mat_idx.cpu(), p_node, True, kn)
        logp = torch.log_softmax(Fn.relu(aug) @ fw.t() + fb, dim=-1)
        outs_r.append(logp[n_train:])
        loss_r = loss_r + Fn.nll_loss(logp[:n_train], labels)
    loss_r = loss_r / 2 + 1.0 * consis_loss_ref(outs_r, 0.5, 0.0, "l2")
    loss_r.backward()

    assert abs(loss.item() - loss_r.item()) <= 1e-5 * abs(loss_r.item()) + 1e-7
    for got, ref in ((W.grad, Wr.grad), (fc.weight.grad, fw.grad), (fc.bias.grad, fb.grad)):
        scale = float(ref.abs().max())
        assert scale > 0
        torch.testing.assert_close(got.double().cpu(), ref, rtol=1e-4, atol=1e-5 * scale)
