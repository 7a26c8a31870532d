"""The evaluation head, valid and predict on the GPU.  The head gets the same fp32 logits as torch, so only
the head is under test there: predictions, flags and counts are exact, the loss follows §7g's rule against torch's
float64 CPU result (tests/evaluate_cases.py).  valid and predict are held exactly to the composition of the existing
pieces on the same logits, and to the float64 chain of the oracles within the bounds derived in evaluate_cases.chain64.
Error ratios ours / torch32 seen on the MI355X are listed in DESIGN §7h."""
import numpy as np
import pytest
import torch

import evaluate_cases as ec

pytestmark = pytest.mark.gpu


def _head(z, y, **kw):
    from grand_plus_amd import eval_head, eval_reduce
    buf = eval_head(z, y, **kw)
    loss, acc, counts = eval_reduce(buf)
    assert loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32 and acc.dim() == 0 and counts.dtype == torch.int64
    return buf, float(loss), float(acc), counts.tolist()


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", ec.HEAD_N)
@pytest.mark.parametrize("C", ec.HEAD_C)
def test_head_matches_torch(C, n):
    z, y, ref64 = ec.head_case(n, C)
    zd, yd = z.cuda(), y.cuda()
    buf, loss, acc, counts = _head(zd, yd)
    pred = torch.argmax(z, dim=1)
    assert torch.equal(buf.pred.cpu().long(), pred)
    assert torch.equal(buf.flag.cpu(), (pred == y).to(torch.uint8))
    n_correct = int((pred == y).sum())
    assert counts == [n, n_correct, 0, 0]
    assert acc == float(np.float32(n_correct / n))
    ec.assert_loss(loss, ec.nll32_on(zd, yd), ref64, f"head C={C} n={n}")
    per_row, bound = ec.bounds64(z, y)                       # row by row, from the kernel's order of operations
    share = float(((buf.nll.cpu().double() - per_row).abs() / bound).max())
    print(f"[evaluate] head C={C} n={n}: max row error / bound {share:.3g}")
    assert share <= 1.0 and float(bound.max()) <= 1e-5 * float(per_row.abs().max()) + 1e-6      # no wider than the batch-wide one was


def test_ties_and_nans_follow_argmax():
    z, y = ec.ties_case()
    buf, loss, acc, counts = _head(z.cuda(), y.cuda())
    expect = torch.argmax(z, dim=1)
    assert expect.tolist() == [0, 63, 64, 100, 5, 64, 0, 10] == np.argmax(z.numpy(), axis=1).tolist()
    assert torch.equal(buf.pred.cpu().long(), expect)
    assert buf.flag.tolist() == [1, 1, 1, 1, 2, 2, 2, 2] and counts == [4, 4, 4, 0] and acc == 0.5
    # a NaN row with a valid label gives a NaN loss, as torch does
    _, loss_nan, _, _ = _head(z[4:5].cuda(), torch.tensor([1]).cuda())
    assert np.isnan(loss_nan) and np.isnan(ec.nll32_on(z[4:5], torch.tensor([1])))


def test_row_and_label_indices_are_gathered_on_the_device():
    n, C = 200, 7
    z, y, _ = ec.head_case(4097, C)
    g = torch.Generator().manual_seed(9)
    rows = torch.randint(0, 4097, (n,), generator=g)
    rows[:40] = torch.arange(4096, 4056, -1)                 # reverse order
    rows[40:60] = 17                                         # duplicates
    lrows = torch.randint(0, 4097, (n,), generator=g)        # labels picked by another list
    buf, loss, acc, counts = _head(z.cuda(), y.cuda(), rows=rows.cuda(), label_rows=lrows.cuda())
    zz, yy = z[rows], y[lrows]
    pred = torch.argmax(zz, dim=1)
    assert torch.equal(buf.pred.cpu().long(), pred) and torch.equal(buf.flag.cpu(), (pred == yy).to(torch.uint8))
    assert counts == [n, int((pred == yy).sum()), 0, 0]
    ec.assert_loss(loss, ec.nll32_on(zz.cuda(), yy.cuda()), float(ec.nll64(zz, yy)), "gathered")
    # rows alone: labels[i]; label_rows alone: logits[i]
    b2, *_ = _head(z.cuda(), y.cuda(), rows=rows.cuda())
    assert torch.equal(b2.flag.cpu(), (pred == y[:n]).to(torch.uint8))
    b3, *_ = _head(z.cuda(), y.cuda(), label_rows=lrows.cuda())
    assert torch.equal(b3.flag.cpu(), (torch.argmax(z[:n], dim=1) == yy).to(torch.uint8))


def test_ignored_and_bad_rows_are_counted_and_leave_the_others_unchanged():
    z, y, y2, rows, lrows, ignored, bad = ec.ignored_case()
    n, C = z.shape
    clean, *_ = _head(z.cuda(), y.cuda())
    buf, loss, acc, counts = _head(z.cuda(), y2.cuda(), rows=rows.cuda(), label_rows=lrows.cuda())
    assert (ignored, bad) == ([3, 77], [5, 100, 200, 9, 10, 11, 12])
    keep = torch.ones(n, dtype=torch.bool)
    keep[ignored + bad] = False
    assert buf.flag[ignored].tolist() == [2, 2] and buf.flag[bad].tolist() == [3] * 7
    assert buf.nll[ignored + bad].abs().sum().item() == 0.0 and buf.pred[[9, 10]].tolist() == [-1, -1]
    other = [i for i in range(n) if i not in (9, 10)]
    assert torch.equal(buf.pred[other], clean.pred[other])   # the argmax is reported whatever the label
    assert _same([t[keep.cuda()] for t in buf], [t[keep.cuda()] for t in clean])
    n_correct = int(clean.flag.cpu()[keep].sum())
    assert counts == [n - 9, n_correct, 2, 7] and acc == float(np.float32(n_correct / n))
    ec.assert_loss(loss, ec.nll32_on(z[keep].cuda(), y[keep].cuda()), float(ec.nll64(z[keep], y[keep])), "with ignored and bad rows")
    # another ignore_index; all rows ignored: NaN loss, acc 0
    _, loss_i, acc_i, counts_i = _head(z.cuda(), torch.full((n,), 3).cuda(), ignore_index=3)
    assert np.isnan(loss_i) and acc_i == 0.0 and counts_i == [0, 0, n, 0]


def test_split_independence_and_determinism():
    from grand_plus_amd import eval_head, eval_reduce
    from grand_plus_amd.evaluate import eval_buffers
    n, C = 4097, 65
    z, y, _ = ec.head_case(n, C)
    zd, yd = z.cuda(), y.cuda()

    def run(cuts):
        buf = eval_buffers(n, zd.device)
        for t in buf:
            t.fill_(7)
        for a, b in zip(cuts[:-1], cuts[1:]):
            eval_head(zd[a:b], yd[a:b], out=buf, offset=a)
        return buf, eval_reduce(buf)

    whole, out = run([0, n])
    for cuts in ([0, n], list(range(0, n, 1000)) + [n], [0, 1, n]):
        buf, o = run(cuts)
        assert _same(buf, whole), cuts
        assert torch.equal(_bits(o[0]), _bits(out[0])) and torch.equal(_bits(o[1]), _bits(out[1])) and torch.equal(o[2], out[2]), cuts
    # an offset call leaves the rows before it alone
    buf = eval_buffers(10, zd.device)
    for t in buf:
        t.fill_(7)
    eval_head(zd[:4], yd[:4], out=buf, offset=6)
    assert buf.pred[:6].tolist() == [7] * 6 and buf.flag[:6].tolist() == [7] * 6 and _same([t[6:] for t in buf], [t[:4] for t in whole])


@pytest.mark.parametrize("n", ec.REDUCE_N)
def test_reduce_across_the_slice_boundaries(n):
    _reduce(n, False)


def test_reduce_takes_in_the_small_rows_after_a_large_one():
    """2^24 every 1024th row, 0.75 on the others: a float32 accumulator would lose the small rows (191 bounds)."""
    assert (f"reduce n={ec.ABSORB_N} absorb", ec.ABSORB_N, True) in ec.reduce_drawn()
    _reduce(ec.ABSORB_N, True)


def _reduce(n, absorb):
    from grand_plus_amd import eval_reduce
    nll, flag, loss64, c = ec.reduce_case(n, absorb=absorb)
    buf = (nll.cuda(), torch.zeros(n, dtype=torch.int32).cuda(), flag.cuda())
    loss, acc, counts = eval_reduce(buf)
    again = eval_reduce(buf)
    assert counts.tolist() == c
    if c[0]:
        assert abs(float(loss) - loss64) <= 2.0 ** -23 * loss64      # the float64 sum, rounded once
    else:
        assert np.isnan(float(loss))
    assert (np.isnan(float(acc)) if n == 0 else float(acc) == float(np.float32(c[1] / n)))
    assert torch.equal(_bits(loss), _bits(again[0])) and torch.equal(_bits(acc), _bits(again[1]))


# ---------------------------------------------------------------------------------------------------- valid end to end
@pytest.fixture(scope="module")
def world():
    """The 2 000-node synthetic graph, its resident rows for 700 seeds (K = 32), Cora-shaped features and labels."""
    import scipy.sparse as sp
    from grand_plus_amd import Graph, synth
    from grand_plus_amd.recipes import make_coef
    from grand_plus_amd.rows import RowMatrix
    indptr, indices = synth.shape_csr("tiny")
    n = len(indptr) - 1
    seeds = synth.seeds(n, 700)
    g = Graph(indptr, indices, 0)
    rm = RowMatrix.compute(g, seeds, make_coef("ppr", 6, 0.2), 1e-5, ec.K_ROWS)
    adj = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    rng = np.random.default_rng(2)
    idx_val = torch.from_numpy(rng.permutation(np.asarray(seeds[100:600], dtype=np.int64)))      # 500 nodes, unsorted
    return {"n": n, "graph": g, "rm": rm, "adj": adj, "X": ec.features(n), "y": ec.node_labels(n), "idx_val": idx_val,
            "host_rows": (rm.col.cpu(), rm.val.cpu(), rm.filled.cpu())}


@pytest.fixture(scope="module")
def valid_refs(world):
    """Per model: (ours on the GPU, the float64 chain's results on idx_val), computed once."""
    out = {}
    pos = world["rm"].batch_positions(world["idx_val"], check=True).cpu()
    for name in ec.MODELS:
        ours, ref = ec.model_pair(name)
        out[name] = (ours.cuda(), ec.valid64(ref, world["X"], *world["host_rows"], ec.K_ROWS, pos, world["y"][world["idx_val"]]))
    return out


def _composed_logits(model, world, batch_size):
    """valid's own composition from the existing pieces, batch by batch: the logits the head gets."""
    from grand_plus_amd.augment import random_prop_rows
    rm, idx = world["rm"], world["idx_val"]
    pos = rm.batch_positions(idx, check=True)
    X = world["X"].cuda()
    model.eval()
    out = []
    with torch.no_grad():
        for s in range(0, idx.numel(), batch_size):
            aug = random_prop_rows(X, rm.col, rm.val, rm.filled, rm.K, batch_rows=pos[s:s + batch_size], training=False)
            out.append(model(aug))
    return torch.cat(out)


@pytest.mark.parametrize("batch_size", [50, 257, 10000])
@pytest.mark.parametrize("name", list(ec.MODELS))
def test_valid_end_to_end(world, valid_refs, name, batch_size, monkeypatch):
    from grand_plus_amd import evaluate, valid
    model, r64 = valid_refs[name]
    idx, y = world["idx_val"], world["y"]
    z = _composed_logits(model, world, batch_size)
    yv = y[idx]
    pred = torch.argmax(z, dim=1).cpu()
    n_correct = int((pred == yv).sum())

    modes, preds = [], []
    real_head = evaluate.eval_head

    def spy(*a, **k):
        modes.append(torch.cuda.get_sync_debug_mode())
        buf = real_head(*a, **k)
        preds.append(buf.pred)
        return buf

    monkeypatch.setattr(evaluate, "eval_head", spy)
    for training in (True, False):
        model.train(training)
        loss, acc, counts = valid(model, world["rm"], world["X"].cuda(), idx, y.cuda(), batch_size=batch_size, return_counts=True)
        assert model.training is training and torch.cuda.get_sync_debug_mode() == 0 and torch.is_grad_enabled()
    assert set(modes) == {2} and len(modes) == 2 * -(-idx.numel() // batch_size)      # "error", one head call per batch
    assert loss.is_cuda and loss.dim() == 0 and acc.is_cuda and acc.dim() == 0
    assert counts.tolist() == [idx.numel(), n_correct, 0, 0] and float(acc) == float(np.float32(n_correct / idx.numel()))
    assert torch.equal(preds[-1].cpu().long(), pred)
    ec.assert_loss(float(loss), ec.nll32_on(z, yv.cuda()), float(ec.nll64(z, yv)), f"valid {name} B={batch_size}")
    # the full float64 chain
    print(f"[evaluate] valid {name} B={batch_size}: |loss-loss64| {abs(float(loss) - r64['loss']):.3e}, bound {r64['loss_bound']:.3e}")
    assert abs(float(loss) - r64["loss"]) <= r64["loss_bound"]
    ec.assert_decided_preds(preds[-1], r64, f"valid {name} B={batch_size}")
    loss2, acc2 = valid(model, world["rm"], world["X"].cuda(), idx, y.cuda(), batch_size=batch_size)
    assert torch.equal(_bits(loss2), _bits(loss)) and torch.equal(_bits(acc2), _bits(acc))


def test_valid_at_small_running_variances_and_one_epsilon_per_layer(world):
    """The bn_norm model with infer_cases.small_var's BatchNorm state (variances from 0 to 1e-3, eps 1e-3 and 1e-5 by layer):
    valid against the float64 chain, whose bounds scale with the model as before."""
    from grand_plus_amd import valid
    ours, ref = ec.model_pair("bn_norm", small=True)
    idx, y = world["idx_val"], world["y"]
    pos = world["rm"].batch_positions(idx, check=True).cpu()
    r64 = ec.valid64(ref, world["X"], *world["host_rows"], ec.K_ROWS, pos, y[idx])
    ours = ours.cuda().eval()
    loss, acc, counts = valid(ours, world["rm"], world["X"].cuda(), idx, y.cuda(), batch_size=257, return_counts=True)
    print(f"[evaluate] valid small_var: |loss-loss64| {abs(float(loss) - r64['loss']):.3e}, bound {r64['loss_bound']:.3e}")
    assert abs(float(loss) - r64["loss"]) <= r64["loss_bound"]
    pred = torch.argmax(_composed_logits(ours, world, 257), dim=1)
    ec.assert_decided_preds(pred, r64, "valid small_var")
    assert counts.tolist() == [idx.numel(), int((pred.cpu() == y[idx]).sum()), 0, 0]


def test_valid_raises_for_a_node_that_is_no_seed(world, valid_refs):
    from grand_plus_amd import valid
    model, _ = valid_refs["plain"]
    seeds = set(world["rm"].seeds.tolist())
    stranger = next(i for i in range(world["n"]) if i not in seeds)
    model.train()
    with pytest.raises(KeyError):
        valid(model, world["rm"], world["X"].cuda(), [int(world["idx_val"][0]), stranger], world["y"].cuda())
    assert model.training and torch.cuda.get_sync_debug_mode() == 0


# -------------------------------------------------------------------------------------------------- predict end to end
@pytest.mark.parametrize("order", [0, 2])
@pytest.mark.parametrize("mode", ["ppr", "avg", "single"])
def test_predict_end_to_end(world, mode, order):
    from grand_plus_amd import predict
    ours, ref = ec.model_pair("bn_norm")
    ours = ours.cuda().train()
    n, y, X = world["n"], world["y"], world["X"]
    rng = np.random.default_rng(7)
    idx = rng.permutation(n)[:600].astype(np.int64)                  # unsorted ...
    idx[17] = idx[400]                                               # ... with a duplicate
    acc, preds = predict(world["graph"], X.cuda(), ours, idx, y.cuda(), mode, order, alpha=0.2, return_preds=True)
    assert ours.training and torch.cuda.get_sync_debug_mode() == 0
    assert acc.is_cuda and acc.dim() == 0 and preds.dtype == torch.int32 and preds.shape == (600,)
    # our own [N, C] logits, gathered on the host
    ours.eval()
    with torch.no_grad():
        z = ours(world["graph"].propagate_features(X.cuda(), mode, order, 0.2)).cpu()
    own = torch.argmax(z, dim=1)[idx]
    assert torch.equal(preds.cpu().long(), own)
    assert float(acc) == float(np.float32(int((own == y[idx]).sum()) / 600))
    assert torch.equal(_bits(predict(world["graph"], X.cuda(), ours, torch.from_numpy(idx), y.cuda(), mode, order)), _bits(acc))
    r64 = ec.predict64(ref, world["adj"], X, mode, order, 0.2, torch.from_numpy(idx), y[idx])
    ec.assert_decided_preds(preds, r64, f"predict {mode} order={order}")


@pytest.mark.parametrize("batch", [10000, 70000])
def test_predict_over_more_than_one_tile_of_rows(batch):
    from grand_plus_amd import Graph, predict, synth
    from grand_plus_amd.mlp import GrandPlusMLP
    N, F, C = 10001, 16, 5
    indptr, indices = synth.powerlaw_csr(N, 40000)
    g = Graph(indptr, indices, 0)
    gen = torch.Generator().manual_seed(21)
    X = torch.randn((N, F), generator=gen).cuda()
    y = torch.randint(0, C, (N,), generator=gen)
    torch.manual_seed(3)
    model = GrandPlusMLP(F, C, 32, 2, True, 0.0, 0.0, True).cuda()
    idx = torch.cat([torch.arange(N - 1, 9990, -1), torch.randint(0, N, (500,), generator=gen)])   # the last tile's rows first
    acc, preds = predict(g, X, model, idx, y.cuda(), "ppr", 2, batch_size_logits=batch, return_preds=True)
    model.eval()
    with torch.no_grad():
        prop = g.propagate_features(X, "ppr", 2, 0.2)
        z = torch.cat([model(prop[s:s + batch]) for s in range(0, N, batch)]).cpu()
    own = torch.argmax(z, dim=1)[idx]
    assert torch.equal(preds.cpu().long(), own)
    assert float(acc) == float(np.float32(int((own == y[idx]).sum()) / idx.numel()))
