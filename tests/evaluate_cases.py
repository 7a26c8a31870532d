"""Inputs, references and bounds shared by tests/test_gpu_evaluate.py and tests/test_host_evaluate.py.

The references are torch's own `F.nll_loss(F.log_softmax(z))` in float64 on the CPU for the head, and for the end-to-end
checks the float64 chain of the oracles: `oracle.random_prop_ref` (or `oracle.predict_ref.propagate_ref`) ->
`oracle.mlp_ref.RefMLP` -> log-softmax -> argmax.  Everything here runs on the CPU and is computed once per case."""
import functools

import numpy as np
import torch
import torch.nn.functional as Fn

from augment_cases import rows_to_coo
from oracle.mlp_ref import RefMLP
from oracle.objective_ref import grand_loss_ref
from oracle.predict_ref import propagate_ref
from oracle.random_prop_ref import random_prop_ref

HEAD_C = (1, 3, 7, 64, 65, 349)
HEAD_N = (1, 63, 64, 65, 4097)
WRONG, CORRECT, IGNORED, BAD = 0, 1, 2, 3

# Cora's shape (run_cora.sh): F, hidden, classes, layers; K of the rows; the two models of the end-to-end tests as
# (use_bn, node_norm).  FIRST_SCALE and LAST_SCALE multiply the first and last layer's weights so that the predictions
# spread over the classes and float64 top-2 logit gaps are far above the fp32 error bound for all but a few rows
# (asserted before every prediction comparison: at most LEFT_OUT of them).
F_IN, HIDDEN, CLASSES, LAYERS, K_ROWS = 1433, 64, 7, 2, 32
MODELS = {"plain": (False, False), "bn_norm": (True, True)}
FIRST_SCALE, LAST_SCALE = 8.0, 4.0
LEFT_OUT = 0.01


@functools.lru_cache(maxsize=None)
def head_case(n, C):
    """(z float32 [n, C], y int64 [n], ref64): random logits of a few units, labels in [0, C), torch's float64 loss."""
    g = torch.Generator().manual_seed(1000 * C + n)
    z = torch.randn((n, C), generator=g) * 3.0
    y = torch.randint(0, C, (n,), generator=g)
    return z, y, float(nll64(z, y))


def nll64(z, y, ignore_index=-100):
    return Fn.nll_loss(Fn.log_softmax(z.double().cpu(), dim=-1), y.cpu(), ignore_index=ignore_index)


def nll32_on(z, y, ignore_index=-100):
    """The same torch call in float32 where z lives (the GPU in the tests): what the project's rule measures ours by."""
    return float(Fn.nll_loss(Fn.log_softmax(z, dim=-1), y, ignore_index=ignore_index))


def assert_loss(ours, torch32, ref64, what):
    """§7g's rule: |ours - ref64| <= 4 |torch32 - ref64| + 2^-23 |ref64|.  Prints the ratio ours / torch32 first."""
    e_ours, e_t = abs(ours - ref64), abs(torch32 - ref64)
    print(f"[evaluate] {what}: |ours-ref64| {e_ours:.3e}  |torch32-ref64| {e_t:.3e}  ratio {e_ours / e_t if e_t else float('nan'):.3g}")
    assert e_ours <= 4.0 * e_t + 2.0 ** -23 * abs(ref64), (what, ours, torch32, ref64)


def ties_case():
    """(z [8, 349], y): ties across lanes and passes, NaNs, a row of -inf and one +inf; labels ignored but for four rows."""
    C = 349
    z = torch.randn((8, C), generator=torch.Generator().manual_seed(5))
    z[0, [0, 63, 64]] = 9.0                                  # lanes 0 / 63 and the second pass of lane 0
    z[1, [63, 64]] = 9.0
    z[2, [64, 128, 320]] = 9.0                               # the same lane, three passes
    z[3, [348, 100]] = 9.0
    z[4, 70] = float("nan"); z[4, 5] = float("nan")          # the first NaN wins
    z[5, 64] = float("nan"); z[5, 3] = 50.0                  # a NaN beats every number
    z[6, :] = float("-inf")                                  # all equal: index 0
    z[7, 10] = float("inf")
    y = torch.full((8,), -100, dtype=torch.int64)            # ignored: the loss of a NaN row is not the subject here
    y[:4] = torch.tensor([0, 63, 64, 100])
    return z, y


def ignored_case():
    """(z [300, 7], clean labels, labels with ignored and bad entries, rows, label_rows, ignored positions, bad positions)."""
    n, C = 300, 7
    z, y, _ = head_case(4097, C)
    z, y = z[:n].clone(), y[:n].clone()
    y2 = y.clone()
    y2[[3, 77]] = -100                                       # ignore_index
    y2[[5, 100]] = torch.tensor([C, -1])                     # labels outside [0, C)
    y2[200] = 2 ** 40
    rows, lrows = torch.arange(n), torch.arange(n)
    rows[[9, 10]] = torch.tensor([n, -1])                    # a logits row outside the array
    lrows[[11, 12]] = torch.tensor([n, -(2 ** 50)])          # a label index outside the array
    return z, y, y2, rows, lrows, [3, 77], [5, 100, 200, 9, 10, 11, 12]


# ---- the head written out in float64, and one deliberate mistake (tests/test_host_mutants.py)
MUTANTS = ("acc_over_valid", "loss_over_rows", "tie_last_index", "nan_not_max", "ignored_in_loss")


def head64(z, y, rows=None, label_rows=None, ignore_index=-100, mut=None):
    """What eval_head + eval_reduce must give, on the CPU in float64: {"pred", "flag", "counts", "acc", "loss"}; mut None, or
    one of MUTANTS built in.  A row whose logits row, label index or label is outside its array is BAD (pred -1 without a
    logits row); a label equal to ignore_index is IGNORED; acc is over all rows, the loss over the others alone."""
    z, y = z.double(), y.long()
    n = rows.numel() if rows is not None else label_rows.numel() if label_rows is not None else z.shape[0]
    C = z.shape[1]
    rows = torch.arange(n) if rows is None else rows.long()
    lrows = torch.arange(n) if label_rows is None else label_rows.long()
    pred, flag = torch.full((n,), -1, dtype=torch.int64), torch.full((n,), BAD, dtype=torch.uint8)
    total, n_valid = 0.0, 0
    for i in range(n):
        r, l = int(rows[i]), int(lrows[i])
        if not 0 <= r < z.shape[0]:
            continue
        row = z[r]
        nan = torch.isnan(row)
        if bool(nan.any()) and mut != "nan_not_max":
            pred[i] = int(nan.nonzero()[0])                  # the first NaN, as torch.argmax and numpy
        else:
            v = torch.where(nan, torch.full_like(row, float("-inf")), row)
            hits = (v == v.max()).nonzero()[:, 0]
            pred[i] = int(hits[-1] if mut == "tie_last_index" else hits[0])
        if not 0 <= l < y.numel():
            continue
        label = int(y[l])
        if label == ignore_index:
            flag[i] = IGNORED
            if mut == "ignored_in_loss":                      # a head that gathers before it tests the label: class 0
                total, n_valid = total - float(torch.log_softmax(row, dim=0)[0]), n_valid + 1
            continue
        if not 0 <= label < C:
            continue
        flag[i] = CORRECT if int(pred[i]) == label else WRONG
        total -= float(torch.log_softmax(row, dim=0)[label])
    counts = [int((flag <= CORRECT).sum()), int((flag == CORRECT).sum()), int((flag == IGNORED).sum()), int((flag == BAD).sum())]
    n_valid += counts[0]
    den_loss = n if mut == "loss_over_rows" else n_valid
    den_acc = counts[0] if mut == "acc_over_valid" else n
    return {"pred": pred, "flag": flag, "counts": counts, "acc": counts[1] / den_acc if den_acc else float("nan"),
            "loss": total / den_loss if den_loss else float("nan")}


def head_share(got, ref, loss32, loss_held=True):
    """How far `got` (a head64 result) is from `ref` under the GPU file's assertions: infinite when a quantity the file
    holds exactly differs (pred, flag, counts, acc, a NaN loss), otherwise |loss - loss64| over assert_loss's bound, or 0
    where the file does not look at the loss (`loss_held`)."""
    same = lambda a, b: a == b or (a != a and b != b)  # noqa: E731
    if not (torch.equal(got["pred"], ref["pred"]) and torch.equal(got["flag"], ref["flag"]) and got["counts"] == ref["counts"]
            and same(got["acc"], ref["acc"])):
        return float("inf")
    if not loss_held:
        return 0.0
    if ref["loss"] != ref["loss"] or got["loss"] != got["loss"] or got["loss"] == ref["loss"]:
        return 0.0 if same(got["loss"], ref["loss"]) else float("inf")
    return abs(got["loss"] - ref["loss"]) / (4.0 * abs(loss32 - ref["loss"]) + 2.0 ** -23 * abs(ref["loss"]))


def head_drawn():
    """The head's inputs that tests/test_gpu_evaluate.py draws, up to 65 rows of the grid (the reference walks row by row):
    (name, z, y, {rows, label_rows, ignore_index}, whether the file holds the loss there)."""
    out = [(f"head C={C} n={n}", *head_case(n, C)[:2], {}, True) for C in HEAD_C for n in HEAD_N if n <= 65]
    z, y = ties_case()
    out.append(("ties", z, y, {}, False))
    z, _, y2, rows, lrows, _, _ = ignored_case()
    out.append(("ignored", z, y2, dict(rows=rows, label_rows=lrows), True))
    out.append(("all ignored", z, torch.full((z.shape[0],), 3), dict(ignore_index=3), True))
    return out


def reduce_case(n, seed=0):
    """Synthetic filled buffers (nll float32, flag uint8) and what the reduce must give: (nll, flag, loss64, counts)."""
    rng = np.random.default_rng(seed + n)
    flag = rng.integers(0, 4, n).astype(np.uint8)
    nll = (rng.random(n) * 5.0).astype(np.float32)
    nll[flag >= IGNORED] = 0.0
    counts = [int((flag <= CORRECT).sum()), int((flag == CORRECT).sum()), int((flag == IGNORED).sum()), int((flag == BAD).sum())]
    loss = float(np.sum(nll.astype(np.float64))) / counts[0] if counts[0] else float("nan")
    return torch.from_numpy(nll), torch.from_numpy(flag), loss, counts


def features(n_nodes, seed=3):
    """Bag-of-words like node features, 5 % non-zero, of either sign: the rows' average carries no common offset that
    would send every node to the same class."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((n_nodes, F_IN), generator=g) < 0.05).float() * torch.sign(torch.randn((n_nodes, F_IN), generator=g))


def node_labels(n_nodes, seed=4):
    return torch.randint(0, CLASSES, (n_nodes,), generator=torch.Generator().manual_seed(seed))


def model_pair(name, seed=11, f_in=F_IN, small=False):
    """(GrandPlusMLP on the CPU, its float64 restatement), equal parameters, non-trivial BatchNorm state; with `small`,
    infer_cases.small_var's running variances and per-layer epsilons."""
    from grand_plus_amd.mlp import GrandPlusMLP
    use_bn, norm = MODELS[name]
    torch.manual_seed(seed)
    ours = GrandPlusMLP(f_in, CLASSES, HIDDEN, LAYERS, use_bn, 0.5, 0.7, norm)
    g = torch.Generator().manual_seed(seed + 1)
    for b in ours.bns:
        b.weight.data = torch.rand(b.weight.shape, generator=g) + 0.5
        b.bias.data = torch.randn(b.bias.shape, generator=g) * 0.01
        b.running_mean.data = torch.randn(b.running_mean.shape, generator=g) * 0.01
        b.running_var.data = torch.rand(b.running_var.shape, generator=g) + 0.5
    ours.fcs[0].weight.data *= FIRST_SCALE
    ours.fcs[-1].weight.data *= LAST_SCALE
    ref = RefMLP(f_in, CLASSES, HIDDEN, LAYERS, use_bn, 0.5, 0.7, norm)
    ref.load_state_dict(ours.state_dict())
    if small:
        from infer_cases import small_var
        small_var(ours, ref)
    return ours, ref.double().eval()


def chain64(ref, x64, y):
    """The float64 end of both chains on the CPU: logits of the restatement in eval mode on x64, then what the tests hold
    ours against.  Returns a dict:
      loss, pred      float64 nll_loss and argmax;
      dz [n]          per row, the largest error the MLP test (tests/test_gpu_mlp.py) allows a logit of ours:
                      max_c 2e-5 * (|a| |W|^T + |b|)_c + 1e-6, a = the last Linear's input;
      loss_bound      log-softmax moves by at most 2 max_c |dz_c| per row (log-sum-exp is 1-Lipschitz in the sup norm, and
                      z_y moves by at most the same), so the mean moves by at most mean_i 2 dz_i; the head's own fp32
                      arithmetic (z - max, log of the sum, the final subtraction: three roundings of at most 2 ulp) adds
                      at most 2^-22 * mean_i (|z_y - max| + |log sum|);
      decided [n]     rows whose float64 top-2 gap exceeds 2 dz_i: no logits within the bound can change their argmax."""
    with torch.no_grad():
        z = ref(x64, None)
        fc = ref.fcs[-1]
        scale = ref.last_a.abs() @ fc.weight.abs().t() + fc.bias.abs()
    dz = (2e-5 * scale + 1e-6).max(dim=1).values
    top2 = torch.topk(z, 2, dim=1).values if z.shape[1] > 1 else torch.cat([z, z - 1.0], dim=1)
    m = z.max(dim=1).values
    lse = torch.log(torch.exp(z - m[:, None]).sum(dim=1))
    zy = z.gather(1, y[:, None])[:, 0]
    head = 2.0 ** -22 * float(((zy - m).abs() + lse.abs()).mean())
    sup = grand_loss_ref([z], y, y.numel(), 0.0, 1.0, 0.0, "l2")[1]      # the supervised term of the objective's restatement
    return {"loss": float(sup), "pred": z.argmax(dim=1), "dz": dz,
            "loss_bound": float((2.0 * dz).mean()) + head, "decided": (top2[:, 0] - top2[:, 1]) > 2.0 * dz}


def valid64(ref, X, col, val, filled, K, positions, y):
    """The reference's valid() in float64: random_prop (eval mode) over the rows at `positions`, then chain64."""
    idx, cols, scores, _ = rows_to_coo(col, val, filled, K, positions)
    n_out = positions.numel()
    if int(idx[-1]) + 1 != n_out:                         # random_prop_ref sizes its output by the last entry
        raise ValueError("the last row of the batch is empty")
    aug = random_prop_ref(X.double()[cols], scores.double(), idx, 0.5, False)
    return chain64(ref, aug, y)


def predict64(ref, adj, X, mode, order, alpha, idx, y):
    """The reference's predict() in float64 on the rows idx."""
    prop = torch.from_numpy(propagate_ref(adj, X.numpy(), mode, order, alpha))
    return chain64(ref, prop[idx], y)


def assert_decided_preds(pred, r64, what):
    """At most LEFT_OUT of the rows may be undecided in float64 (asserted first); on every other row pred must match."""
    left_out = 1.0 - float(r64["decided"].double().mean())
    print(f"[evaluate] {what}: {left_out:.4f} of the rows within the margin")
    assert left_out <= LEFT_OUT, (what, left_out)
    d = r64["decided"]
    assert torch.equal(pred.cpu().long()[d], r64["pred"][d]), what
