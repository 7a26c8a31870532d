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


def model_pair(name, seed=11, f_in=F_IN):
    """(GrandPlusMLP on the CPU, its float64 restatement), equal parameters, non-trivial BatchNorm state."""
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
