"""Shapes, inputs and the host-number step shared by the tests of the captured training step (DESIGN §7m,
tests/test_gpu_captured_step.py).

One resident matrix for every case: 96 rows with K = 8 over 256 nodes, `filled` drawn from {0, 3, 8}; C = 5 classes.
The two pools are the first 20 rows' nodes (labelled) and the other 76 (unlabelled).  `host_step` is the composition the
end-to-end tests use today -- random_prop_rows(seed) -> model(seed) -> grand_plus_loss(weight) -> backward -> ClipAdam --
with every step number formed on the host: step_seed(base, t), the weight of model.py:329 and Adam's step count t.
"""
import functools

import numpy as np
import torch

N_NODES, S_ROWS, K, C, F = 256, 96, 8, 5, 33
N_TRAIN = 20
BASE_SEED, LAM, WARMUP, TEM, P_NODE, CONF = 0x5EED0FACADE, 0.8, 4, 0.5, 0.5, 0.22
HYPER = dict(lr=1e-2, weight_decay=5e-4, clip=0.1)                  # optim_cases.HYPERS[0]: clipping active

# name: hidden size, layers, use_bn / node_norm, input dropout, hidden dropout, loss
LAYOUTS = {
    "cora": (16, 2, False, 0.5, 0.7, "l2"),                         # two layers, input dropout, no BN
    "reddit": (16, 2, True, 0.0, 0.5, "kl"),                        # two layers, BN, hidden dropout only
    "pubmed": (16, 1, True, 0.2, 0.2, "l2"),                        # one layer with BN
}


@functools.lru_cache(maxsize=None)
def problem():
    """The CPU tensors every case shares: (seeds, col, val, filled, features, labels)."""
    rng = np.random.default_rng(11)
    seeds = rng.permutation(N_NODES)[:S_ROWS].astype(np.int64)
    col = rng.integers(0, N_NODES, S_ROWS * K).astype(np.int32)
    val = np.sort(rng.random((S_ROWS, K)) ** 2, axis=1)[:, ::-1].copy().reshape(-1)
    filled = rng.choice(np.array([0, 3, 8], np.int32), S_ROWS)
    filled[:4] = (8, 3, 0, 8)                                       # each kind among the labelled rows, too
    filled[N_TRAIN:N_TRAIN + 3] = (0, 3, 8)
    gen = torch.Generator().manual_seed(12)
    X = torch.randn((N_NODES, F), generator=gen)
    labels = torch.randint(0, C, (N_NODES,), generator=gen)
    return seeds, torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(filled), X, labels


def resident(dev="cuda"):
    """(RowMatrix, features, labels) on the device."""
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, X, labels = problem()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    rm = RowMatrix(seeds, K, row.to(dev), col.to(dev), val.to(dev), filled.to(dev), N_NODES)
    return rm, X.to(dev), labels.to(dev)


def pools():
    seeds = problem()[0]
    return seeds[:N_TRAIN], seeds[N_TRAIN:]


def model(name, dev="cuda"):
    from grand_plus_amd.mlp import GrandPlusMLP
    H, nl, bn, p_in, p_hid, _kind = LAYOUTS[name]
    torch.manual_seed(5)
    return GrandPlusMLP(F, C, H, nl, bn, p_in, p_hid, bn).to(dev).train()


def selection(t, n_l=8, n_u=24):
    """The selections of step t into the two pools: (train_sel, unlabel_sel), different for every t."""
    rng = np.random.default_rng(1000 + t)
    return rng.choice(N_TRAIN, n_l, replace=False), rng.choice(S_ROWS - N_TRAIN, n_u, replace=False)


def optimizer(params, capturable):
    """ClipAdam with HYPER; capturable: over a fresh StepState on the parameters' device."""
    import optim_cases as oc
    from grand_plus_amd import ClipAdam, StepState
    kw = dict(capturable=True, state=StepState(params[0].device)) if capturable else {}
    return ClipAdam(params, lr=HYPER["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=HYPER["weight_decay"],
                    clip_norm=HYPER["clip"], **kw)


def train_step(name, capture, S=2, dev="cuda", resident_=None):
    """(TrainStep, model, optimizer) of a layout over the shared problem."""
    from grand_plus_amd import TrainStep
    from grand_plus_amd.step import trained_parameters
    rm, X, labels = resident_ or resident(dev)
    m = model(name, dev)
    opt = optimizer(trained_parameters(m), True)
    tr, un = pools()
    ts = TrainStep(m, opt, rm, X, labels, tr, un, samples=S, dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM,
                   conf=CONF, kind=LAYOUTS[name][5], seed=BASE_SEED, capture=capture)
    return ts, m, opt


def host_step(m, opt, rm, X, labels, pos, t, sel, name, S=2):
    """Step t of the composition of today with host numbers; `pos`: the positions of both pools, labelled first.
    Returns the gradients of the step (CPU clones, in the optimiser's parameter order)."""
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.step import step_weight
    tr, un = sel
    seed, w = step_seed(BASE_SEED, t), float(step_weight(LAM, WARMUP, t))
    idx = torch.from_numpy(np.concatenate([tr, un + N_TRAIN])).to(X.device)
    batch_rows = pos[idx]
    y = labels[torch.from_numpy(pools()[0][tr]).to(X.device)]
    opt.zero_grad(set_to_none=True)
    aug = random_prop_rows(X, rm.col, rm.val, rm.filled, rm.K, batch_rows=batch_rows, dropnode_rate=P_NODE, training=True,
                           seed=seed, samples=S)
    loss, _ = grand_plus_loss(m(aug, seed=seed), y, len(tr), w, tem=TEM, conf=CONF, kind=LAYOUTS[name][5])
    loss.backward()
    grads = [p.grad.detach().cpu().clone() for g in opt.param_groups for p in g["params"]]
    opt.step()
    return grads


def snapshot(m, opt):
    """Everything a step changes, as clones: parameters, Adam's moments, BatchNorm's running statistics and counters."""
    ps = [p for g in opt.param_groups for p in g["params"]]
    out = [p.detach().clone() for p in ps]
    out += [opt.state[p][k].clone() for p in ps for k in ("exp_avg", "exp_avg_sq")]
    out += [b.clone() for _n, b in sorted(m.named_buffers())]
    return out
