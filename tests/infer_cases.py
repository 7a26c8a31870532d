"""Shapes, model builders and bounds shared by tests/test_gpu_infer.py and tests/test_host_infer.py.

Models are built as tests/test_gpu_mlp.py builds them (non-trivial BatchNorm affine maps and running statistics, a
float64 twin from oracle/mlp_ref.py); the output rule is that file's: per output
|got - ref64| <= 2e-5 * (|a_last| |W|^T + |b|) + 1e-6, a_last the last Linear's input in float64, and all outputs finite."""
import functools

import numpy as np
import torch

from oracle.mlp_ref import RefMagMLP, RefMLP
from oracle.predict_ref import propagate_ref

# (name, layout, F, H, C, nlayers, use_bn, node_norm): tests/test_gpu_mlp.py's CASES (the run_*.sh shapes, a three-layer
# one at F = 7, the two MAG layouts) without their dropout rates and batch sizes, which an eval pass does not use
CASES = [
    ("cora", "model", 1433, 64, 7, 2, False, False),
    ("citeseer", "model", 3703, 256, 6, 2, False, False),
    ("pubmed", "model", 500, 16, 3, 1, True, True),
    ("reddit", "model", 602, 512, 41, 2, True, True),
    ("amazon2m", "model", 100, 1024, 47, 2, True, True),
    ("aminer", "model", 100, 32, 18, 1, True, False),
    ("deep", "model", 7, 100, 5, 3, True, True),
    ("mag", "mag", 64, 64, 8, 2, False, False),
    ("mag_bn", "mag", 64, 64, 8, 3, True, True),
]
CASE_ROWS = (1, 129, 1000)

# where gp_mlp_block_forward takes one k-chain per output (f_in <= 64 in every layer): infer must give its bits
BITWISE = [
    ("mag_bn", "mag", 64, 64, 8, 3, True, True),
    ("deep33_bn_norm", "model", 7, 33, 5, 3, True, True),
    ("deep33_plain", "model", 7, 33, 5, 3, False, False),
    ("f48", "model", 48, 64, 7, 2, True, False),
]
BITWISE_ROWS = (1, 127, 128, 129, 257, 300)
# ... and one layer at K = 200 with 4096 / 64 * 128 / 64 = 128 tiles of 64 x 64, where the block path does not split either
TILE_COUNT = ("tiles128", "model", 200, 0, 128, 1, True, True)

CHUNK = ("deep33_bn_norm", "model", 7, 33, 5, 3, True, True)        # row independence and chunking, B = 385
EDGE_ROWS = 130
EDGE_SHAPES = sorted({(fi, fo) for fi in (1, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100) for fo in (5, 130)} |
                     {(fi, fo) for fo in (1, 47, 48, 49, 63, 64, 65, 127, 128, 129, 200) for fi in (17, 96)})


# ---- eval BatchNorm where its epsilon decides (tests/test_host_mutants.py): running variances from 0 to 1e-3 in every third
# column, those columns' running means scaled down by 1e-3 (a mean of 0.1 over sqrt(1e-7) would be all the column holds), and
# one epsilon per layer.  The first rows of the inputs are special too, see `inputs`.
SMALL_VARS = (0.0, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3)
SMALL_EPS = (1e-3, 1e-5, 1e-7)
SMALL_ROWS = 129
SMALL_VAR = [
    ("deep", "model", 7, 100, 5, 3, True, True),
    ("mag_bn", "mag", 64, 64, 8, 3, True, True),
    ("17-130-5", "model", 17, 130, 5, 2, True, True),
]
SMALL_VAR_TILE32 = (("17-1024-5", "model", 17, 1024, 5, 2, True, True), 33)      # the chain's 32-row tile, B = 33
SMALL_DRAWN = [(c, SMALL_ROWS) for c in SMALL_VAR] + [SMALL_VAR_TILE32]
# what tests/test_gpu_infer.py holds to the float64 rule: (case, rows, with small variances)
DRAWN = [(c, B, False) for c in CASES for B in CASE_ROWS] + [(c, B, True) for c, B in SMALL_DRAWN]
SMALL_VAR_BITWISE =[c for c in SMALL_VAR if max(c[2] if c[1] == "model" else c[3], c[3]) <= 64]    # f_in <= 64 in every layer


def small_var(*models):
    """Gives the BatchNorms of `models` (built alike) the small running variances and the per-layer epsilons, in place."""
    for m in models:
        for i, b in enumerate(m.bns):
            cols = torch.arange(0, b.running_var.numel(), 3)
            var = torch.tensor(SMALL_VARS, dtype=torch.float32)[torch.arange(cols.numel()) % len(SMALL_VARS)]
            b.running_var.data[cols] = var.to(b.running_var.dtype)                     # float32 values in the float64 twin too
            b.running_mean.data[cols] = (b.running_mean.data[cols].float() * 1e-3).to(b.running_mean.dtype)
            b.eps = SMALL_EPS[i]
    return models


def small_pair(case, seed=0):
    ours, ref = pair(case, seed)
    small_var(ours, ref)
    return ours, ref


def small_inputs(case, B, seed=7):
    """`inputs`, but row 1 has a norm of 1e-12, the epsilon of node_norm: 1 / (1e-12 + L) is half of 1 / max(L, 1e-12)."""
    X = inputs(case, B, seed)
    if B > 1:
        X[1] *= 1e-12 / float(X[1].double().norm())
        if case[1] != "model":
            X[1] = X[1].abs()                                # the MAG layout's first block begins with ReLU
    return X


# ---- the eval MLP written out in float64, and one deliberate mistake
MUTANTS = ("eps_x2", "eps_default", "eps_outside_sqrt", "eps_swapped", "norm_max", "bn_before_norm", "relu_after_norm", "mean_sign")


def manual64(ref, X, mut=None, dtype=torch.float64):
    """(logits, the last Linear's input) of the restatement `ref` (RefMLP or RefMagMLP, eval mode) on X from explicit
    formulas (mut None), or with one of MUTANTS built in.  In float32 it is the kernels' documented arithmetic (DESIGN
    §7j): r = 1 / (1e-12 + |relu?(x)|), mul = gamma * is, add = beta - mean * mul, a = (relu?(x) * r) * mul + add."""
    mag = isinstance(ref, RefMagMLP)
    f32 = dtype == torch.float32
    eps = [b.eps for b in ref.bns]
    if mut == "eps_swapped" and len(eps) >= 2:
        eps[-1], eps[-2] = eps[-2], eps[-1]
    h = X.to(dtype)
    a = None
    with torch.no_grad():
        for i, (fc, bn) in enumerate(zip(ref.fcs, ref.bns)):
            relu = mag or i > 0

            def norm(v):
                L = v.norm(dim=-1, keepdim=True)
                return v * (1.0 / L.clamp(min=1e-12) if mut == "norm_max" else 1.0 / (1e-12 + L))

            def bnorm(v):
                e = {"eps_x2": 2 * eps[i], "eps_default": 1e-5}.get(mut, eps[i])
                var, mean = bn.running_var.to(dtype), bn.running_mean.to(dtype)
                istd = 1.0 / (var.sqrt() + e) if mut == "eps_outside_sqrt" else 1.0 / (var + e).sqrt()
                gamma, beta = bn.weight.to(dtype), bn.bias.to(dtype)
                if f32:
                    mul = gamma * istd
                    return v * mul + (beta - mean * mul)
                return (v + mean if mut == "mean_sign" else v - mean) * istd * gamma + beta

            steps = []
            if relu and mut != "relu_after_norm":
                steps.append(torch.relu)
            if ref.node_norm:
                steps.append(norm)
            if relu and mut == "relu_after_norm":
                steps.append(torch.relu)
            if ref.use_bn:
                steps.append(bnorm)
            if mut == "bn_before_norm" and ref.use_bn and ref.node_norm:
                steps[-1], steps[-2] = steps[-2], steps[-1]
            for f in steps:
                h = f(h)
            a = h
            h = a @ fc.weight.to(dtype).t() + fc.bias.to(dtype)
    return h, a


def share(got, want, bound):
    """max |got - want| / bound of the rule; a non-finite entry counts as infinite."""
    r = ((got.double() - want).abs() / bound).max()
    return float(r) if bool(torch.isfinite(r)) else float("inf")


def pair(case, seed=0):
    """(ours on the CPU, the float64 restatement on the CPU in eval mode), same parameters and running statistics."""
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    _, layout, F, H, C, nl, bn, norm = case
    torch.manual_seed(seed)
    ours = (GrandPlusMLP if layout == "model" else MagMLP)(F, C, H, nl, bn, 0.3, 0.4, norm)
    g = torch.Generator().manual_seed(seed + 1)
    for b in ours.bns:
        b.weight.data = torch.rand(b.weight.shape, generator=g) + 0.5
        b.bias.data = torch.randn(b.bias.shape, generator=g) * 0.1
        b.running_mean.data = torch.randn(b.running_mean.shape, generator=g) * 0.1
        b.running_var.data = torch.rand(b.running_var.shape, generator=g) + 0.5
    ref = (RefMLP if layout == "model" else RefMagMLP)(F, C, H, nl, bn, 0.3, 0.4, norm)
    ref.load_state_dict(ours.state_dict())
    return ours, ref.double().eval()


def in_features(case):
    """Columns of the input: F for model.py's layout, the hidden size for the MAG layout (its input is the embedding)."""
    return case[2] if case[1] == "model" else case[3]


def inputs(case, B, seed=7):
    """X float32 [B, F] on the CPU; bag-of-words like (sparse) rows for the wide first layers, as tests/test_gpu_mlp.py."""
    F = in_features(case)
    g = torch.Generator().manual_seed(seed)
    X = torch.randn((B, F), generator=g)
    if case[1] == "model" and F > 100:
        X = X * (torch.rand((B, F), generator=g) < 0.1)
    return X


def ref_out(ref, X64):
    """(float64 logits, the per-output bound of the rule) of the restatement on X64, wherever X64 lives."""
    with torch.no_grad():
        out = ref(X64, None)
        fc = ref.fcs[-1]
        bound = 2e-5 * (ref.last_a.abs() @ fc.weight.abs().t() + fc.bias.abs()) + 1e-6
    return out, bound


def assert_rule(got, ref64, bound, what=""):
    err = (got.double() - ref64).abs()
    print(f"[infer] {what}: max err {float(err.max()):.3e}, max err / bound {float((err / bound).max()):.3g}")
    bad = err > bound
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs off, max err {float(err.max()):.3g}"
    assert bool(torch.isfinite(got).all()), what


def single_layer(f_in, f_out, seed=0):
    """One Linear without BatchNorm or node_norm, as a GrandPlusMLP (CPU)."""
    from grand_plus_amd.mlp import GrandPlusMLP
    torch.manual_seed(seed + 1000 * f_in + f_out)
    return GrandPlusMLP(f_in, f_out, 0, 1, False, 0.0, 0.0, False)


# ---- the predict world: a power-law graph of 10 001 nodes (more than one batch of 10 000 rows)
N_NODES, N_EDGES = 10001, 40000
SMALL = ("f48_graph", "model", 48, 64, 7, 2, True, True)            # bitwise against predict's batch loop
REDDIT = ("reddit_graph", "model", 602, 512, 41, 2, True, True)     # against the float64 chain
# The reddit-shaped model's weights are scaled up, its BatchNorm offsets down and its first bias shifted (a sparse hidden
# layer) so that the predictions spread over the classes and, in float64 on the CPU alone, no row's top-2 gap is inside twice the rule's bound (tests/test_host_infer.py asserts that with no GPU); the GPU test allows
# LEFT_OUT of the rows, asserted first.
REDDIT_SEED, REDDIT_FIRST_SCALE, REDDIT_LAST_SCALE, REDDIT_BN_OFFSET, REDDIT_BIAS_SHIFT = 50, 8.0, 8.0, 0.02, -0.6
LEFT_OUT = 0.01


@functools.lru_cache(maxsize=None)
def graph_csr():
    from grand_plus_amd import synth
    return synth.powerlaw_csr(N_NODES, N_EDGES)


def graph_features(F, seed=21):
    return torch.randn((N_NODES, F), generator=torch.Generator().manual_seed(seed + F))


def graph_labels(C, seed=22):
    return torch.randint(0, C, (N_NODES,), generator=torch.Generator().manual_seed(seed))


def query_ids(seed=23):
    """600 node ids, unsorted, with a duplicate, the last rows first."""
    idx = np.random.default_rng(seed).permutation(N_NODES)[:600].astype(np.int64)
    idx[0] = N_NODES - 1
    idx[17] = idx[400]
    return idx


def reddit_pair():
    ours, ref = pair(REDDIT, seed=REDDIT_SEED)
    for b in ours.bns:                                       # node_norm leaves entries of about F^-1/2: keep the offsets below them
        b.bias.data *= REDDIT_BN_OFFSET
        b.running_mean.data *= REDDIT_BN_OFFSET
    ours.fcs[0].weight.data *= REDDIT_FIRST_SCALE
    ours.fcs[0].bias.data += REDDIT_BIAS_SHIFT              # few hidden units active per row: little cancellation in the logits
    ours.fcs[-1].weight.data *= REDDIT_LAST_SCALE
    ref.load_state_dict(ours.state_dict())
    return ours, ref.double().eval()


@functools.lru_cache(maxsize=None)
def reddit_chain64(mode="ppr", order=2, alpha=0.2):
    """The float64 chain propagate_ref -> RefMLP over every node, on the CPU, once: (pred [N], decided [N]); a row is
    decided when its float64 top-2 gap exceeds twice the largest bound the rule allows one of its logits."""
    import scipy.sparse as sp
    indptr, indices = graph_csr()
    adj = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(N_NODES, N_NODES))
    _, ref = reddit_pair()
    prop = torch.from_numpy(propagate_ref(adj, graph_features(REDDIT[2]).numpy(), mode, order, alpha))
    z, bound = ref_out(ref, prop)
    top2 = torch.topk(z, 2, dim=1).values
    return z.argmax(dim=1), (top2[:, 0] - top2[:, 1]) > 2.0 * bound.max(dim=1).values
