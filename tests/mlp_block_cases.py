"""One MLP block, its float64 twin and the bounds: shared by tests/test_gpu_mlp_block.py and
tests/test_host_mlp_block.py.

    block(x) = Linear( dropout_p( BN( node_norm( relu?(x) ) ) ) )      on x [S, B, F], BatchNorm per sample

`build` makes a case's tensors and modules on the CPU from one torch.Generator; `block_ref` is the block with plain torch
ops through autograd, in float64 (`block_ref64`, the reference) or float32 (the headroom restatement); `block_manual64`
is the same block with its backward written out, and takes the name of one deliberate mistake (MUTANTS) for the
sensitivity proof.  Bounds (`bounds`):

    out         |d| <= 2e-5 * (|a| |W|^T + |b|) + 1e-6                 the project's output rule, a = the Linear's input
    dW, db      |d| <= 2e-5 * sum_m |dY[m,n] a[m,k]| + 1e-6,  2e-5 * sum_m |dY[m,n]| + 1e-6        plain fma sums as well
    dX, dgamma, dbeta   |d| <= 1e-5 * (|ref| + max|ref|) + 1e-9        through cancellation: scaled by the tensor
                        (dX at F = 1 under NORM is zero in exact arithmetic: there max|ref| is max|r g|, see `bounds`)
    running statistics  |d| <= 1e-5 * |ref| + 1e-6;  num_batches_tracked exact

Cases with B = 2 under BN|TRAINING keep test_gpu_mlp._assert_grad's 1e-4 * (|ref| + max|ref|) + 1e-9 for dX and dW: with
two rows per sample xhat is +-1 and dn = ((dy - mean dy) - xhat * mean(dy * xhat)) * c is the difference of two nearly
equal numbers, so float32 torch itself uses up to 0.28 of that rule for dX here (tests/test_host_mlp_block.py prints it).
B = 3 stays on the tight rules; under RELU its columns are built to be well conditioned (see `_special`).
"""
import collections
import copy
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from grand_plus_amd._common import layer_seed
from oracle.mlp_ref import _bn, _drop, _normalize

RELU, NORM, BN, TRAIN = 1, 2, 4, 8                       # GP_MLP_* of grandplus.h
ALL = frozenset(("x", "w", "b", "gamma", "beta"))
DROP_SEED = 0xDEADBEEF12345

Case = collections.namedtuple("Case", "name S B F N flags p bias affine rg special hashed loose seed eps momentum",
                              defaults=(None, None))      # BatchNorm's eps and momentum; None: torch's defaults
Built = collections.namedtuple("Built", "case x fc bn keep gy")
Ref = collections.namedtuple("Ref", "out a gx gw gb gg gbe rm rv nbt")


def flag_name(flags):
    return "".join(ch for ch, bit in zip("RNBT", (RELU, NORM, BN, TRAIN)) if flags & bit) or "0"


def case(lst, S, B, F, N, flags, p=None, bias=True, affine=True, rg=ALL, special=None, hashed=False, tag="", eps=None, momentum=None):
    """p defaults to 0.5 under TRAINING and 0 otherwise."""
    if p is None:
        p = 0.5 if flags & TRAIN else 0.0
    name = f"{lst}-{flag_name(flags)}-S{S}-B{B}-F{F}-N{N}" + (f"-{tag}" if tag else "")
    loose = B == 2 and (flags & (BN | TRAIN)) == (BN | TRAIN)
    return Case(name, S, B, F, N, flags, float(p), bias, affine, frozenset(rg), special, hashed, loose,
                zlib.crc32(name.encode()), eps, momentum)


# ---- the lists
FLAGS_SHAPE = (3, 37, 70, 19)        # one row tile with two sample boundaries, two column tiles of F, a 6-wide k tail, an N tail
FLAGS = [case("flags", *FLAGS_SHAPE, f) for f in range(16)]

FULL = RELU | NORM | BN | TRAIN
SAMPLES = [case("samples", S, 5, 33, 65, f) for f in (FULL, 0) for S in (1, 5, 15, 16)]


def _gemm_edges():
    T = TRAIN
    out = [case("gemm", 1, B, 17, 5, T, p=0) for B in (1, 63, 64, 65, 129)]                       # M of fwd and dA, K of dW
    out += [case("gemm", 1, 9, F, 33, T, p=0) for F in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65)]      # K of fwd, N of dA and dW
    out += [case("gemm", 1, 9, 17, N, T, p=0) for N in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)]  # N of fwd, K of dA, M of dW
    out += [case("gemm", 1, 9, F, 5, T, p=0, tag="split") for F in (65, 97, 129, 193, 2049)]      # 2, 2, 3, 4, 26 forward chunks
    out += [case("gemm", 1, 9, 5, N, T, p=0, tag="split_dA") for N in (65, 193)]
    out += [case("gemm", 1, M, 9, 5, T, p=0, tag="split_dW") for M in (65, 193)]
    out += [case("gemm", 5, 13, 9, 5, T, p=0, tag="split_dW")]                                    # the split across sample boundaries
    return list({c.name: c for c in out}.values())                                                # (9, 17, 33) is in two walks


GEMM_EDGES = _gemm_edges()

BN_EDGES = [case("bn", 2, B, F, 3, f, special="bn_cols") for f in (BN | TRAIN, FULL) for B in (2, 3, 15, 16, 17, 33)
            for F in (1, 15, 16, 17, 33)]

ROW_EDGES = [case("row", 3, 3, F, 4, f, special="rows") for f in (NORM | TRAIN, RELU | NORM | TRAIN) for F in (1, 63, 64, 65, 130)]
ZERO_ROW = case("row", 3, 3, 65, 4, NORM | TRAIN, special="zero_row")       # NORM without RELU over an all-zero row: its own test

OPTIONAL = [case("opt", *FLAGS_SHAPE, FULL, bias=False, tag="no_bias"),
            case("opt", *FLAGS_SHAPE, FULL, affine=False, tag="no_affine"),
            case("opt", *FLAGS_SHAPE, FULL, rg=("x",), tag="grad_x"),
            case("opt", *FLAGS_SHAPE, FULL, rg=("w", "b"), tag="grad_w_b"),
            case("opt", *FLAGS_SHAPE, FULL, rg=("x", "w"), tag="grad_x_w"),
            case("opt", *FLAGS_SHAPE, FULL, rg=("gamma", "beta"), tag="grad_gamma_beta")]

DROPOUT = [case("drop", *FLAGS_SHAPE, f, p=p, hashed=h, tag=f"p{p}" + ("_hash" if h else ""))
           for f in (BN | TRAIN, RELU | NORM | TRAIN) for p, h in ((0.0, False), (1.0, False), (1.0, True), (0.5, True))]

# the shapes that fill a workspace to its last float (tests/test_host_mlp_block.py proves that they do)
TIGHT = [case("tight", 2, 128, 2048, 128, FULL, tag="fwd"),          # 32 chunks of 64: 32 * 128 * 128 floats per sample
         case("tight", 2, 64, 128, 2048, FULL, tag="dA"),            # dA: S B = 128 rows, 32 chunks over N
         case("tight", 16, 128, 128, 128, FULL, tag="dW")]           # dW: 32 chunks over S B = 2048 rows; dA: 2 chunks of 2048 x 128
GUARD = TIGHT + [case("tight", *FLAGS_SHAPE, FULL, tag="flags_shape"),
                 case("tight", *FLAGS_SHAPE, BN, tag="eval_saved")]  # eval, no NORM: `saved` is unused but for slot 0 of the statistics

# BatchNorm's eps and momentum away from torch's defaults (1e-5, 0.1): forward, backward and the running statistics
BN_HYPER = [case("bnh", *FLAGS_SHAPE, f, eps=1e-3, momentum=0.3, tag="eps1e-3_mom0.3") for f in (BN | TRAIN, FULL)]

LISTS = {"FLAGS": FLAGS, "SAMPLES": SAMPLES, "GEMM_EDGES": GEMM_EDGES, "BN_EDGES": BN_EDGES, "ROW_EDGES": ROW_EDGES,
         "OPTIONAL": OPTIONAL, "DROPOUT": DROPOUT, "BN_HYPER": BN_HYPER}


def ids(cases):
    return [c.name for c in cases]


# ---- the hashed keep mask on the host: mlp.layer_seed and augment.hip's counter hash, entry b * F + f
def hashed_keep(seed, layer, S, B, F, p):
    out = np.zeros((S, B, F), np.uint8)
    e = np.arange(B * F, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for s in range(S):
            x = np.uint64(layer_seed(seed, layer, s)) + e * np.uint64(0x9E3779B97F4A7C15)
            x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            x ^= x >> np.uint64(31)
            u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
            out[s] = (u >= np.float32(p)).reshape(B, F)
    return torch.from_numpy(out)


# ---- the builder
def _special(c, x):
    S, B, F = x.shape
    relu = bool(c.flags & RELU)
    if c.special == "bn_cols" and F >= 2:
        x[:, :, F - 1] = 0.0                                 # zero everywhere: the common bag-of-words column
        # Constant within each sample: var = 0, invstd = eps^-1/2 = 316.  BN(v) = v * mul + add rounds v * mul, so the column
        # comes out as beta + O(316 * 2^-24 * |v|), in float32 torch as in mlp.hip; the constants are 2^-15 and 2^-14 to keep that
        # under a tenth of dW's bound (at 0.5 it is 2.3 bounds), and powers of two so that the mean is exact.  Under ReLU the
        # column is negative instead, a second zero column.
        for s in range(S):
            x[s, :, 0] = -0.5 * (s + 1) if relu else 2.0 ** (s - 15)
    if c.special == "bn_cols" and F == 1 and not relu:
        # One column: BatchNorm's backward leaves dn = c * (dy minus its parts along 1 and xhat / (1 + eps / var)), all of it
        # at B = 2 and by chance at B = 3, and no second column gives the rule a scale.  Rows 2^-8 apart have var ~ eps, so
        # about 0.4 of the part along xhat stays and dX is as well conditioned as in a wide layer.
        x *= 2.0 ** -8
    if c.special == "bn_cols" and F == 1 and relu:          # node_norm leaves 1 or 0: every sample gets both, or it would be the
        x[:, 0, 0] = x[:, 0, 0].abs() + 0.1                  # constant column at 1 (see above)
        x[:, 1, 0] = -x[:, 1, 0].abs() - 0.1
    if c.special == "bn_cols" and B == 3 and relu:
        # Three rows after ReLU: a column with one positive entry has xhat = (-1, 2, -1) / sqrt 2 whatever its value, dn is then
        # along (1, 0, -1), zero at the one row ReLU lets through, and dX gets rounding noise of c * |dy| with nothing left to
        # scale it by; a small positive entry makes c = gamma / sigma large on top.  Random signs give such columns by chance
        # (float32 torch then uses up to 0.37 of dX's bound).  So every other column holds two positive entries of at least 0.5
        # and one negative, the negative one in row k mod 3.
        for k in range(1 if F >= 2 else 0, F - 1 if F >= 2 else F):
            x[:, :, k] = x[:, :, k].abs() + 0.5
            x[:, k % 3, k] *= -1.0
    if c.special == "rows":
        r = x.view(S * B, F)
        if relu:
            r[0] = -r[0].abs() - 0.1                         # zero after ReLU: output = bias, dX row = 0
            r[1] = -r[1].abs() - 0.1
            r[1, F // 2] = 1.5                               # one positive entry
            r[2, 0] = -0.0
            if F >= 3:
                r[2, 1] = 0.0
            else:
                r[3, 0] = 0.0                                # F = 1: a row that is -0.0 and one that is 0.0
        elif F >= 3:                                         # no ReLU: exact zeros inside rows that stay non-zero
            r[2, 0] = -0.0
            r[2, 1] = 0.0
    if c.special == "zero_row":
        x.view(S * B, F)[4] = 0.0
    return x


def build(c):
    """A case's tensors and modules on the CPU: x [S, B, F], Linear(F, N), BatchNorm1d(F) or None with a non-trivial affine
    map and running statistics (as test_gpu_mlp._pair sets them), a uint8 keep mask [S, B, F] (the hash's own when
    c.hashed), gy [S, B, N]."""
    g = torch.Generator().manual_seed(c.seed)
    x = _special(c, torch.randn((c.S, c.B, c.F), generator=g))
    fc = nn.Linear(c.F, c.N, bias=c.bias)
    k = c.F ** -0.5
    fc.weight.data = (torch.rand((c.N, c.F), generator=g) * 2 - 1) * k
    if c.bias:
        fc.bias.data = (torch.rand((c.N,), generator=g) * 2 - 1) * k
    bn = None
    if c.flags & BN:
        bn = nn.BatchNorm1d(c.F, affine=c.affine, **{k: v for k, v in (("eps", c.eps), ("momentum", c.momentum)) if v is not None})
        if c.affine:
            bn.weight.data = torch.rand((c.F,), generator=g) + 0.5
            bn.bias.data = torch.randn((c.F,), generator=g) * 0.1
        bn.running_mean.data = torch.randn((c.F,), generator=g) * 0.1
        bn.running_var.data = torch.rand((c.F,), generator=g) + 0.5
    keep = (torch.rand((c.S, c.B, c.F), generator=g) >= c.p).to(torch.uint8)
    if c.hashed:
        keep = hashed_keep(DROP_SEED, 0, c.S, c.B, c.F, c.p)
    gy = torch.randn((c.S, c.B, c.N), generator=g)
    return Built(c, x, fc, bn, keep, gy)


def to(b, device):
    """The case on `device`, modules copied."""
    return Built(b.case, b.x.to(device), copy.deepcopy(b.fc).to(device), copy.deepcopy(b.bn).to(device) if b.bn is not None else None,
                 b.keep.to(device), b.gy.to(device))


# ---- the reference: plain torch ops and autograd
def block_ref(b, dtype=torch.float64):
    """The block in `dtype` on the device of b's tensors, BatchNorm per sample in sample order on a copy of the running
    statistics; every gradient from autograd.  b is left as it was."""
    c = b.case
    training = bool(c.flags & TRAIN)
    x = b.x.detach().to(dtype).requires_grad_(True)
    fc = copy.deepcopy(b.fc).to(dtype)
    bn = copy.deepcopy(b.bn).to(dtype) if b.bn is not None else None
    outs, acts = [], []
    for s in range(c.S):
        h = x[s]
        if c.flags & RELU:
            h = Fn.relu(h)
        if c.flags & NORM:
            h = _normalize(h)
        if bn is not None:
            h = _bn(bn, h, training)
        h = _drop(h, c.p, b.keep[s] if training else None)
        acts.append(h)
        outs.append(fc(h))
    out = torch.stack(outs)
    out.backward(b.gy.to(dtype))
    grad = lambda t: t.grad if t is not None else None  # noqa: E731
    return Ref(out.detach(), torch.stack(acts).detach(), x.grad, fc.weight.grad, grad(fc.bias),
               grad(bn.weight) if bn is not None else None, grad(bn.bias) if bn is not None else None,
               bn.running_mean if bn is not None else None, bn.running_var if bn is not None else None,
               (c.S if training else 0) if bn is not None else None)


def block_ref64(b):
    return block_ref(b, torch.float64)


# ---- mlp.hip's k_chunk: the chunk of a reduction of length K when one sample's output has `tiles` 64 x 64 tiles
def k_chunk(tiles, K):
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    want = 1 if tiles >= 128 else 128 // tiles
    want = max(1, min(want, cdiv(K, 64), 32))
    return cdiv(cdiv(K, 16), want) * 16


def splits(rows, cols, K):
    """Chunks of a GEMM with a rows x cols output (per sample in the forward) and a reduction of length K."""
    return -(-K // k_chunk(-(-rows // 64) * -(-cols // 64), K))


# ---- the same block with the backward written out, and one deliberate mistake
MUTANTS = ("relu_ge", "no_mean_dy", "unbiased_norm_var", "biased_running_var", "running_once", "sample0_stats", "no_norm_jacobian",
           "drop_scale_once", "last_chunk", "last_row", "bias_per_chunk",
           "eps_x2", "eps_default", "eps_outside_sqrt", "momentum_default")


def _gemm(A, Bm, rows, cols, mut):
    """A [M, K] @ Bm [K, N]; under "last_chunk" without the last chunk of a split reduction."""
    K = A.shape[1]
    if mut == "last_chunk":
        n = splits(rows, cols, K)
        if n > 1:
            K = (n - 1) * k_chunk(-(-rows // 64) * -(-cols // 64), K)
    return A[:, :K] @ Bm[:K]


def block_manual64(b, mut=None):
    """block_ref64's results from explicit formulas (mut None), or with one of MUTANTS built in."""
    c = b.case
    S, B, F, N = c.S, c.B, c.F, c.N
    relu, norm, training = bool(c.flags & RELU), bool(c.flags & NORM), bool(c.flags & TRAIN)
    x = b.x.double()
    W, gy = b.fc.weight.detach().double(), b.gy.double()
    bias = b.fc.bias.detach().double() if b.fc.bias is not None else None
    u = x.clamp(min=0) if relu else x
    L = u.norm(dim=-1, keepdim=True)
    r = 1.0 / (1e-12 + L) if norm else torch.ones_like(L)
    n = u * r
    rm = rv = nbt = gamma = None
    if b.bn is not None:
        eps = {"eps_x2": 2 * b.bn.eps, "eps_default": 1e-5}.get(mut, b.bn.eps)
        mom = 0.1 if mut == "momentum_default" else b.bn.momentum
        rm, rv = b.bn.running_mean.double().clone(), b.bn.running_var.double().clone()
        gamma = b.bn.weight.detach().double() if b.bn.weight is not None else torch.ones(F, dtype=torch.float64, device=x.device)
        beta = b.bn.bias.detach().double() if b.bn.bias is not None else torch.zeros(F, dtype=torch.float64, device=x.device)
        if training:
            rows = n[:, :-1] if mut == "last_row" else n
            mu = rows.sum(1, keepdim=True) / B
            var = ((n - mu) ** 2).sum(1, keepdim=True) / (B - 1 if mut == "unbiased_norm_var" else B)
            if mut == "sample0_stats":
                mu, var = mu[:1].expand(S, 1, F), var[:1].expand(S, 1, F)
            for s in range(1 if mut == "running_once" else S):
                rm = (1 - mom) * rm + mom * mu[s, 0]
                rv = (1 - mom) * rv + mom * var[s, 0] * (1.0 if mut == "biased_running_var" else B / (B - 1))
            nbt = S
        else:
            mu, var, nbt = rm.view(1, 1, F), rv.view(1, 1, F), 0
        istd = 1.0 / (torch.sqrt(var) + eps) if mut == "eps_outside_sqrt" else 1.0 / torch.sqrt(var + eps)
        xhat = (n - mu) * istd
        h = xhat * gamma + beta
    else:
        h = n
    drop = training and c.p > 0
    scale = (1.0 / (1.0 - c.p) if c.p < 1 else 0.0) if drop else 1.0
    d = b.keep.double() * scale if drop else torch.ones_like(x)
    a = h * d
    a2, gy2 = a.reshape(S * B, F), gy.reshape(S * B, N)
    out = _gemm(a2, W.t(), B, N, mut)
    if bias is not None:
        out = out + bias * (splits(B, N, F) if mut == "bias_per_chunk" else 1)
    gw = _gemm(gy2.t(), a2, N, F, mut)
    gb = gy2.sum(0) if bias is not None else None
    dy = _gemm(gy2, W, S * B, F, mut).reshape(S, B, F) * (d / scale if mut == "drop_scale_once" and drop and scale else d)
    gg = gbe = None
    if b.bn is not None:
        gg, gbe = (dy * xhat).sum((0, 1)), dy.sum((0, 1))
        if b.bn.weight is None:
            gg = gbe = None
        if training:
            mdy = 0.0 if mut == "no_mean_dy" else dy.mean(1, keepdim=True)
            dn = ((dy - mdy) - xhat * (dy * xhat).mean(1, keepdim=True)) * (gamma * istd)
        else:
            dn = dy * (gamma * istd)
    else:
        dn = dy
    if norm:
        second = torch.where(L > 0, u * (r * r / L.clamp(min=1e-300)) * (dn * u).sum(-1, keepdim=True), torch.zeros_like(u))
        du = r * dn - (0.0 if mut == "no_norm_jacobian" else second)
    else:
        du = dn
    gx = du * ((x >= 0) if mut == "relu_ge" else (x > 0)) if relu else du
    return Ref(out.reshape(S, B, N), a, gx, gw, gb, gg, gbe, rm, rv, nbt)


# ---- the bounds
def _scaled(ref, k):
    return k * (ref.abs() + ref.abs().max()) + 1e-9


def _norm_first_term(b):
    """max|r g| over the entries ReLU lets through: the gradient at u = relu?(x) with the row scales r held fixed, float64."""
    c = b.case
    training = bool(c.flags & TRAIN)
    x = b.x.double()
    u = (Fn.relu(x) if c.flags & RELU else x).detach().requires_grad_(True)
    r = (1.0 / (1e-12 + u.norm(dim=-1, keepdim=True))).detach()
    fc = copy.deepcopy(b.fc).double()
    bn = copy.deepcopy(b.bn).double() if b.bn is not None else None
    outs = []
    for s in range(c.S):
        h = u[s] * r[s]
        if bn is not None:
            h = _bn(bn, h, training)
        outs.append(fc(_drop(h, c.p, b.keep[s] if training else None)))
    torch.stack(outs).backward(b.gy.double())
    return (u.grad * (x > 0) if c.flags & RELU else u.grad).abs().max()


def bounds(b, ref):
    """{quantity: bound tensor} from the float64 reference, for every quantity the reference has."""
    c = b.case
    W = b.fc.weight.detach().double().abs()
    a = ref.a.abs().reshape(-1, c.F)
    gy = b.gy.double().abs().reshape(-1, c.N)
    bias = b.fc.bias.detach().double().abs() if b.fc.bias is not None else 0.0
    gx = _scaled(ref.gx, 1e-4 if c.loose else 1e-5)
    if c.F == 1 and c.flags & NORM:
        # node_norm of one column: du = r g - u r^2 / |u| <g, u> = g / |x| - g / |x|, zero in exact arithmetic, so max|ref| is no
        # scale.  The rule's "largest entry" is taken from the two terms that cancel, max|r g|; each is rounded a few times, so
        # float32 leaves about 2^-23 of it, the same distance from 1e-5 as everywhere else.
        gx = 1e-5 * (ref.gx.abs() + _norm_first_term(b)) + 1e-9
    out = {"out": (2e-5 * (a @ W.t() + bias) + 1e-6).reshape(c.S, c.B, c.N),
           "gx": gx,
           "gw": _scaled(ref.gw, 1e-4) if c.loose else 2e-5 * (gy.t() @ a) + 1e-6}
    if ref.gb is not None:
        out["gb"] = 2e-5 * gy.sum(0) + 1e-6
    for name in ("gg", "gbe"):
        if getattr(ref, name) is not None:
            out[name] = _scaled(getattr(ref, name), 1e-5)
    for name in ("rm", "rv"):
        if getattr(ref, name) is not None:
            out[name] = 1e-5 * getattr(ref, name).abs() + 1e-6
    return out


def wanted(c):
    """Which of gx, gw, gb, gg, gbe a call of the case must return: the rest must be None."""
    has = {"gx": "x", "gw": "w", "gb": "b" if c.bias else None,
           "gg": "gamma" if c.flags & BN and c.affine else None, "gbe": "beta" if c.flags & BN and c.affine else None}
    return {k for k, v in has.items() if v in c.rg}


def shares(b, got, ref, only=None):
    """{quantity: worst err / bound} of `got` (a Ref in any dtype; None fields are left out) against the reference."""
    out = {}
    for name, bound in bounds(b, ref).items():
        g = getattr(got, name)
        if g is None or (only is not None and name not in only):
            continue
        out[name] = float(((g.double() - getattr(ref, name)).abs() / bound).max())
    return out


def assert_case(b, got, ref, what=None):
    """Every quantity of `got` inside its bound and finite, the gradients that must not exist None, num_batches_tracked
    exact; prints the worst err / bound per quantity and returns them."""
    c = b.case
    need = wanted(c)
    for name in ("gx", "gw", "gb", "gg", "gbe"):
        assert (getattr(got, name) is not None) == (name in need), f"{c.name}: {name} {'missing' if name in need else 'must be None'}"
    sh = shares(b, got, ref)
    print(f"[mlp_block] {what or c.name}: " + ", ".join(f"{k} {v:.3g}" for k, v in sh.items()))
    for name, v in sh.items():
        assert bool(torch.isfinite(getattr(got, name)).all()), f"{c.name}: {name} is not finite"
        assert v <= 1.0, f"{c.name}: {name} is {v:.3g} bounds off"
    assert got.nbt == ref.nbt, f"{c.name}: num_batches_tracked {got.nbt}, expected {ref.nbt}"
    return sh


# ---- the rule of the whole model (tests/test_gpu_mlp.py, tests/test_gpu_reference_training.py)
def model_assert_out(got, ref_out, last_a, fc):
    """The logits of a whole model: |d| <= 2e-5 * (|a| |W|^T + |b|) + 1e-6 with a the last Linear's input, and finite."""
    scale = last_a.detach().abs() @ fc.weight.detach().abs().t() + fc.bias.detach().abs()
    err = (got.double() - ref_out.detach()).abs()
    bad = err > 2e-5 * scale + 1e-6
    assert not bool(bad.any()), f"{int(bad.sum())} outputs off, max err {float(err.max()):.3g}"
    assert bool(torch.isfinite(got).all())


def model_assert_grad(got, ref, name):
    """A gradient of a whole model: rtol 1e-4, atol 1e-4 max|ref| + 1e-9."""
    assert got is not None, name
    scale = float(ref.abs().max())
    torch.testing.assert_close(got.double(), ref, rtol=1e-4, atol=1e-4 * scale + 1e-9, msg=name)
