"""Shapes, inputs and the reference maths of the optimiser tests, shared by test_gpu_optim.py and
test_host_optim.py.

The reference is torch's own `clip_grad_norm_` + `torch.optim.Adam(foreach=False)` on the CPU, in float64 (and in float32
for the error bound), fed a pre-generated gradient sequence -- the same one for every implementation, so nothing chaotic
enters.  With max_norm <= 0 the reference skips `clip_grad_norm_`, as model.py:119-120 does (a negative max_norm passed to
torch would flip the gradients' sign); the norm it reports is then formed directly.
"""
import functools

import torch

CHUNK = 4096          # kChunk of csrc/optim.hip: elements of one tensor per unit of work
MAX_TENSORS = 32      # GP_OPTIM_MAX_TENSORS
GRID_CAP = 1024       # kMaxGrid = kSlots = GP_OPTIM_WORKSPACE_BYTES / 8: workgroups of one launch
STEPS = 5
BETAS, EPS = (0.9, 0.999), 1e-8

# the smallest sets that take each path
SETS = {
    "cora": [(64, 1433), (64,), (7, 64), (7,)],
    "odd": [(1,), (3, 5), (0,), (CHUNK + 1,), (2 * CHUNK - 1,)],      # one element, empty, chunk boundary +1 and -1
    "views": [(5,), (3, 7), (CHUNK + 3,), (66,)],                    # views of one flat buffer, none 16-byte aligned
    "many": [(n,) for n in range(1, 41)],                             # over the table capacity: two groups
    "holes": [(64, 1433), (64,), (7, 64), (7,)],                      # cora with .grad = None on two of them
    # past the grid cap of GRID_CAP workgroups (tests/test_gpu_second_trip.py): 1 028 chunks, so workgroups 0 .. 3 take a
    # second chunk each -- two whole chunks of the second tensor, its 5-element tail and the whole third tensor
    "stride": [(5,), ((GRID_CAP + 1) * CHUNK + 5,), (7,)],
    # two table groups, the second with more chunks (42) than the first (32): the first norm launch owns slots it has no
    # chunk for, and the second launch adds into them
    "late_big": [(1,)] * MAX_TENSORS + [(40 * CHUNK + 3,), (3,)],
    "solo": [(1,)],                                                   # one element: one workgroup, every other slot zeroed
}
# Sets that tests/test_gpu_second_trip.py runs, outside the 5-step grid of test_gpu_optim.py.  "stride" is too large for
# 15 cases of 5 steps and takes STRIDE_STEPS.  "solo" is stepped once, after "stride", for its norm: the grid's rule
# measures ours by the maximum of torch's float32 error over all elements, which one element does not give (on its five
# gradients exp_avg = 4.7e-3 is what is left of terms of 1e-2; the kernel's documented arithmetic, walked in numpy
# float32, is 2.59e-9 off float64, torch's lerp form 2.1e-10 by luck, the bound from it 1.4e-9).
OWN_TESTS = ("stride", "solo")
STRIDE_STEPS = 2
VIEW_OFFSETS = (1, 2, 3, 5)       # element offset of each view past a 64-element boundary of the flat buffer
HOLES = (1, 2)                    # indices of "holes" without a gradient

# lr, weight_decay, clip_norm, scale of the gradients
HYPERS = [
    dict(lr=1e-2, weight_decay=5e-4, clip=0.1, gscale=1.0),          # clipping active: the run scripts' values
    dict(lr=1e-2, weight_decay=0.0, clip=0.0, gscale=1.0),           # no clipping
    dict(lr=1e-3, weight_decay=1e-5, clip=5.0, gscale=1e-3),         # the coefficient clamps to 1
    # total norms of 1e-8 sqrt(n), 1.1e-6 on "odd": coef = clip / (norm + 1e-6) is about half of clip / norm, so the 1e-6
    # of the coefficient decides the step (tests/test_host_mutants.py: without it "cora" moves by 3.5e4 bounds)
    dict(lr=1e-2, weight_decay=5e-4, clip=2e-6, gscale=1e-8),
]
TINY = 3                          # the entry above: gradients at the scale of clip_grad_norm's 1e-6
# betas and eps away from torch's defaults, on the host-number and on the capturable path: (set, hyper, betas, eps)
OFF_DEFAULT = [("cora", 0, (0.8, 0.99), 1e-6), ("odd", 0, (0.8, 0.99), 1e-6)]

# what tests/test_gpu_optim.py draws: the 5-step grid at the default betas and eps, then OFF_DEFAULT on both paths
GRID = [(name, hi) for name in SETS if name not in OWN_TESTS for hi in range(len(HYPERS))]
DRAWN = [(name, hi, BETAS, EPS) for name, hi in GRID] + OFF_DEFAULT

assert len(SETS["many"]) > MAX_TENSORS and (CHUNK + 1,) in SETS["odd"]
SEED_ORDER = ("cora", "holes", "many", "odd", "views", "stride", "late_big", "solo")   # a set's place seeds its inputs: append only
assert sorted(SEED_ORDER) == sorted(SETS)


def numel(shape):
    n = 1
    for d in shape:
        n *= d
    return n


@functools.lru_cache(maxsize=None)
def inputs(name, hi, steps=STEPS):
    """(initial parameters, gradient sequence) of a case as float32 CPU tensors; a gradient of "holes" may be None."""
    g = torch.Generator().manual_seed(1000 * hi + SEED_ORDER.index(name))
    init = [torch.randn(s, generator=g) * 0.1 for s in SETS[name]]
    scale = HYPERS[hi]["gscale"]
    seq = []
    for _ in range(steps):
        grads = [torch.randn(s, generator=g) * scale for s in SETS[name]]
        if name == "holes":
            for i in HOLES:
                grads[i] = None
        seq.append(grads)
    return init, seq


def total_norm(grads):
    """sqrt(sum of squares) in the gradients' own dtype, as torch forms it: the norm of the per-tensor norms."""
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))


def torch_run(init, seq, hyper, dtype, betas=BETAS, eps=EPS):
    """torch's clip_grad_norm_ + Adam(foreach=False) on the CPU in `dtype`, over the gradient sequence `seq`.
    Returns {"param", "exp_avg", "exp_avg_sq"}: lists over the tensors (None where a tensor got no state), and "norm":
    the total norm of every step before clipping."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in init]
    opt = torch.optim.Adam(params, lr=hyper["lr"], betas=betas, eps=eps, weight_decay=hyper["weight_decay"], foreach=False)
    norms = []
    for grads in seq:
        for p, g in zip(params, grads):
            p.grad = None if g is None else g.to(dtype).clone()
        with_grad = [p for p in params if p.grad is not None]
        if hyper["clip"] > 0:
            norms.append(torch.nn.utils.clip_grad_norm_(with_grad, hyper["clip"], foreach=False).detach().clone())
        else:
            norms.append(total_norm([p.grad for p in with_grad]))
        opt.step()
    state = [opt.state.get(p, {}) for p in params]
    return {"param": [p.detach() for p in params], "exp_avg": [s.get("exp_avg") for s in state],
            "exp_avg_sq": [s.get("exp_avg_sq") for s in state], "norm": norms}


@functools.lru_cache(maxsize=None)
def reference(name, hi, steps=STEPS, betas=BETAS, eps=EPS):
    """(float64 run, float32 run) of torch on the CPU over the `steps` gradients of the case; computed once."""
    init, seq = inputs(name, hi, steps)
    return torch_run(init, seq, HYPERS[hi], torch.float64, betas, eps), torch_run(init, seq, HYPERS[hi], torch.float32, betas, eps)


# ---- the same run written out, and one deliberate mistake (tests/test_host_mutants.py)
MUTANTS = ("eps_x10", "eps_0", "eps_before_bias_correction", "eps_in_sqrt", "clip_no_1e6", "clip_no_clamp", "wd_before_clip",
           "wd_decoupled", "bc_step_minus_1", "betas_default", "eps_default", "lr_without_bc1")


def manual_run(init, seq, hyper, betas=BETAS, eps=EPS, mut=None, dtype=torch.float64):
    """torch_run's results from explicit formulas (mut None), or with one of MUTANTS built in.  In float32 it is the kernel's
    documented arithmetic: the float64 norm rounded once, coef, then per element g = grad coef + wd p,
    m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g, p -= step_size (m / (sqrt(v) rsqrt_bc2 + eps)), the two step numbers
    formed in double."""
    lr, wd, clip = hyper["lr"], hyper["weight_decay"], hyper["clip"]
    if mut == "betas_default":
        betas = BETAS
    if mut == "eps_default":
        eps = EPS
    eps = {"eps_x10": 10 * eps, "eps_0": 0.0}.get(mut, eps)
    b1, b2 = betas
    P = [p.to(dtype).clone() for p in init]
    M, V = [None] * len(P), [None] * len(P)
    cast = lambda v: torch.tensor(v, dtype=dtype)  # noqa: E731
    for t, grads in enumerate(seq, 1):
        G = [None if g is None else g.to(dtype) for g in grads]
        if mut == "wd_before_clip":
            G = [None if g is None else g + cast(wd) * p for g, p in zip(G, P)]
        if clip > 0:
            sq = sum(float((g.double() ** 2).sum()) for g in G if g is not None)
            norm = cast(sq ** 0.5)
            coef = cast(clip) / (norm if mut == "clip_no_1e6" else norm + cast(1e-6))
            if mut != "clip_no_clamp":
                coef = coef.clamp(max=1.0)
        else:
            coef = cast(1.0)
        tb = t - 1 if mut == "bc_step_minus_1" else t
        bc1, bc2 = 1.0 - b1 ** tb, 1.0 - b2 ** tb
        with torch.no_grad():
            for i, g in enumerate(G):
                if g is None:
                    continue
                if M[i] is None:
                    M[i], V[i] = torch.zeros_like(P[i]), torch.zeros_like(P[i])
                g = g * coef
                if mut == "wd_decoupled":
                    P[i] = P[i] * cast(1.0 - lr * wd)
                elif mut != "wd_before_clip":
                    g = g + cast(wd) * P[i]
                M[i] = cast(b1) * M[i] + cast(1.0 - b1) * g
                V[i] = cast(b2) * V[i] + cast(1.0 - b2) * g * g
                if bc1 == 0.0 or bc2 == 0.0:                          # bc_step_minus_1 at the first step: lr / 0
                    P[i] = P[i] * float("nan")
                    continue
                step_size = lr if mut == "lr_without_bc1" else lr / bc1
                if mut == "eps_before_bias_correction":
                    denom = (V[i].sqrt() + cast(eps)) * cast(bc2 ** -0.5)
                elif mut == "eps_in_sqrt":
                    denom = (V[i] * cast(1.0 / bc2) + cast(eps)).sqrt()
                else:
                    denom = V[i].sqrt() * cast(bc2 ** -0.5) + cast(eps)
                P[i] = P[i] - cast(step_size) * (M[i] / denom)
    return {"param": P, "exp_avg": M, "exp_avg_sq": V}


def rule(ours, t32, r64):
    """{key: (max|ours - ref64|, max|torch32 - ref64|, the bound)} of error_ratios' rule; nothing asserted but that state is
    present on both sides or on neither.  A non-finite entry of `ours` counts as an infinite error."""
    out = {}
    for key in ("param", "exp_avg", "exp_avg_sq"):
        e_ours = e_t32 = top = 0.0
        for o, t, r in zip(ours[key], t32[key], r64[key]):
            assert (o is None) == (r is None), f"{key}: state present on one side only"
            if r is None or r.numel() == 0:
                continue
            e = float((o.detach().cpu().double() - r).abs().max())
            e_ours = max(e_ours, e if e == e else float("inf"))
            e_t32 = max(e_t32, float((t.double() - r).abs().max()))
            top = max(top, float(r.abs().max()))
        out[key] = (e_ours, e_t32, 4 * e_t32 + 2.0 ** -23 * top)
    return out


def error_ratios(ours, t32, r64, label=""):
    """The bound of the issue, separately for param, exp_avg and exp_avg_sq, the maxima over all elements of all tensors:

        max|ours - ref64| <= 4 max|torch32 - ref64| + 2^-23 max|ref64|

    4 covers another association of the same ten or so fp32 operations; the floor is one ulp of the largest value, for
    the case where torch happens to be exact.  `ours` maps the three keys to lists of tensors (any device; None where
    there is no state).  Prints each figure, then asserts; returns {key: ours / torch32}."""
    out = {}
    for key, (e_ours, e_t32, bound) in rule(ours, t32, r64).items():
        out[key] = e_ours / e_t32 if e_t32 > 0 else float("inf") if e_ours > 0 else 0.0
        print(f"{label} {key}: ours {e_ours:.3e} torch32 {e_t32:.3e} ratio {out[key]:.3g} bound {bound:.3e}")
        assert e_ours <= bound, f"{label} {key}: max error {e_ours:.3e} over the bound {bound:.3e} (torch32 {e_t32:.3e})"
    return out


def device_params(name, init, device="cuda"):
    """The case's parameters on the device, holding `init`.  "views": four views of one flat buffer, each starting
    VIEW_OFFSETS[i] elements past a 64-element boundary (so no pointer is 16-byte aligned)."""
    if name != "views":
        return [torch.nn.Parameter(p.to(device)) for p in init]
    starts, cursor = [], 0
    for p, off in zip(init, VIEW_OFFSETS):
        cursor = (cursor + 63) // 64 * 64 + off
        starts.append(cursor)
        cursor += p.numel()
    flat = torch.zeros(cursor, device=device)
    params = []
    for p, s in zip(init, starts):
        view = flat[s:s + p.numel()].view(p.shape)
        view.copy_(p)
        params.append(torch.nn.Parameter(view))
        assert params[-1].data_ptr() % 16 != 0 and params[-1].is_contiguous()
    return params


def set_grads(params, grads):
    """Gives every parameter its gradient (None = no gradient).  A parameter that is a view at an odd offset ("views")
    gets a gradient that is one too, as a caller with flattened gradients has them: a view of a fresh buffer at the same
    offset modulo 4 elements, so the gradient pointer is not 16-byte aligned either."""
    for p, g in zip(params, grads):
        if g is None:
            p.grad = None
        elif p.data_ptr() % 16 == 0:
            p.grad = g.to(p.device).clone()
        else:
            k = p.storage_offset() % 4
            view = torch.empty(k + g.numel(), dtype=g.dtype, device=p.device)[k:].view(g.shape)
            view.copy_(g)
            assert view.data_ptr() % 16 != 0 and view.is_contiguous()
            p.grad = view
