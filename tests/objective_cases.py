"""Cases, the reference with upstream gradients and the tolerance of the fused-objective edge tests, shared
by test_gpu_objective.py and test_host_objective.py.  The reference maths itself is oracle/objective_ref.py.

Every case is a `Case`; `build(case)` gives its inputs and `reference(case, coeffs)` the float64 (or float32) result,
each computed once.  `build` guarantees a margin: the tests assert `n_conf` equal to a float64 count, so no unlabelled
row's float64 `avg_p.max(1)` may lie within relative MARGIN of `conf` (rows that do are redrawn), unless `conf` is
outside (0, 1), where every row (conf <= 0) or none (conf >= 1) is confident whatever the rounding.
"""
import collections
import functools
import math

import torch
import torch.nn.functional as Fn

from oracle.objective_ref import consis_loss_ref, grand_loss_ref

MARGIN = 1e-4
MAX_S, MAX_C = 16, 4096                  # kMaxS, kMaxC of csrc/objective.hip
GRID_ROWS = 65535 * 4                    # rows of one trip of the grid-stride loop: row_grid's cap times kWaves
IGNORE = -100

# special: "" (random logits), "ignore" (one ignore_index label), "ties", "neginf" and "underflow" (see build)
Case = collections.namedtuple("Case", "S B C n_l kind tem w conf scale seed log_probs special",
                              defaults=(0.5, 0.7, None, 3.0, 0, False, ""))

COEFFS = ((2.5, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0.5, -1.5), (-1, 2, 0.25))      # (a, b, c) of a*loss + b*L_sup + c*L_con
KINDS = ("kl", "l2")


def _seed(*xs):
    h = 17
    for x in xs:
        h = (h * 1000003 + int(x)) % (2 ** 31 - 1)
    return h


def upstream_case(kind, w):
    return Case(3, 90, 7, 30, kind, w=w, seed=_seed(1, kind == "kl"))


def logprob_case(S, C, kind):
    return Case(S, 70, C, 20, kind, seed=_seed(2, S, C, kind == "kl"), log_probs=True, special="ignore")


def sample_case(S, C, n_l, kind):
    return Case(S, 70 + n_l, C, n_l, kind, tem=(0.1, 0.5, 1.0)[(S + C + n_l) % 3], seed=_seed(3, S, C, n_l, kind == "kl"))


def class_case(C, S, kind):
    """C = 1: every probability is 1, conf = 0.5 makes every row confident.  C = 2: 2 / C = 1 would leave no row
    confident, so 0.7.  C >= 1000: logits of scale 6, whose largest probability is far above 2 / C."""
    conf = {1: 0.5, 2: 0.7}.get(C)
    return Case(S, 24, C, 8, kind, conf=conf, scale=6.0 if C >= 1000 else 3.0, seed=_seed(4, C, S, kind == "kl"))


def row_case(B, n_l, kind):
    return Case(2, B, 7, n_l, kind, seed=_seed(5, B, n_l, kind == "kl"))


ALL_LABELLED = Case(2, 40, 7, 40, "l2", seed=_seed(6))
SECOND_TRIP = Case(2, GRID_ROWS + 37, 3, 1000, "kl", tem=0.5, seed=_seed(7))
STRIDED = Case(3, 50, 7, 10, "kl", seed=_seed(8))
NEGINF = Case(2, 26, 130, 6, "l2", scale=1.0, seed=_seed(9), special="neginf")
TIES = Case(2, 26, 130, 6, "l2", scale=1.0, seed=_seed(10), special="ties")


def sharpen_case(kind):
    """avg_p ~ 1 / 4096 = 2^-12 and 1 / tem = 20: avg_p ** 20 ~ 2^-240 is 0 in fp32, so the naive sharp_p is 0 / 0."""
    return Case(2, 16, 4096, 0, kind, tem=0.05, w=1.0, conf=0.0, scale=0.01, seed=_seed(11, kind == "kl"))


UPSTREAM = [upstream_case(k, w) for k in KINDS for w in (0.7, 0.0, -0.6)]
LOGPROB = [logprob_case(S, C, k) for S in (1, 3) for C in (7, 65) for k in KINDS]
SAMPLES = [sample_case(S, C, n_l, k) for S in (5, 8, 15, 16) for C in (7, 65) for n_l in (0, 20) for k in KINDS]
CLASSES = [class_case(C, S, k) for C in (1, 2, 63, 64, 65, 128, 129, 1000, 4096) for S in (1, 3) for k in KINDS]
ROWS = [row_case(B, n_l, k) for B in (1, 2, 3, 5) for n_l in sorted({0, 1, B}) for k in KINDS] + [ALL_LABELLED]
# a probability that is 0 in fp32 itself (logit 120 below the rest, e^-120 ~ 1e-52) under a flattening tem = 20: its
# share of q is ~ e^-6 / C, which log(avg_p) formed from fp32 probabilities would lose
UNDERFLOW = Case(2, 16, 7, 0, "kl", tem=20.0, w=1.0, conf=0.0, seed=_seed(12), special="underflow")
SHARPEN = [sharpen_case(k) for k in KINDS] + [UNDERFLOW]

# tied columns of the last sample per labelled row: same lane and another 64-column stride; adjacent lanes; lanes 0 and
# 63; the third stride (columns 128, 129 = lanes 0, 1) against column 0; a lower column in a higher lane (1 before 128);
# lane 63 against lane 0 of the next stride
TIE_COLUMNS = ((5, 69), (17, 18), (0, 63), (0, 128, 129), (1, 128, 129), (63, 64))


PLAIN = ((1, 0, 0),)
# every case the GPU tests draw, with the (a, b, c) combinations each is run under
DRAWN = ([(c, COEFFS) for c in UPSTREAM] + [(c, (PLAIN[0], COEFFS[3])) for c in LOGPROB] +
         [(c, PLAIN) for c in SAMPLES + CLASSES + ROWS + SHARPEN + [SECOND_TRIP, STRIDED, NEGINF, TIES]])


def case_id(case):
    return "S{}-B{}-C{}-nl{}-{}{}{}".format(case.S, case.B, case.C, case.n_l, case.kind, "-w%g" % case.w if case.w != 0.7 else "",
                                           "-logp" if case.log_probs else "") + ("-" + case.special if case.special else "")


def avg_p_max(z, n_l, log_probs):
    """float64 avg_p.max(1) of the unlabelled rows, as consis_loss forms it."""
    z = z.double()
    p = torch.exp(z if log_probs else torch.log_softmax(z, -1))
    return p.mean(0)[n_l:].max(1)[0] if z.shape[1] > n_l else z.new_zeros(0)


def margin_ok(z, n_l, conf, log_probs=False):
    """The margin condition: conf outside (0, 1), or no unlabelled row within relative MARGIN of conf."""
    if not 0.0 < conf < 1.0:
        return True
    return not bool(((avg_p_max(z, n_l, log_probs) - conf).abs() <= MARGIN * conf).any())


def make_case(S, B, C, seed, scale=3.0, n_l=0, conf=None, log_probs=False):
    """(z float32 [S, B, C], labels int64 [max(n_l, 1)], n_l, conf) under the margin condition.  conf=None is 2 / C
    (the value is returned).  Even labelled rows carry the last sample's argmax as their label, the others a random one.  With log_probs, z holds the float32 log_softmax of the drawn logits."""
    g = torch.Generator().manual_seed(seed)
    raw = torch.randn((S, B, C), generator=g) * scale
    labels = torch.randint(0, C, (max(n_l, 1),), generator=g)
    labels[:n_l:2] = raw[S - 1, :n_l:2].argmax(1)                # every other labelled row is predicted correctly
    conf = 2.0 / C if conf is None else float(conf)

    def as_input(x):
        return torch.log_softmax(x.double(), -1).float() if log_probs else x

    z = as_input(raw)
    for _ in range(100):
        if margin_ok(z, n_l, conf, log_probs):
            return z, labels, n_l, conf
        near = torch.nonzero((avg_p_max(z, n_l, log_probs) - conf).abs() <= MARGIN * conf)[:, 0] + n_l
        raw[:, near] = torch.randn((S, near.numel(), C), generator=g) * scale
        z = as_input(raw)
    raise AssertionError("no draw met the margin condition")


@functools.lru_cache(maxsize=None)
def build(case):
    """The inputs of a case: (z, labels, n_l, conf), computed once; callers must not modify them."""
    z, labels, n_l, conf = make_case(case.S, case.B, case.C, case.seed, case.scale, case.n_l, case.conf, case.log_probs)
    if case.special == "ignore":
        labels[3] = IGNORE
    elif case.special == "ties":
        for r, cols in enumerate(TIE_COLUMNS):
            z[case.S - 1, r, list(cols)] = 10.0                  # far above every drawn logit (scale 1)
            labels[r] = cols[0] if r % 2 == 0 else cols[-1]      # the first tied index is the correct answer on even rows only
    elif case.special == "underflow":
        z[:, :, 0] -= 120.0
    elif case.special == "neginf":
        z[:, 2, :] = -math.inf                                    # row 2: only the label and one more class are finite
        other = (int(labels[2]) + 67) % case.C
        for s in range(case.S):
            z[s, 2, int(labels[2])] = 0.5 - s
            z[s, 2, other] = 1.0 + s
    assert margin_ok(z, n_l, conf, case.log_probs)
    return z, labels, n_l, conf


def reference_terms(z, labels, n_l, w, tem, conf, kind, log_probs=False, ignore_index=IGNORE):
    """(loss, L_sup, L_con) in z's dtype, differentiable in z.  With log_probs, z holds log-probabilities: nll_loss and
    consis_loss_ref take them directly, with no log_softmax."""
    if not log_probs:
        return grand_loss_ref(z, labels, n_l, w, tem, conf, kind, ignore_index=ignore_index)
    S = len(z)
    sup = 0.
    for s in range(S):
        sup = sup + Fn.nll_loss(z[s][:n_l], labels[:n_l], ignore_index=ignore_index)
    sup = sup / S
    con = consis_loss_ref([z[s][n_l:] for s in range(S)], tem, conf, kind)
    return sup + w * con, sup, con


# ---- the same terms written out, and one deliberate mistake (tests/test_host_mutants.py)
MUTANTS = ("conf_ge", "mean_over_all_rows", "sharp_not_detached", "kl_reversed", "tem_not_inverted", "weight_on_sup",
           "sup_last_sample_only", "sup_summed_over_samples")
# `avg_p.max(1) >= conf` differs from `> conf` on a row whose float64 avg_p.max(1) equals conf, and on no other.  The
# reference's own exp(log_softmax) is not exact there, so which side a tie falls on is not defined by it, and make_case keeps
# every row away from conf by MARGIN for that reason: no case can see this mistake, and none should.
INDISTINGUISHABLE = ("conf_ge",)


def manual_terms(z, labels, n_l, w, tem, conf, kind, log_probs=False, ignore_index=IGNORE, mut=None):
    """reference_terms from explicit formulas (mut None), or with one of MUTANTS built in."""
    S = len(z)
    lps = [z[s] if log_probs else torch.log_softmax(z[s], dim=-1) for s in range(S)]
    sup = 0.
    for s in (range(S - 1, S) if mut == "sup_last_sample_only" else range(S)):
        sup = sup + Fn.nll_loss(lps[s][:n_l], labels[:n_l], ignore_index=ignore_index)
    if mut not in ("sup_last_sample_only", "sup_summed_over_samples"):
        sup = sup / S
    ps = [torch.exp(lp[n_l:]) for lp in lps]
    avg_p = sum(ps[1:], ps[0]) / S
    powered = torch.pow(avg_p, tem if mut == "tem_not_inverted" else 1. / tem)
    sharp_p = powered / powered.sum(dim=1, keepdim=True)
    if mut != "sharp_not_detached":
        sharp_p = sharp_p.detach()
    top = avg_p.max(1)[0]
    mask = top >= conf if mut == "conf_ge" else top > conf
    con = 0.
    for p in ps:
        if kind == "kl":
            row = (-p * torch.log(sharp_p)).sum(1) if mut == "kl_reversed" else (-sharp_p * torch.log(p)).sum(1)
        else:
            row = (p - sharp_p).pow(2).sum(1)
        con = con + (row[mask].sum() / row.numel() if mut == "mean_over_all_rows" else torch.mean(row[mask]))
    con = con / S
    return (w * sup + con if mut == "weight_on_sup" else sup + w * con), sup, con


def manual_with_upstream(z, labels, n_l, w, tem, conf, kind, coeffs=(1, 0, 0), log_probs=False, mut=None):
    """reference_with_upstream in float64 over manual_terms."""
    leaf = z.detach().double().clone().requires_grad_(True)
    terms = manual_terms(leaf, labels, n_l, w, tem, conf, kind, log_probs, mut=mut)
    total = combine(terms, coeffs)
    if total is not None and total.requires_grad:
        total.backward()
    grad = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    loss, sup, con = (float(t.detach()) for t in terms)
    return {"loss": loss, "sup": sup, "con": con, "grad": grad.detach()}


def manual(case, coeffs=(1, 0, 0), mut=None):
    z, labels, n_l, conf = build(case)
    return manual_with_upstream(z, labels, n_l, case.w, case.tem, conf, case.kind, coeffs, case.log_probs, mut)


def share(got, ref):
    """The largest |got - ref| / bound over the loss, its parts and the gradient, under assert_matches' rule."""
    out = grad_error(got["grad"], ref["grad"])[1]
    for k in ("loss", "sup", "con"):
        e, b = value_error(got[k], ref[k])
        out = max(out, e / b if b else (math.inf if e else 0.0))
    return out


def combine(terms, coeffs):
    """a*loss + b*L_sup + c*L_con without the terms whose coefficient is 0 (so that autograd passes None for them);
    None when every coefficient is 0."""
    total = None
    for k, t in zip(coeffs, terms):
        if k != 0:
            total = k * t if total is None else total + k * t
    return total


def reference_with_upstream(z, labels, n_l, w, tem, conf, kind, coeffs=(1, 0, 0), log_probs=False, dtype=torch.float64):
    """The reference under upstream gradients: {"loss", "sup", "con"} as floats and "grad" = d(a*loss + b*L_sup +
    c*L_con)/dz, in `dtype` on the host (zeros where nothing depends on z)."""
    leaf = z.detach().to(dtype).clone().requires_grad_(True)
    terms = reference_terms(leaf, labels, n_l, w, tem, conf, kind, log_probs)
    total = combine(terms, coeffs)
    if total is not None and total.requires_grad:
        total.backward()
    grad = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
    loss, sup, con = (float(t.detach()) for t in terms)
    return {"loss": loss, "sup": sup, "con": con, "grad": grad.detach()}


@functools.lru_cache(maxsize=None)
def reference(case, coeffs=(1, 0, 0), dtype=torch.float64, rows=None):
    """reference_with_upstream of a case, computed once; `rows` keeps only the first rows of the batch (the host check
    of the largest case)."""
    z, labels, n_l, conf = build(case)
    if rows is not None:
        z = z[:, :rows]
    return reference_with_upstream(z, labels, n_l, case.w, case.tem, conf, case.kind, coeffs, case.log_probs, dtype)


def counts(case):
    """{"n_conf", "n_valid", "n_correct", "n_bad_labels"} from float64 and torch.argmax (the first index of the maximum)."""
    z, labels, n_l, conf = build(case)
    y = labels[:n_l]
    valid = (y >= 0) & (y < case.C)
    pred = z[case.S - 1, :n_l].argmax(1) if n_l else y
    return {"n_conf": int((avg_p_max(z, n_l, case.log_probs) > conf).sum()), "n_valid": int(valid.sum()),
            "n_correct": int(((pred == y) & valid).sum()), "n_bad_labels": int((~valid & (y != IGNORE)).sum())}


def value_error(got, want):
    """(|got - want|, the bound 1e-5 |want| + 1e-7) of the loss or a part; NaN matches NaN alone (error 0 or inf)."""
    got, want = float(got), float(want)
    if math.isnan(want) or math.isnan(got):
        return (0.0 if math.isnan(want) and math.isnan(got) else math.inf), 0.0
    return abs(got - want), 1e-5 * abs(want) + 1e-7


def grad_error(dz, gref):
    """(the largest |dz - gref|, the largest ratio of |dz - gref| to its bound 1e-5 max|gref row| + 1e-7); a NaN
    on either side gives inf."""
    dz, gref = dz.detach().double().cpu(), gref.double()
    if dz.numel() == 0:
        return 0.0, 0.0
    tol = 1e-5 * gref.abs().amax(dim=-1, keepdim=True) + 1e-7
    d = torch.nan_to_num((dz - gref).abs(), nan=math.inf)
    return float(d.max()), float((d / tol).max())


def assert_matches(got, dz, ref, label=""):
    """The file's rule, stated once: loss and parts within 1e-5 |ref| + 1e-7 (NaN matching NaN), dz per element within
    1e-5 max|ref row| + 1e-7.  `got` maps "loss", "sup", "con" to scalars.  Prints each figure, then asserts."""
    figures = {k: value_error(got[k], ref[k]) for k in ("loss", "sup", "con")}
    g_err, g_ratio = grad_error(dz, ref["grad"])
    print(f"[objective] {label}: " + "  ".join(f"{k} |d| {e:.3e} / {b:.3e}" for k, (e, b) in figures.items()) +
          f"  dz max |d| {g_err:.3e}, {g_ratio:.3g} of its bound")
    for k, (e, b) in figures.items():
        assert e <= b, f"{label} {k}: {float(got[k])!r} against {ref[k]!r}"
    assert g_ratio <= 1.0, f"{label} dz: max |d| {g_err:.3e} is {g_ratio:.3g} of the bound"
