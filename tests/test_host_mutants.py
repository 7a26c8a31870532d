"""The audit of the bounds themselves, with no GPU: would a GPU test fail if its kernel were subtly wrong?

Each case module keeps, beside its float64 reference, the same maths written out with the name of one deliberate mistake
(`mut`).  Per module two tests: every mistake, built into the float64 formulas, moves some case that the module's GPU file
draws by more than SEEN bounds under the module's own rule (so the GPU test can fail); and every case added for this audit
leaves a correct float32 kernel room, its float32 restatement using less than ROOM of the bound (so it can pass).  SEEN and
ROOM are tests/test_host_mlp_block.py's figures.  The printed figures are in DESIGN §7q."""
import copy
import math
import functools

import numpy as np
import pytest
import torch

import augment_cases as ac
import evaluate_cases as ec
import infer_cases as ic
import mag_cases as gc
import objective_cases as jc
import optim_cases as oc
import propagate_cases as pc
from test_host_mlp_block import ROOM, SEEN


def _report(module, mut, best):
    """best = (share, case): an infinite share is a quantity the GPU file holds exactly, or a value that is not finite."""
    moved = "differs in a quantity held exactly, or is not finite" if math.isinf(best[0]) else f"moves by {best[0]:.3g} bounds"
    print(f"[mutants] {module} {mut}: {best[1]} {moved}")
    assert best[0] > SEEN, f"{module} {mut}: no drawn case moves by more than {best[0]:.3g} bounds ({best[1]})"


# ------------------------------------------------------------------------------------------------------------ the optimiser
def _optim_share(run, name, hi, betas, eps):
    r64, t32 = oc.reference(name, hi, oc.STEPS, betas, eps)
    return max(e / bound for e, _, bound in oc.rule(run, t32, r64).values())


def test_optim_manual_formulas_are_torchs_adam():
    for name, hi, betas, eps in oc.DRAWN:
        init, seq = oc.inputs(name, hi)
        man = oc.manual_run(init, seq, oc.HYPERS[hi], betas, eps)
        r64 = oc.reference(name, hi, oc.STEPS, betas, eps)[0]
        for key in man:
            for m, r in zip(man[key], r64[key]):
                assert (m is None) == (r is None), (name, hi, key)
                if r is not None and r.numel():
                    torch.testing.assert_close(m, r, rtol=1e-9, atol=1e-12 * float(r.abs().max()), msg=f"{name}-h{hi} {key}")


@pytest.mark.parametrize("mut", oc.MUTANTS)
def test_optim_each_mistake_is_seen(mut):
    best = (0.0, None)
    for name, hi, betas, eps in oc.DRAWN:
        init, seq = oc.inputs(name, hi)
        share = _optim_share(oc.manual_run(init, seq, oc.HYPERS[hi], betas, eps, mut), name, hi, betas, eps)
        if share > best[0]:
            best = (share, f"{name}-h{hi}" + ("" if (betas, eps) == (oc.BETAS, oc.EPS) else f"-betas{betas}-eps{eps}"))
    _report("optim", mut, best)


def test_optim_new_cases_leave_room():
    """The rule measures ours by torch's own float32 error, so torch32 itself uses at most a quarter of it by construction;
    what is held to ROOM is the correct walk in float64 (the mistakes' baseline) and, printed beside it, the kernel's
    documented arithmetic walked in float32, which must stay inside the bound."""
    new = [d for d in oc.DRAWN if d[1] == oc.TINY or d in oc.OFF_DEFAULT]
    assert len(new) == len([n for n in oc.SETS if n not in oc.OWN_TESTS]) + len(oc.OFF_DEFAULT)
    for name, hi, betas, eps in new:
        init, seq = oc.inputs(name, hi)
        exact = _optim_share(oc.manual_run(init, seq, oc.HYPERS[hi], betas, eps), name, hi, betas, eps)
        walk = _optim_share(oc.manual_run(init, seq, oc.HYPERS[hi], betas, eps, dtype=torch.float32), name, hi, betas, eps)
        print(f"[mutants] optim room {name}-h{hi} betas {betas} eps {eps}: float64 walk {exact:.3g}, float32 contract {walk:.3g}")
        assert exact < ROOM and walk <= 1.0, (name, hi, exact, walk)


# ------------------------------------------------------------------------------------------------------- the eval-mode MLP
@functools.lru_cache(maxsize=None)
def _infer_case(case, B, small):
    """(the restatement, X64, its logits, the rule's bound), once: nothing that reads them modifies them."""
    _, ref = (ic.small_pair if small else ic.pair)(case)
    X = (ic.small_inputs if small else ic.inputs)(case, B).double()
    return (ref, X) + ic.ref_out(ref, X)


def _infer_name(case, B, small):
    return f"{case[0]}{'-small_var' if small else ''} B={B}"


def test_infer_manual_formulas_are_the_restatement():
    for case, B, small in ic.DRAWN:
        if B > ic.SMALL_ROWS:
            continue
        ref, X, want, _ = _infer_case(case, B, small)
        torch.testing.assert_close(ic.manual64(ref, X)[0], want, rtol=1e-9, atol=1e-12 * float(want.abs().max()),
                                   msg=_infer_name(case, B, small))


@pytest.mark.parametrize("mut", ic.MUTANTS)
def test_infer_each_mistake_is_seen(mut):
    best = (0.0, None)
    for case, B, small in ic.DRAWN:
        if B > ic.SMALL_ROWS and best[0] > SEEN:             # the 1000-row cases only where the smaller ones do not see it
            continue
        ref, X, want, bound = _infer_case(case, B, small)
        s = ic.share(ic.manual64(ref, X, mut)[0], want, bound)
        if s > best[0]:
            best = (s, _infer_name(case, B, small))
    _report("infer", mut, best)


def test_infer_small_variance_cases_leave_room():
    """Float32 torch (the restatement's own ops) and the kernels' documented fold, walked in float32."""
    for case, B in ic.SMALL_DRAWN:
        ref, X, want, bound = _infer_case(case, B, True)
        ref32 = copy.deepcopy(ref).float()
        with torch.no_grad():
            t32 = ic.share(ref32(X.float(), None), want, bound)
        fold = ic.share(ic.manual64(ref, X, dtype=torch.float32)[0], want, bound)
        print(f"[mutants] infer room {_infer_name(case, B, True)}: float32 torch {t32:.3g}, float32 fold {fold:.3g}")
        assert t32 < ROOM and fold < ROOM, (case[0], t32, fold)


# ----------------------------------------------------------------------------------------------------- the evaluation head
def _valid_rows(z, y, kw):
    """(logits, labels) of the rows that enter the loss, for torch's own nll_loss."""
    ref = ec.head64(z, y, **kw)
    keep = ref["flag"] <= ec.CORRECT
    rows = kw.get("rows", torch.arange(keep.numel()))[keep]
    lrows = kw.get("label_rows", torch.arange(keep.numel()))[keep]
    return ref, z[rows], y[lrows]


def test_head_manual_formulas_are_torchs_nll_loss_and_argmax():
    for name, z, y, kw, _ in ec.head_drawn():
        ref, zz, yy = _valid_rows(z, y, kw)
        if yy.numel():
            want = float(ec.nll64(zz, yy))
            assert abs(ref["loss"] - want) <= 1e-9 * abs(want) or (ref["loss"] != ref["loss"] and want != want), name
        else:
            assert ref["loss"] != ref["loss"], name
        if "rows" not in kw:
            assert torch.equal(ref["pred"], torch.argmax(z, dim=1)), name
    ref = ec.head64(*ec.ties_case())
    assert ref["pred"].tolist() == [0, 63, 64, 100, 5, 64, 0, 10] and ref["flag"].tolist() == [1, 1, 1, 1, 2, 2, 2, 2]
    assert ref["counts"] == [4, 4, 4, 0] and ref["acc"] == 0.5
    z, y, y2, rows, lrows, ignored, bad = ec.ignored_case()
    ref = ec.head64(z, y2, rows=rows, label_rows=lrows)
    assert ref["flag"][ignored].tolist() == [2, 2] and ref["flag"][bad].tolist() == [3] * 7 and ref["pred"][[9, 10]].tolist() == [-1, -1]
    assert ref["counts"][0] == 300 - 9 and ref["counts"][2:] == [2, 7]


@pytest.mark.parametrize("mut", ec.BOOKKEEPING)
def test_head_each_mistake_is_seen(mut):
    best = (0.0, None)
    for name, z, y, kw, loss_held in ec.head_drawn():
        ref, zz, yy = _valid_rows(z, y, kw)
        loss32 = ec.nll32_on(zz, yy) if yy.numel() else float("nan")
        s = ec.head_share(ec.head64(z, y, mut=mut, **kw), ref, loss32, loss_held)
        if s > best[0]:
            best = (s, name)
    _report("evaluate", mut, best)


def test_head_mistakes_are_each_judged_or_declared():
    assert set(ec.MUTANTS) == set(ec.BOOKKEEPING + ec.HEAD_ARITHMETIC + ec.REDUCE_MUTANTS) and len(set(ec.MUTANTS)) == len(ec.MUTANTS)
    assert set(ec.INDISTINGUISHABLE) <= set(ec.MUTANTS)


def test_head_edge_cases_hold_what_their_names_say():
    """The list the GPU file parametrises over: every family at every class count where it exists, 65 rows, labels inside
    [0, C) that reach C-1, 64 and beyond, the argmax and the argmin; the four rows of `special` are what they are named."""
    fams = {}
    for name, z, y, kw in ec.EDGE_DRAWN:
        fams.setdefault(ec.edge_family(name), []).append(z.shape[1])
        assert z.dtype == torch.float32 and y.dtype == torch.int64 and int(y.min()) >= 0 and int(y.max()) < z.shape[1], name
        if not kw:
            assert z.shape[0] == y.numel() == ec.EDGE_N, name
            last = z.shape[1] - 1
            if ec.edge_family(name) in ("masked", "special") and last % 3 == 2:
                last -= 1                                    # the last finite class
            assert int(y[1]) == last and int(y[0]) == 0 and int(y[3]) == min(64, last), name
        for idx in kw.values():
            assert int(idx.min()) >= 0 and int(idx.max()) < z.shape[0], name
    every = list(ec.EDGE_C)
    assert fams == {"wide": every, "huge": every, "confident": every, "flat": every, "flat signed zeros": every,
                    "masked": [C for C in every if C >= 3], "special": [C for C in every if C >= 65], "gathered4096": [4096]}
    for name in ec.EDGE_NAMES:
        ref, fam = ec.edge_reference(name), ec.edge_family(name)
        odd = [i for i in range(ref["nll"].numel()) if not math.isfinite(float(ref["nll"][i]))]
        assert odd == (list(ec.EDGE_SPECIAL_ROWS) if fam == "special" else []), name
        if fam == "special":
            assert float(ref["nll"][5]) == math.inf and all(math.isnan(float(ref["nll"][i])) for i in (17, 40, 64)), name
            assert ref["pred"][[17, 40, 64]].tolist() == [ref["zz"].shape[1] - 1, 64, 0] and int(ref["flag"][64]) == ec.CORRECT
        if fam in ("masked", "special"):
            assert bool(torch.isinf(ref["zz"][:, 2::3]).all()), name
        if fam == "flat":
            assert float((ref["nll"] - math.log(ref["zz"].shape[1])).abs().max()) < 1e-12 and not bool(ref["pred"].any()), name
        if fam == "flat signed zeros":
            z = ref["zz"][::2]                               # the rows with a -0.0 first and a 0.0 after it
            assert not bool(ref["pred"].any()) and (z.shape[1] == 1 or bool((torch.signbit(z).any(dim=1) & ~torch.signbit(z).all(dim=1)).all())), name
        if fam == "confident" and ref["zz"].shape[1] > 1:
            assert 0.0 < float(ref["nll"].min()) and float(ref["nll"].max()) < 1e-8, name
        if fam in ("wide", "huge") and ref["zz"].shape[1] > 2:
            assert float(ref["nll"].max()) > (100.0 if fam == "wide" else 1e4), name


@functools.lru_cache(maxsize=None)
def _edge_head64(name):
    """head64 without a mistake on a case of EDGE_DRAWN, once."""
    _, z, y, kw = ec.EDGE_DRAWN[ec.EDGE_NAMES.index(name)]
    return ec.head64(z, y, **kw)


def test_head_edge_formulas_are_torchs_nll_loss_and_argmax():
    for name, z, y, kw in ec.EDGE_DRAWN:
        got, ref = _edge_head64(name), ec.edge_reference(name)
        assert torch.equal(got["pred"], ref["pred"]) and torch.equal(got["flag"], ref["flag"]) and got["counts"] == ref["counts"], name
        assert float(np.float32(got["acc"])) == ref["acc"], name
        torch.testing.assert_close(got["nll"], ref["nll"], rtol=1e-9, atol=0.0, equal_nan=True, msg=name)
        want = ref["mean"]
        assert (math.isnan(want) and math.isnan(got["loss"])) or got["loss"] == want or abs(got["loss"] - want) <= 1e-9 * abs(want), name
        # the formulas that take the mistakes, with none: a float64 sum of C terms exp(z - m) <= 1 rounds at most C - 1 partial
        # sums by 2^-53 each, in torch's log_softmax and here, in whatever order each adds; relative to a sum of at least 1
        # that is an absolute 2^-53 C on the logarithm, and at the `confident` losses of 1e-12 all that separates the two
        out = ec.head64(z, y, mut=ec.WRITTEN_OUT, **kw)["nll"]
        torch.testing.assert_close(out, ref["nll"], rtol=1e-9, atol=2.0 ** -53 * (z.shape[1] + 2), equal_nan=True, msg=name)
        # row_bound64, the one-row form, is the same function
        i = ref["nll"].numel() - 1
        one = ec.row_bound64(ref["zz"][i], ref["yy"][i])
        assert all(a == float(b) or (a != a and float(b) != float(b)) for a, b in zip(one, (ref["nll"][i], ref["bound"][i]))), name


@pytest.mark.parametrize("mut", [m for m in ec.HEAD_ARITHMETIC if m not in ec.INDISTINGUISHABLE])
def test_head_each_arithmetic_mistake_is_seen_at_the_edges(mut):
    """Either way counts: a quantity the GPU file holds exactly (the first such case is printed), or a row moved by more
    than SEEN of its row_bound64 (the largest such move)."""
    best, exact = (0.0, None), None
    for name, z, y, kw in ec.EDGE_DRAWN:
        s = ec.edge_share(ec.head64(z, y, mut=mut, **kw), _edge_head64(name), ec.edge_reference(name)["bound"])
        if math.isinf(s):
            exact = exact or name
        elif s > best[0]:
            best = (s, name)
    print(f"[mutants] evaluate {mut}: held exactly in {exact}; the largest move of a finite row is {best[0]:.3g} bounds ({best[1]})")
    _report("evaluate", mut, (math.inf, exact) if exact else best)


@pytest.mark.parametrize("mut", [m for m in ec.REDUCE_MUTANTS if m not in ec.INDISTINGUISHABLE])
def test_reduce_each_mistake_is_seen(mut):
    best = (0.0, None)
    for name, n, absorb in ec.reduce_drawn():
        nll, flag, loss64, counts = ec.reduce_case(n, absorb=absorb)
        assert ec.reduce_share(ec.reduce64(nll, flag), loss64, counts, n) <= 2.0 ** -29, name     # the float64 sum itself
        s = ec.reduce_share(ec.reduce64(nll, flag, mut), loss64, counts, n)
        print(f"[mutants] evaluate {mut}: {name} {s:.3g} bounds")
        if s > best[0]:
            best = (s, name)
    _report("evaluate", mut, best)


def test_head_walk_in_float32_stays_inside_the_row_bound():
    """row_bound64 is a worst-case derivation, so the kernel's order walked in float32 is held to the bound itself; its
    share is printed per family beside ROOM, which is not asserted (as for §7g's walk)."""
    worst = {}
    for name, z, y, kw in ec.EDGE_DRAWN:
        ref = ec.edge_reference(name)
        walk = torch.from_numpy(ec.head_walk32(ref["zz"], ref["yy"])).double()
        fin = torch.isfinite(ref["nll"])
        assert torch.equal(torch.nan_to_num(walk[~fin], nan=1.0), torch.nan_to_num(ref["nll"][~fin], nan=1.0)), name
        share = float(((walk - ref["nll"]).abs()[fin] / ref["bound"][fin]).max())
        assert share <= 1.0, (name, share)
        fam = ec.edge_family(name)
        worst[fam] = max(worst.get(fam, (0.0, "")), (share, name))
    for fam, (share, name) in worst.items():
        print(f"[mutants] evaluate walk {fam}: the float32 walk uses {share:.3g} of the row bound at most ({name}); ROOM is {ROOM}")


# ------------------------------------------------------------------------------------------------------ propagate_features
def _propagate_small(case):
    return len(pc.graph(case.graph)[0]) * case.F <= 6000 * 128


def test_propagate_manual_formulas_are_the_restatement():
    for case in filter(_propagate_small, pc.ALL_CASES):
        ref = pc.reference(case)
        np.testing.assert_allclose(pc.propagate_manual64(case), ref, rtol=1e-9, atol=1e-12 * np.abs(ref).max(), err_msg=str(case))


@pytest.mark.parametrize("mut", pc.MUTANTS)
def test_propagate_each_mistake_is_seen(mut):
    best = (0.0, None)
    for case in pc.ALL_CASES:
        if not _propagate_small(case) and best[0] > SEEN:    # the wide products only where the others do not see it
            continue
        s = pc.share(pc.propagate_manual64(case, mut), pc.reference(case))
        if s > best[0]:
            best = (s, str(case))
    _report("propagate", mut, best)


def test_propagate_row_at_the_epsilons_scale_leaves_room():
    """The row whose float32 weights sum to 1e-12, in the numpy statement of the kernel's arithmetic: by itself and with
    every other row, below ROOM of the tolerance in each weighted case."""
    tiny = pc.tiny_row("hub")
    indptr = pc.graph("hub")[0]
    w = pc.edge_weights("hub")[0]
    assert abs(float(w[indptr[tiny]:indptr[tiny + 1]].astype(np.float64).sum()) - 1e-12) < 1e-18 and tiny != pc.edge_weights("hub")[1]
    worst = (0.0, None)
    for case in [c for c in pc.ALL_CASES if c.weighted]:
        indptr, indices, w, X = pc.inputs(case)
        ref = pc.reference(case)
        emu = pc.emulate_fp32_storage(indptr, indices, w, X, case.mode, case.order, case.alpha)
        row = float((np.abs(emu[tiny] - ref[tiny]) / pc.tolerance(ref)[tiny]).max())
        assert np.abs(ref[tiny]).max() > 0.01 * np.abs(ref).max(), case          # the row is not lost beside the others
        worst = max(worst, (max(row, pc.share(emu, ref)), str(case)))
    print(f"[mutants] propagate room: fp32 storage uses {worst[0]:.3g} of the tolerance at most ({worst[1]})")
    assert worst[0] < ROOM


# ----------------------------------------------------------------------------------------------------------- the objective
_OBJECTIVE = [(c, k) for c, coeffs in jc.DRAWN if c.B <= 1000 for k in coeffs]        # without the second grid-stride trip


def test_objective_manual_formulas_are_the_reference():
    for case, coeffs in _OBJECTIVE:
        ref, man = jc.reference(case, tuple(coeffs)), jc.manual(case, tuple(coeffs))
        for k in ("loss", "sup", "con"):
            assert (math.isnan(ref[k]) and math.isnan(man[k])) or abs(man[k] - ref[k]) <= 1e-9 * abs(ref[k]) + 1e-300, (case, k)
        torch.testing.assert_close(man["grad"], ref["grad"], rtol=1e-9, atol=1e-12 * max(1e-300, float(ref["grad"].abs().max())),
                                   equal_nan=True, msg=jc.case_id(case))


def _objective_best(mut):
    """(the largest finite share, its case, whether some case turns a finite value into one that is not)."""
    best, broken = (0.0, None), None
    for case, coeffs in _OBJECTIVE:
        s = jc.share(jc.manual(case, tuple(coeffs), mut), jc.reference(case, tuple(coeffs)))
        if math.isinf(s):
            broken = broken or f"{jc.case_id(case)} {tuple(coeffs)}"
        elif s > best[0]:
            best = (s, f"{jc.case_id(case)} {tuple(coeffs)}")
    return best, broken


@pytest.mark.parametrize("mut", [m for m in jc.MUTANTS if m not in jc.INDISTINGUISHABLE])
def test_objective_each_mistake_is_seen(mut):
    best, broken = _objective_best(mut)
    if broken:
        print(f"[mutants] objective {mut}: not finite where the reference is, in {broken}")
    _report("objective", mut, best)


@pytest.mark.parametrize("mut", jc.INDISTINGUISHABLE)
def test_objective_the_indistinguishable_mistake_moves_nothing(mut):
    """See objective_cases.INDISTINGUISHABLE: the cases keep away from the tie that would tell the two apart."""
    best, broken = _objective_best(mut)
    print(f"[mutants] objective {mut} (declared indistinguishable): the largest share is {best[0]:.3g} ({best[1]})")
    assert best[0] < ROOM and broken is None


# ------------------------------------------------------------------------------------- random_prop and the embedding bag
@functools.lru_cache(maxsize=None)
def _augment_drawn():
    """[(name, kind, case, training, ref, terms)], the references computed once."""
    out = []
    for name, kind, c, training in ac.drawn_forward():
        ref, terms = ac.coo_reference(c, training) if kind == "coo" else ac.bag_reference(c, training)[:2]
        out.append((name, kind, c, training, ref, terms))
    return out


def _augment_manual(kind, c, training, mut=None):
    return ac.coo_manual64(c, training, mut) if kind == "coo" else ac.bag_manual64(c, training, mut)


def test_augment_manual_formulas_are_the_references():
    for name, kind, c, training, ref, _ in _augment_drawn():
        torch.testing.assert_close(_augment_manual(kind, c, training), ref, rtol=1e-9, atol=1e-12 * float(ref.abs().max()), msg=name)


# the bag takes one mask, so it has no samples to confuse: every other pair of mistake and operation
@pytest.mark.parametrize("mut,kind", [(m, k) for m in ac.MUTANTS for k in ("coo", "bag") if (m, k) != ("sample0_mask_for_all", "bag")])
def test_augment_each_mistake_is_seen(mut, kind):
    """Per operation: random_prop (rows and COO forms share the COO reference) and the embedding bag."""
    best, broken = (0.0, None), None
    for name, k, c, training, ref, terms in _augment_drawn():
        if k != kind:
            continue
        s, bad = ac.finite_ratio(_augment_manual(kind, c, training, mut), ref, terms)
        broken = broken or (name if bad else None)
        if s > best[0]:
            best = (s, name)
    if broken:
        print(f"[mutants] augment {kind} {mut}: not finite where the reference is, in {broken}")
    _report(f"augment {kind}", mut, best)


def test_augment_bags_at_the_epsilons_scale_leave_room():
    for H in ac.TINY_BAG_H:
        for training in (False, True):
            c = ac.tiny_bags(H)
            ref, terms, dW, dW_terms = ac.bag_reference(c, training)
            out, g = ac.f32_bag(c, training)
            share = max(ac.ratio(out, ref, terms), ac.ratio(g, dW, dW_terms))
            print(f"[mutants] augment room tiny bag H={H} training={training}: the float32 walk uses {share:.3g} of the bound")
            assert share < ROOM


# ------------------------------------------------------------------------------------------------------ MAG's front end
def _mag_args(name):
    c = gc.case(name)
    H, K, S, filled, mode, p_node, p_in, training, bags = gc.CASES[name]
    return c, (c["P"], c["batch"], S, p_node, p_in, training, c["keep"], gc.SEED)


_MAG = [n for n in gc.CASES if n != "hub"]                  # the hub's bag of 4 097 entries: one case of 14, left to the GPU


def test_mag_manual_formulas_are_the_reference():
    for name in _MAG:
        c, args = _mag_args(name)
        ref = c["ref"][0]
        torch.testing.assert_close(gc.manual64(*args), ref, rtol=1e-9, atol=1e-12 * float(ref.abs().max()), msg=name)


@pytest.mark.parametrize("mut", gc.MUTANTS)
def test_mag_each_mistake_is_seen(mut):
    best, broken = (0.0, None), None
    for name in _MAG:
        c, args = _mag_args(name)
        got = gc.manual64(*args, mut=mut)
        ok = torch.isfinite(got)
        r = ((got - c["ref"][0]).abs() / gc.bound(c["ref"][1], c["roundings"]))[ok]
        broken = broken or (name if not bool(ok.all()) else None)
        if r.numel() and float(r.max()) > best[0]:
            best = (float(r.max()), name)
    if broken:
        print(f"[mutants] mag {mut}: not finite where the reference is, in {broken}")
    _report("mag", mut, best)


def test_mag_case_at_the_epsilons_scale_leaves_room():
    c, args = _mag_args("eps_scale")
    emu = gc.emulate(*args)
    share = float(((emu.double() - c["ref"][0]).abs() / gc.bound(c["ref"][1], c["roundings"])).max())
    print(f"[mutants] mag room eps_scale: the float32 walk of the order contract uses {share:.3g} of the bound")
    assert share < ROOM
