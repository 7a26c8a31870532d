"""The float64 restatements the training kernels are held to, against recorded runs of the real reference.

tests/golden/train_*.npz hold what the reference's own model.py and model_mag.py computed on recorded inputs and recorded
dropout masks (tests/golden/make_training_golden.py).  Here, with no GPU and without the reference tree: every restatement
on those inputs gives the recorded outputs (rtol 1e-9, atol 1e-12 max|ref|; NaN in the same places; integers and booleans
exactly); the first steps of main() replayed through the restatements give the recorded losses, norms, parameters and
moments; the early-stop rule gives the recorded saves and stop; and each misreading of the reference that the suite could
not see before moves some fixture by more than SEEN of that quantity's bound.  The last test re-runs the recorder where the
reference tree is present and finds every committed array bit-equal."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

import augment_cases as ac
import evaluate_cases as ec
import mag_cases as gc
import objective_cases as jc
import optim_cases as oc
import reference_training_cases as rc
from oracle.objective_ref import consis_loss_ref
from oracle.random_prop_ref import random_prop_ref
from test_host_mlp_block import SEEN


def _report(what, mut, share, case):
    moved = "differs in a quantity held exactly, or is not finite" if math.isinf(share) else f"moves by {share:.3g} bounds"
    print(f"[mutants] reference {what} {mut}: {case} {moved}")
    assert share > SEEN, f"{what} {mut}: {case} moves by {share:.3g} bounds only"


# --------------------------------------------------------------------------------------- restatements against the pieces
@pytest.mark.parametrize("training", [True, False])
def test_random_prop_ref_is_the_reference(training):
    d, c = rc.load("train_pieces.npz"), rc.rp_case(training)
    mode = "train" if training else "eval"
    out = random_prop_ref(c.feats, c.scores, c.idx, c.p, training, c.keep[0])
    assert out.shape[0] == rc.B                                    # dim_size = mat_idx[-1] + 1 (model.py:84)
    rc.close64(out, d[f"rp_{mode}_out"], f"random_prop {mode}")
    rc.close64(ac.coo_manual64(c, training)[0], d[f"rp_{mode}_out"], f"coo_manual64 {mode}")
    rc.close64(ac.coo_ref_grad(c, training, x=c.X)[0], d[f"rp_{mode}_dX"], f"random_prop {mode} dX")
    assert not out[35].any() and (not training or not out[10].any())          # the empty row; the row dropped whole


@pytest.mark.parametrize("tag", rc.mlp_tags())
def test_mlp_ref_is_the_reference(tag):
    d = rc.load("train_pieces.npz")
    ref, c = rc.mlp_ref(tag)
    X, G = rc.t(d["mlp_X"]), rc.t(d["mlp_G"])
    with torch.no_grad():
        rc.close64(ref.eval()(X, None), d[tag + "__eval_out"], tag + " eval")
    x = X.clone().requires_grad_(True)
    out = ref.train()(x, rc.mlp_keeps(tag, c["nlayers"]))
    (out * G).sum().backward()
    rc.close64(out.detach(), d[tag + "__train_out"], tag + " train")
    after = {k: v for k, v in ref.state_dict().items() if "running" in k}
    assert sorted(after) == sorted(k for k in rc.sub(d, tag + "__after__") if "running" in k)
    for k, v in after.items():
        rc.close64(v, d[f"{tag}__after__{k}"], f"{tag} {k}")
    grads = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    assert sorted(grads) == sorted(rc.sub(d, tag + "__grad__")), tag      # the same parameters are trained
    for k, g in grads.items():
        rc.close64(g, d[f"{tag}__grad__{k}"], f"{tag} d{k}")
    if c["node_norm"]:
        assert tag + "__dX" not in d and (x.grad is None or not x.grad.any())      # X is detached (model.py:50)
    else:
        rc.close64(x.grad, d[tag + "__dX"], tag + " dX")


def _consis_cases():
    return sorted(rc.meta()["consis_loss"]["cases"].items())


def _consis_manual(lp, c, mut=None):
    leaf = lp.clone().requires_grad_(True)
    con = jc.manual_terms(leaf, torch.zeros(1, dtype=torch.int64), 0, 1.0, c["tem"], c["conf"], c["kind"], log_probs=True, mut=mut)[2]
    con.backward()
    return con.detach(), leaf.grad


def test_consis_loss_ref_is_the_reference():
    d = rc.load("train_pieces.npz")
    nans = 0
    for tag, c in _consis_cases():
        lp = rc.t(d[f"cl_S{c['S']}_logp"])
        leaves = [lp[s].clone().requires_grad_(True) for s in range(c["S"])]
        loss = consis_loss_ref(leaves, c["tem"], c["conf"], c["kind"])
        loss.backward()
        rc.close64(loss.detach(), d[tag + "__loss"], tag)
        rc.close64(torch.stack([x.grad for x in leaves]), d[tag + "__grad"], tag + " grad")
        con, grad = _consis_manual(lp, c)
        rc.close64(con, d[tag + "__loss"], tag + " manual")
        rc.close64(grad, d[tag + "__grad"], tag + " manual grad")
        assert bool(np.isnan(d[tag + "__loss"])) == c["nan"] == (c["passing"] == 0)
        nans += c["nan"]
    assert nans == 12 and len(_consis_cases()) == 36                # kl, l2 x S 1, 2, 4 x tem 0.5, 0.1 x some, none, tie


@pytest.mark.parametrize("tag", rc.mag_tags())
@pytest.mark.parametrize("mode", rc.MAG_MODES)
def test_mag_restatements_are_the_reference(tag, mode):
    d = rc.load("train_mag.npz")
    got = rc.mag_chain64(tag, mode)
    for k in ("emb", "prop", "out", "demb", "dprop"):
        rc.close64(got[k], d[f"{tag}__{mode}_{k}"], f"{tag} {mode} {k}")
    if mode != "train0":
        training = mode == "train"
        rc.close64(ac.bag_manual64(rc.mag_bag_case(tag, training), training), d[f"{tag}__{mode}_emb"], f"{tag} {mode} bag_manual64")
    assert sorted(got["grads"]) == sorted(rc.sub(d, f"{tag}__{mode}_grad__")), tag
    for k, g in got["grads"].items():
        rc.close64(g, d[f"{tag}__{mode}_grad__{k}"], f"{tag} {mode} d{k}")
    if mode == "train":
        for k, v in got["after"].items():
            rc.close64(v, d[f"{tag}__after__{k}"], f"{tag} {k}")
    nbr, idx = d["mag_nbr"], d["mag_idx"]
    assert not got["emb"][nbr == 14].any() and not got["prop"][30].any() and (idx == 30).any()      # the empty bag, in the middle


@pytest.mark.parametrize("tag", rc.mag_tags())
@pytest.mark.parametrize("mode", ["eval", "train0"])
def test_mag_cases_references_are_the_reference(tag, mode):
    """mag_cases.chain64, manual64 and ref64, which hold mag_prop_rows and carry their own 1e-10 and 1e-12, on the
    fixture's bags and resident rows."""
    d = rc.load("train_mag.npz")
    P, keep, training = rc.mag_problem(tag, mode)
    args = (P, None, 1, float(d["mag_p"][0]), 0.0, training, keep, 0)
    want = d[f"{tag}__{mode}_prop"]
    rc.close64(gc.chain64(P, P.W.double(), *args[1:])[0], want, f"{tag} {mode} chain64")
    rc.close64(gc.manual64(*args)[0], want, f"{tag} {mode} manual64")
    out, _terms, dW, _dWt = gc.ref64(*args, G=rc.t(d[f"{tag}__{mode}_dprop"])[None])
    rc.close64(out[0], want, f"{tag} {mode} ref64")
    rc.close64(dW, d[f"{tag}__{mode}_grad__embeds.weight"], f"{tag} {mode} ref64 dW")


# ------------------------------------------------------------------------------------------------------------- the runs
@pytest.mark.parametrize("name", rc.RUNS)
def test_replayed_steps_are_the_reference_run(name):
    d, steps = rc.load(f"train_run_{name}.npz"), rc.replay64(name)
    assert len(steps) == 4
    for i, st in enumerate(steps):
        p = f"r64_s{i}_"
        rc.close64(st["loss"], d[p + "loss"], f"{name} step {i} loss")
        rc.close64(st["grad_norm"], d[p + "grad_norm"], f"{name} step {i} grad norm")
        assert sorted("mlp." + k for k in st["pre"]) == sorted(rc.sub(d, p + "pre__")), (name, i)
        for k in st["pre"]:
            rc.close64(st["pre"][k], d[f"{p}pre__mlp.{k}"], f"{name} step {i} d{k}")
            rc.close64(st["m"][k], d[f"{p}m__mlp.{k}"], f"{name} step {i} exp_avg {k}")
            rc.close64(st["v"][k], d[f"{p}v__mlp.{k}"], f"{name} step {i} exp_avg_sq {k}")
        for k, v in st["state"].items():
            if "num_batches" not in k:
                rc.close64(v, d[f"{p}state__mlp.{k}"], f"{name} step {i} {k}")


@pytest.mark.parametrize("name", rc.RUNS)
def test_manual_adam_is_the_reference_run(name):
    """optim_cases.manual_run, the formulas the optimiser's mistakes are built into, over the run's recorded gradients."""
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    names = sorted(k for k in rc.sub(d, "r64_s0_pre__"))
    init = [rc.t(d["r64_init__" + k]) for k in names]
    seq = [[rc.t(d[f"r64_s{i}_pre__{k}"]) for k in names] for i in range(a["steps_recorded"])]
    run = oc.manual_run(init, seq, dict(lr=a["lr"], weight_decay=a["weight_decay"], clip=a["clip_norm"]))
    last = f"r64_s{a['steps_recorded'] - 1}_"
    for j, k in enumerate(names):
        rc.close64(run["param"][j], d[f"{last}state__{k}"], f"{name} {k}")
        rc.close64(run["exp_avg"][j], d[f"{last}m__{k}"], f"{name} exp_avg {k}")
        rc.close64(run["exp_avg_sq"][j], d[f"{last}v__{k}"], f"{name} exp_avg_sq {k}")


def _implied_weight(d, i):
    """(loss - mean of the samples' supervised terms) / consis_loss's value, from the float64 run's own numbers."""
    return (float(d[f"r64_s{i}_loss"]) - float(d[f"r64_s{i}_sup"].mean())) / float(d[f"r64_s{i}_con"])


@pytest.mark.parametrize("name", rc.RUNS)
def test_step_weight_is_the_weight_of_the_recorded_run(name):
    from grand_plus_amd.step import step_weight
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    for i in range(a["steps_recorded"]):
        tick = int(d[f"s{i}_num_batch"]) + 1
        assert tick == i + 1
        w, implied = float(step_weight(a["lam"], a["warmup"], tick)), _implied_weight(d, i)
        # the quotient carries the roundings of the loss (2^-53 of about 2) over con; the weight itself is a float32
        assert abs(w - implied) <= 2.0 ** -24 * abs(implied) + 2.0 ** -50 / abs(float(d[f"r64_s{i}_con"])), (name, i, w, implied)
    assert _implied_weight(d, 0) == 0.0 and a["warmup"] > a["steps_recorded"]         # the ramp starts at 0 and is not over


def _validated_ticks(eval_batch, n_steps, rule=None):
    """The steps t = 1 .. n_steps after which the loop validates: fit.validates_at, the one test FitLoop.advance makes."""
    from grand_plus_amd.fit import validates_at
    return [tk for tk in range(1, n_steps + 1) if (rule or validates_at)(tk, eval_batch)]


@pytest.mark.parametrize("name", rc.RUNS)
def test_fit_validates_where_the_reference_run_did(name):
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    at = d["r64_valid"][:, 0].astype(np.int64)
    assert np.array_equal(at, d["t32_valid"][:, 0].astype(np.int64)) and len(at) >= 3
    ticks = _validated_ticks(a["eval_batch"], int(d["r64_num_batch"]))
    assert [tk - 1 for tk in ticks] == at.tolist()                  # num_batch counts finished steps before this one


@pytest.mark.parametrize("name", rc.RUNS)
def test_valid64_and_predict64_are_the_reference_run(name):
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    _seeds, col, val, filled, where = rc.resident_rows(name)
    X, y = rc.t(d["features"]), rc.t(d["labels"]).long()
    pos = torch.tensor([where[int(i)] for i in d["idx_val"]])
    seen = 0
    for nb, loss, acc in d["r64_valid"]:
        if int(nb) >= a["steps_recorded"]:
            continue
        ref = rc.run_model64(name, rc.sub(d, f"r64_s{int(nb)}_state__")).eval()
        r = ec.valid64(ref, X, col, val, filled, rc.K, pos, y[rc.t(d["idx_val"])])
        rc.close64(r["loss"], loss, f"{name} valid at {int(nb)}")
        # evaluate_cases.head64, the restatement of valid's tail (model.py:163-166) that the evaluation head is held to, on
        # the float64 logits of the recorded validation rows
        e_idx, e_cols, e_scores, _ = ac.rows_to_coo(col, val, filled, rc.K, pos)
        with torch.no_grad():
            z = ref(random_prop_ref(X[e_cols], e_scores.double(), e_idx, a["dropnode_rate"], False), None)
        head = ec.head64(z, y[rc.t(d["idx_val"])])
        rc.close64(head["loss"], loss, f"{name} head64 at {int(nb)}")
        assert head["acc"] == acc and head["counts"] == [len(pos), round(acc * len(pos)), 0, 0], (name, nb)
        assert float((r["pred"] == y[rc.t(d["idx_val"])]).double().mean()) == acc, (name, nb)
        seen += 1
    assert seen == 2
    from oracle.predict_ref import propagate_ref
    rc.close64(propagate_ref(rc.adjacency(name), d["features"], a["prop_mode"], a["order"], a["alpha"]), d["propagated"], f"{name} propagation")
    ref = rc.run_model64(name, rc.sub(d, "r64_final__")).eval()
    idx = rc.t(d["idx_test"])
    r = ec.predict64(ref, rc.adjacency(name), X, a["prop_mode"], a["order"], a["alpha"], idx, y[idx])
    assert float((r["pred"] == y[idx]).double().sum()) / len(idx) == float(d["r64_test_acc"]), name


# ------------------------------------------------------------------------------------------------------- early stopping
@pytest.mark.parametrize("mode", ["both", "acc"])
def test_early_stop_rule_is_the_reference_loop(mode):
    d = rc.load("train_stop.npz")
    saved, stop_tick = rc.drive_rule(mode)
    assert saved == d[f"{mode}_saved"].tolist()
    assert stop_tick is not None and stop_tick - 1 == int(d[f"{mode}_stop_at"]) == int(d[f"{mode}_eval_at"][-1])
    assert d[f"{mode}_eval_at"].tolist() == list(range(len(saved)))
    if mode == "both":                                               # the script holds what its comment says
        assert saved[:4] == [True, True, False, False] and not saved[8] and len(saved) == 10


# ---------------------------------------------------------------------------------------------------------------- teeth
def test_misread_epsilons_are_seen():
    """1e-10 in place of random_prop's 1e-12 (model.py:87), and 1e-12 in place of emb's 1e-10 (model_mag.py:54), under the
    bound of augment_cases."""
    d, c = rc.load("train_pieces.npz"), rc.rp_case(False)
    terms = ac.coo_reference(c, False)[1][0]
    ref = rc.t(d["rp_eval_out"])
    _report("random_prop", "1e-10 for 1e-12", ac.ratio(ac.coo_manual64(c, False, "den_eps_swapped")[0], ref, terms), "rp eval")
    dm, tag = rc.load("train_mag.npz"), rc.mag_tags()[0]
    bag = rc.mag_bag_case(tag, False)
    terms = ac.bag_reference(ac.Case(**{**bag.__dict__, "G": torch.zeros((bag.n_out, rc.H))}), False)[1]
    ref = rc.t(dm[tag + "__eval_emb"])
    _report("emb", "1e-12 for 1e-10", ac.ratio(ac.bag_manual64(bag, False, "den_eps_swapped"), ref, terms), tag)
    # the same pair in mag_cases' own formulas, under mag_cases' bound
    P, keep, training = rc.mag_problem(tag, "eval")
    args = (P, None, 1, float(dm["mag_p"][0]), 0.0, training, keep, 0)
    terms = gc.ref64(*args)[1][0]
    share = float(((gc.manual64(*args, mut="den_eps_swapped")[0] - rc.t(dm[tag + "__eval_prop"])).abs() / gc.bound(terms, gc.ROUNDINGS)).max())
    _report("mag_cases", "the two epsilons swapped", share, tag)


def test_misread_conf_comparison_is_seen():
    """`>=` for `>` at conf (model.py:134-136) on the cases whose conf is one row's own avg_p.max, under objective_cases' bound."""
    d, best = rc.load("train_pieces.npz"), (0.0, None)
    for tag, c in _consis_cases():
        if not tag.endswith("_tie"):
            continue
        con = _consis_manual(rc.t(d[f"cl_S{c['S']}_logp"]), c, "conf_ge")[0]
        e, b = jc.value_error(con, float(d[tag + "__loss"]))
        best = max(best, (e / b, tag))
    _report("consis_loss", "conf >=", *best)


@pytest.mark.parametrize("mut", ["ramp_from_t", "sup_not_divided"])
def test_misread_step_loss_is_seen(mut):
    """The ramp taken from t instead of t - 1 (model.py:329, 360) and the supervised sum not divided by S (model.py:327),
    in the loss of a recorded step, under four times the reference's own float32 error."""
    best = (0.0, None)
    for name in rc.RUNS:
        d = rc.load(f"train_run_{name}.npz")
        for i, st in enumerate(rc.replay64(name, mut)[:1]):          # the first step: later ones start from moved weights
            r, _e, bound = rc.run_bound(d, f"s{i}_loss")
            best = max(best, (abs(float(st["loss"]) - r) / bound, f"{name} step {i}"))
    _report("step loss", mut, *best)


def test_misread_cadence_is_seen():
    """Validation at t % eval_batch == 0 instead of (t - 1) % eval_batch == 0 (model.py:336, 360)."""
    d, a = rc.load("train_run_plain.npz"), rc.meta()["run_plain"]

    def shifted(tk, eval_batch):
        return tk % eval_batch == 0

    ticks = _validated_ticks(a["eval_batch"], int(d["r64_num_batch"]), shifted)
    same = [tk - 1 for tk in ticks] == d["r64_valid"][:, 0].astype(np.int64).tolist()
    _report("fit", "cadence shifted by one", 0.0 if same else math.inf, "run plain")


def test_misread_tie_branch_is_seen():
    """The tie with a higher loss under `both` counted as a bad evaluation (model.py:344-354: it is neither)."""
    d = rc.load("train_stop.npz")
    saved, stop_tick = rc.drive_rule("both", tie_is_bad=True)
    same = saved == d["both_saved"].tolist() and stop_tick - 1 == int(d["both_stop_at"])
    _report("early stop", "tie counted as bad", 0.0 if same else math.inf, "both")


# ------------------------------------------------------------------------------------------------------------ live check
def test_fixtures_match_live_reference():
    path = os.path.join(rc.GOLDEN, "make_training_golden.py")
    spec = importlib.util.spec_from_file_location("make_training_golden", path)
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    if not rec.available():
        pytest.skip("the reference tree or oracle/_ref is absent")
    files, meta = rec.record()
    assert sorted(files) == sorted(rc.FILES)
    for name, arrays in files.items():
        have = rc.load(name)
        assert sorted(arrays) == sorted(have), name
        for k, v in arrays.items():
            assert v.dtype == have[k].dtype and v.shape == have[k].shape and v.tobytes() == have[k].tobytes(), (name, k)
    import json
    assert json.loads(json.dumps(meta)) == rc.meta()
