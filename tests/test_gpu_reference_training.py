"""The training and evaluation kernels against recorded runs of the real reference.

tests/golden/train_*.npz hold what the reference's own model.py and model_mag.py computed on recorded inputs and recorded
dropout masks (tests/golden/make_training_golden.py); tests/test_host_reference_training.py holds the float64 restatements
to them.  Here the kernels run on the fixtures' inputs with `keep=` set to the recorded masks, and every comparison uses
the rule of the kernel's own GPU file: augment_cases.close (random_prop, the embedding bag), the whole-model MLP rule
of tests/test_gpu_mlp.py (mlp_block_cases.model_assert_out / model_assert_grad), objective_cases' value and gradient
rule, mag_cases.bound, evaluate_cases' loss bound and decided rows, propagate_cases.tolerance and optim_cases.rule.  The per-step loss and gradient norm of the replayed run, which had
no rule, are held to four times the reference's own float32 error |t32 - r64| with a floor of one float32 ulp.  Nothing
here reads the reference tree."""
import numpy as np
import pytest
import torch

import augment_cases as ac
import evaluate_cases as ec
import fit_cases as fc
import mag_cases as gc
import objective_cases as jc
import optim_cases as oc
import propagate_cases as pc
import reference_training_cases as rc
from mlp_block_cases import model_assert_grad as _assert_grad, model_assert_out as _assert_out

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ random_prop
@pytest.mark.parametrize("training", [True, False])
def test_random_prop_and_random_prop_rows(training):
    from grand_plus_amd.augment import random_prop, random_prop_rows
    d, c = rc.load("train_pieces.npz"), rc.rp_case(training)
    mode = "train" if training else "eval"
    ref, dX = rc.t(d[f"rp_{mode}_out"]), rc.t(d[f"rp_{mode}_dX"])
    terms, dterms = ac.coo_reference(c, training)[1][0], ac.coo_ref_grad(c, training, x=c.X)[1]
    G = c.G[0].float().cuda()
    # the reference's own signature
    X = c.X.float().cuda().requires_grad_(True)
    out = random_prop(X[c.cols.cuda()], c.scores.float().cuda(), c.idx.cuda(), c.p, training=training, keep=c.keep[0].cuda())
    assert tuple(out.shape) == (rc.B, rc.F)
    ac.close(out.detach(), ref, terms)
    out.backward(G)
    ac.close(X.grad, dX, dterms)
    # the resident rows: every entry in its slot
    col, val, filled, slot = rc.rp_rows(d)
    keep = rc.slot_keep(torch.from_numpy(slot), [c.keep[0]], rc.B * rc.K)[0]
    X2 = c.X.float().cuda().requires_grad_(True)
    out2 = random_prop_rows(X2, col.cuda(), val.cuda(), filled.cuda(), rc.K, dropnode_rate=c.p, training=training, keep=keep.cuda())
    ac.close(out2.detach(), ref, terms)
    out2.backward(G)
    ac.close(X2.grad, dX, dterms)
    assert not out[35].any() and not out2[35].any()                # the row without entries


# -------------------------------------------------------------------------------------------------------------------- MLP
def _check_param_grads(ours, want, cancelled=()):
    for name, p in ours.named_parameters():
        if name not in want:
            assert p.grad is None, name
        elif name not in cancelled:
            _assert_grad(p.grad.cpu(), want[name].double(), name)


@pytest.mark.parametrize("tag", rc.mlp_tags())
def test_grandplus_mlp(tag):
    from grand_plus_amd.mlp import GrandPlusMLP
    d, m = rc.load("train_pieces.npz"), rc.meta()["mlp"]
    ref, c = rc.mlp_ref(tag)
    ours = GrandPlusMLP(rc.F, rc.C, rc.H, c["nlayers"], c["use_bn"], m["input_droprate"], m["hidden_droprate"], c["node_norm"])
    ours.load_state_dict(rc.state32(rc.sub(d, tag + "__sd__")))
    ours = ours.cuda()
    X, G = rc.t(d["mlp_X"]), rc.t(d["mlp_G"])
    with torch.no_grad():
        ref.eval()(X, None)                                          # for last_a, the scale of the output rule
        _assert_out(ours.eval()(X.float().cuda()).cpu(), rc.t(d[tag + "__eval_out"]), ref.last_a, ref.fcs[-1])
    keeps = rc.mlp_keeps(tag, c["nlayers"])
    with torch.no_grad():
        ref.train()(X, keeps)
    Xo = X.float().cuda().requires_grad_(True)
    out = ours.train()(Xo, keep=[k.cuda() for k in keeps])
    _assert_out(out.detach().cpu(), rc.t(d[tag + "__train_out"]), ref.last_a, ref.fcs[-1])
    out.backward(G.float().cuda())
    # fcs.0.bias under a following BatchNorm is cancelled: 0 up to rounding on both sides (tests/test_gpu_mlp.py)
    cancelled = ("fcs.0.bias",) if c["use_bn"] and not c["node_norm"] and c["nlayers"] > 1 else ()
    _check_param_grads(ours, rc.sub(d, tag + "__grad__"), cancelled)
    if c["node_norm"]:
        assert Xo.grad is None
    else:
        _assert_grad(Xo.grad.cpu(), rc.t(d[tag + "__dX"]), "X")
    for name, b in ours.named_buffers():
        want = rc.t(d[f"{tag}__after__{name}"])
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(want), name
        else:
            torch.testing.assert_close(b.double().cpu(), want, rtol=1e-5, atol=1e-6, msg=name)


@pytest.mark.parametrize("tag", rc.mag_tags())
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_mag_mlp(tag, mode):
    from grand_plus_amd.mlp import MagMLP
    d, c = rc.load("train_mag.npz"), rc.meta()["mag"]["cases"][tag]
    p_in, p_hid = float(d["mag_p"][1]), float(d["mag_p"][2])
    ours = MagMLP(rc.meta()["mag"]["V"], rc.C, rc.H, 2, c["use_bn"], p_in, p_hid, c["node_norm"])
    ours.load_state_dict(rc.state32(rc.sub(d, tag + "__sd__")))
    ours = ours.cuda().train(mode == "train")
    chain = rc.mag_chain64(tag, mode)                                # the restatement, for last_a
    prop = rc.t(d[f"{tag}__{mode}_prop"]).float().cuda().requires_grad_(True)
    k_hid = rc.mag_keeps(tag, mode)[1]
    out = ours(prop, keep=None if k_hid is None else [k_hid.cuda()])
    _assert_out(out.detach().cpu(), rc.t(d[f"{tag}__{mode}_out"]), chain["ref"].last_a, chain["ref"].fcs[-1])
    out.backward(rc.t(d["mag_G"]).float().cuda())
    want = {k: v for k, v in rc.sub(d, f"{tag}__{mode}_grad__").items() if k != "embeds.weight"}
    _check_param_grads(ours, want)
    _assert_grad(prop.grad.cpu(), rc.t(d[f"{tag}__{mode}_dprop"]), "the propagated embedding")
    if mode == "train":
        for name, b in ours.named_buffers():
            if not name.endswith("num_batches_tracked"):
                torch.testing.assert_close(b.double().cpu(), rc.t(d[f"{tag}__after__{name}"]), rtol=1e-5, atol=1e-6, msg=name)


# ------------------------------------------------------------------------------------------------------------------- loss
def test_consis_loss():
    from grand_plus_amd.objective import consis_loss
    d = rc.load("train_pieces.npz")
    for tag, c in sorted(rc.meta()["consis_loss"]["cases"].items()):
        if tag.endswith("_tie"):                                     # float32 cannot hold a row exactly on conf: the host's case
            continue
        lp = rc.t(d[f"cl_S{c['S']}_logp"]).float().cuda().requires_grad_(True)
        con = consis_loss(lp, c["tem"], c["conf"], loss=c["kind"])
        con.backward()
        e, b = jc.value_error(float(con), float(d[tag + "__loss"]))
        g_err, g_ratio = jc.grad_error(lp.grad, rc.t(d[tag + "__grad"]))
        print(f"[reference] {tag}: |d| {e:.3e} / {b:.3e}; grad max |d| {g_err:.3e}, {g_ratio:.3g} of its bound")
        assert e <= b and g_ratio <= 1.0, tag


@pytest.mark.parametrize("name", rc.RUNS)
def test_grand_plus_loss_on_the_recorded_steps(name):
    """The loss of each recorded step from the float64 logits of the replayed restatement (held to the run on the host)."""
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.step import step_weight
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    for i, st in enumerate(rc.replay64(name)):
        _src, _nbr, _sc, y, n_l, _k = rc.step_inputs(name, i)
        w = float(step_weight(a["lam"], a["warmup"], i + 1))
        loss, parts = grand_plus_loss(torch.stack(st["z"]).float().cuda(), y.cuda(), n_l, w, tem=a["tem"], conf=2.0 / rc.C, kind=a["loss"])
        for got, want, what in ((loss, d[f"r64_s{i}_loss"], "loss"), (parts["sup"], d[f"r64_s{i}_sup"].mean(), "sup"),
                                (parts["con"], d[f"r64_s{i}_con"], "con")):
            e, b = jc.value_error(float(got), float(want))
            print(f"[reference] {name} step {i} {what}: |d| {e:.3e} / {b:.3e}")
            assert e <= b, (name, i, what)


# -------------------------------------------------------------------------------------------------------------------- MAG
@pytest.mark.parametrize("tag", rc.mag_tags())
@pytest.mark.parametrize("mode", ["eval", "train"])
def test_embedding_bag(tag, mode):
    from grand_plus_amd.embedding import embedding_bag
    d, bag = rc.load("train_mag.npz"), rc.mag_bag_case(tag, mode == "train")
    _out, terms, _dW, dW_terms = rc.mag_bag_reference(tag, mode)
    W = bag.W.float().cuda().requires_grad_(True)
    out = embedding_bag(W, bag.attr_idx.cuda(), bag.node_idx.cuda(), bag.attr_data.float().cuda(), bag.p, mode == "train",
                        keep=bag.keep.reshape(-1).cuda() if mode == "train" else None)
    ac.close(out.detach(), rc.t(d[f"{tag}__{mode}_emb"]), terms)
    out.backward(rc.t(d[f"{tag}__{mode}_demb"]).float().cuda())
    ac.close(W.grad, rc.t(d[f"{tag}__{mode}_grad__embeds.weight"]), dW_terms)
    assert not out[torch.from_numpy(d["mag_nbr"] == 14).cuda()].any()          # the empty bag


@pytest.mark.parametrize("tag", rc.mag_tags())
@pytest.mark.parametrize("mode", ["eval", "train0"])
def test_mag_prop_rows(tag, mode):
    """emb and random_prop as one launch.  The kernel draws its input mask from the seed, so training is held at
    input_droprate = 0 (the fixture's train0), under the recorded DropNode mask."""
    from grand_plus_amd.mag import mag_prop_rows
    d = rc.load("train_mag.npz")
    col, val, filled, slot = rc.rp_rows(d, "mag_")
    k_node = rc.mag_keeps(tag, mode)[0]
    keep = None if k_node is None else rc.slot_keep(torch.from_numpy(slot), [k_node], rc.B * rc.K).cuda()
    W = rc.t(d[tag + "__sd__embeds.weight"]).float().cuda().requires_grad_(True)
    out = mag_prop_rows(W, rc.t(d["mag_bag_indptr"]).long().cuda(), rc.t(d["mag_bag_attrs"]).int().cuda(),
                        rc.t(d["mag_bag_data"]).float().cuda(), col.cuda(), val.cuda(), filled.cuda(), rc.K, None, samples=1,
                        dropnode_rate=float(d["mag_p"][0]), input_droprate=0.0, training=mode != "eval", keep=keep, validate=True)
    terms, dW_terms = rc.mag_prop_terms(tag, mode)
    share = gc.close(out.detach(), rc.t(d[f"{tag}__{mode}_prop"]), terms, gc.ROUNDINGS, f"{tag} {mode}")
    out.backward(rc.t(d[f"{tag}__{mode}_dprop"]).float().cuda())
    gshare = gc.close(W.grad, rc.t(d[f"{tag}__{mode}_grad__embeds.weight"]), dW_terms, gc.ROUNDINGS, f"{tag} {mode} dW")
    print(f"[reference] mag_prop_rows {tag} {mode}: {share:.3g} of the bound, dW {gshare:.3g}")


# ------------------------------------------------------------------------------------------------------------- evaluation
def _row_matrix(name):
    from grand_plus_amd.rows import RowMatrix
    d = rc.load(f"train_run_{name}.npz")
    seeds, col, val, filled, where = rc.resident_rows(name)
    row = torch.from_numpy(np.repeat(seeds, rc.K).astype(np.int32))
    return RowMatrix(seeds, rc.K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), len(d["labels"])), (col, val, filled, where)


def _model(name, state):
    from grand_plus_amd.mlp import GrandPlusMLP
    a = rc.meta()[f"run_{name}"]
    m = GrandPlusMLP(rc.F, rc.C, a["hidden"], a["nlayers"], a["use_bn"], a["input_droprate"], a["hidden_droprate"], a["node_norm"])
    m.load_state_dict(rc.state32({k[len("mlp."):]: v for k, v in state.items()}))
    return m.cuda()


@pytest.mark.parametrize("name", rc.RUNS)
def test_valid_against_the_recorded_validations(name):
    from grand_plus_amd import valid
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    rm, (col, val, filled, where) = _row_matrix(name)
    X, y = rc.t(d["features"]), rc.t(d["labels"]).long()
    idx = rc.t(d["idx_val"]).long()
    pos = torch.tensor([where[int(i)] for i in idx])
    for nb, want_loss, want_acc in d["r64_valid"][:2]:
        state = rc.sub(d, f"r64_s{int(nb)}_state__")
        model = _model(name, state)
        loss, acc, counts = valid(model, rm, X.float().cuda(), idx, y.cuda(), batch_size=a["batch_size"],
                                  dropnode_rate=a["dropnode_rate"], return_counts=True)
        r64 = ec.valid64(rc.run_model64(name, state).eval(), X, col, val, filled, rc.K, pos, y[idx])
        print(f"[reference] valid {name} at {int(nb)}: |loss - recorded| {abs(float(loss) - want_loss):.3e}, bound {r64['loss_bound']:.3e}")
        assert abs(float(loss) - want_loss) <= r64["loss_bound"]
        undecided = int((~r64["decided"]).sum())
        n_correct = round(want_acc * idx.numel())
        assert counts.tolist()[0] == idx.numel() and counts.tolist()[2:] == [0, 0]
        assert abs(int(counts[1]) - n_correct) <= undecided, (name, nb)
        if not undecided:                                            # predictions and counts exact
            assert float(acc) == float(np.float32(n_correct / idx.numel()))


@pytest.mark.parametrize("name", rc.RUNS)
def test_predict_against_the_recorded_test_accuracy(name):
    from grand_plus_amd import Graph, predict
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    assert (d["adj_data"] == 1.0).all()                              # adj + I without weights
    g = Graph(d["adj_indptr"], d["adj_indices"], 0)
    X, y, idx = rc.t(d["features"]), rc.t(d["labels"]).long(), rc.t(d["idx_test"]).long()
    prop = g.propagate_features(X.float().cuda(), a["prop_mode"], a["order"], a["alpha"]).cpu().numpy().astype(np.float64)
    share = pc.share(prop, d["propagated"])
    print(f"[reference] propagate_features {name}: {share:.3g} of the tolerance")
    assert share <= 1.0
    state = rc.sub(d, "r64_final__")
    acc, preds = predict(g, X.float().cuda(), _model(name, state), idx, y.cuda(), a["prop_mode"], a["order"], alpha=a["alpha"],
                         return_preds=True)
    r64 = ec.predict64(rc.run_model64(name, state).eval(), rc.adjacency(name), X, a["prop_mode"], a["order"], a["alpha"], idx, y[idx])
    ec.assert_decided_preds(preds, r64, f"predict {name}")
    if bool(r64["decided"].all()):
        assert float(acc) == float(np.float32(float(d["r64_test_acc"])))


# ---------------------------------------------------------------------------------------------------- the four-step replay
@pytest.mark.parametrize("name", rc.RUNS)
def test_four_steps_of_the_public_pieces_follow_the_recorded_run(name):
    """random_prop_rows -> GrandPlusMLP -> grand_plus_loss -> backward -> ClipAdam.step with the recorded selections and
    masks.  Parameters and moments after each step by optim_cases.rule over the recorded (t32, r64) pair; the loss and the
    gradient norm by four times |t32 - r64| with a floor of one float32 ulp (rc.run_bound)."""
    from grand_plus_amd import ClipAdam
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.objective import grand_plus_loss
    from grand_plus_amd.step import step_weight
    d, a = rc.load(f"train_run_{name}.npz"), rc.meta()[f"run_{name}"]
    S = a["sample"]
    rm, _host = _row_matrix(name)
    n_slots = rm.col.numel()
    model = _model(name, rc.sub(d, "t32_init__")).train()
    names = sorted(rc.sub(d, "r64_s0_pre__"))                        # the trained parameters, with the reference's prefix
    params = [dict(model.named_parameters())[k[len("mlp."):]] for k in names]
    opt = ClipAdam(params, lr=a["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=a["weight_decay"], clip_norm=a["clip_norm"])
    X, y_all = rc.t(d["features"]).float().cuda(), rc.t(d["labels"]).long()
    for i in range(a["steps_recorded"]):
        batch_rows, slots = rc.batch_slots(name, i)
        _src, _nbr, _sc, y, n_l, keeps = rc.step_inputs(name, i)
        B = batch_rows.numel()
        k_node = rc.slot_keep(slots, [k[0] for k in keeps], n_slots).cuda()
        k_in = torch.stack([k[1] for k in keeps]).cuda()
        k_hid = torch.stack([k[2] for k in keeps]).cuda()
        assert tuple(k_in.shape) == (S, B, rc.F) and tuple(k_hid.shape) == (S, B, a["hidden"])
        opt.zero_grad(set_to_none=True)
        aug = random_prop_rows(X, rm.col, rm.val, rm.filled, rm.K, batch_rows=batch_rows.cuda(), dropnode_rate=a["dropnode_rate"],
                               training=True, keep=k_node, samples=S)
        w = float(step_weight(a["lam"], a["warmup"], i + 1))
        loss, _parts = grand_plus_loss(model(aug, keep=[k_in, k_hid]), y.cuda(), n_l, w, tem=a["tem"], conf=2.0 / rc.C, kind=a["loss"])
        loss.backward()
        norm = opt.step()
        for got, key in ((loss, f"s{i}_loss"), (norm, f"s{i}_grad_norm")):
            r, e32, bound = rc.run_bound(d, key)
            err = abs(float(got) - r)
            print(f"[reference] {name} {key}: ours {err:.3e} torch32 {e32:.3e} bound {bound:.3e} share {err / bound:.3g}")
            assert err <= bound, (name, key, err, bound)
        ours = {"param": [p.detach() for p in params], "exp_avg": [opt.state[p]["exp_avg"] for p in params],
                "exp_avg_sq": [opt.state[p]["exp_avg_sq"] for p in params]}
        t32, r64 = ({"param": [rc.t(d[f"{kind}_s{i}_state__{k}"]) for k in names], "exp_avg": [rc.t(d[f"{kind}_s{i}_m__{k}"]) for k in names],
                     "exp_avg_sq": [rc.t(d[f"{kind}_s{i}_v__{k}"]) for k in names]} for kind in ("t32", "r64"))
        oc.error_ratios(ours, t32, r64, label=f"[reference] {name} step {i}")
        for bname, b in model.named_buffers():
            if a["use_bn"] and not bname.endswith("num_batches_tracked"):
                torch.testing.assert_close(b.double().cpu(), rc.t(d[f"r64_s{i}_state__mlp.{bname}"]), rtol=1e-5, atol=1e-6, msg=bname)


# --------------------------------------------------------------------------------------------------------- early stopping
@pytest.mark.parametrize("mode", ["both", "acc"])
def test_fit_track_update_follows_the_recorded_loop(mode):
    from grand_plus_amd import BestTracker, StepState
    from grand_plus_amd.fit import early_stop_rule, new_track
    d = rc.load("train_stop.npz")
    tr = BestTracker(torch.nn.Linear(3, 2).cuda(), "cuda", mode, int(d["patience"]))
    st, track, saved = StepState("cuda", 1, 0.0, 1.0), new_track(), []
    for i, (loss, acc) in enumerate(d["script"]):
        st.advance()
        v = torch.tensor([loss, acc], dtype=torch.float32, device="cuda")
        tr.update(v[0], v[1], st)
        image = tr.read()
        track = early_stop_rule(track, loss, acc, i + 1, mode, int(d["patience"]))
        assert fc.bits(image) == fc.bits(track), (mode, i)           # field for field
        saved.append(bool(image.copy_now))
        if image.stopped:
            break
    assert saved == d[f"{mode}_saved"].tolist() and image.stopped and image.stop_tick - 1 == int(d[f"{mode}_stop_at"])
