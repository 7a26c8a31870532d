"""The training-side fixtures of the real reference (tests/golden/train_*.npz, written by tests/golden/make_training_golden.py;
DESIGN §7zb) and what both their test files do with them: tests/test_host_reference_training.py holds the float64
restatements to them, tests/test_gpu_reference_training.py the kernels.  Nothing here reads the reference tree."""
import functools
import json
import os

import numpy as np
import scipy.sparse as sp
import torch

import augment_cases as ac
from oracle.mlp_ref import RefMagMLP, RefMLP
from oracle.objective_ref import grand_loss_ref
from oracle.random_prop_ref import random_prop_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("train_pieces.npz", "train_mag.npz", "train_run_plain.npz", "train_run_bn.npz", "train_stop.npz")
B, F, H, C, K = 70, 33, 17, 5, 8
RUNS = ("plain", "bn")


@functools.lru_cache(maxsize=None)
def load(name):
    """A fixture as {key: array}, read once (allow_pickle=False); callers must not modify the arrays."""
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as d:
        return {k: d[k] for k in d.files}


@functools.lru_cache(maxsize=None)
def meta():
    with open(os.path.join(GOLDEN, "training_meta.json")) as f:
        return json.load(f)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def sub(d, prefix):
    """{rest of the key: tensor} of the keys that start with `prefix`."""
    return {k[len(prefix):]: t(v) for k, v in d.items() if k.startswith(prefix)}


def close64(got, ref, what):
    """The rule of the "manual formulas are the reference" tests: rtol 1e-9, atol 1e-12 max|ref|, NaN where the reference
    has NaN."""
    got, ref = torch.as_tensor(got, dtype=torch.float64), torch.as_tensor(ref, dtype=torch.float64)   # a Python float is a double
    fin = ref[torch.isfinite(ref)]
    top = float(fin.abs().max()) if fin.numel() else 0.0
    torch.testing.assert_close(got, ref, rtol=1e-9, atol=1e-12 * top, equal_nan=True, msg=lambda m: f"{what}: {m}")


# ------------------------------------------------------------------------------------------------------------ random_prop
def rp_case(training, p="rp_", d=None):
    """The random_prop fixture as an augment_cases.Case (COO form): feats = X[nbr]."""
    d = d or load("train_pieces.npz")
    idx, nbr = t(d[p + "idx"]).long(), t(d[p + "nbr"]).long()
    X = t(d[p + "X"])
    return ac.Case(F=X.shape[1], S=1, feats=X[nbr], scores=t(d[p + "scores"]), idx=idx, cols=nbr, n_out=B, keep=t(d[p + "keep"])[None],
                   G=t(d[p + "G"])[None], p=float(d[p + "p"]), X=X)


def rp_rows(d, p="rp_"):
    """The same entries as resident rows: (col int32 [B*K], val float64 [B*K], filled int32 [B], slot of every entry)."""
    idx = d[p + "idx"]
    lens = np.bincount(idx, minlength=B)
    slot = np.arange(idx.size) - np.repeat(np.cumsum(lens) - lens, lens)
    col, val = np.zeros((B, K), np.int32), np.zeros((B, K), np.float64)
    col[idx, slot], val[idx, slot] = d[p + "nbr"], d[p + "scores"]
    return t(col.reshape(-1)), t(val.reshape(-1)), t(lens.astype(np.int32)), idx * K + slot


# -------------------------------------------------------------------------------------------------------------------- MLP
def mlp_tags():
    return sorted(meta()["mlp"]["cases"])


def mlp_ref(tag):
    """(RefMLP in float64 with the fixture's state, the case's flags)."""
    c, m = meta()["mlp"]["cases"][tag], meta()["mlp"]
    ref = RefMLP(F, C, H, c["nlayers"], c["use_bn"], m["input_droprate"], m["hidden_droprate"], c["node_norm"]).double()
    ref.load_state_dict(sub(load("train_pieces.npz"), tag + "__sd__"))
    return ref, c


def mlp_keeps(tag, n):
    d = load("train_pieces.npz")
    return [t(d[f"{tag}__keep{i}"]) for i in range(n)]


# ------------------------------------------------------------------------------------------------------------------- MAG
def mag_tags():
    return sorted(meta()["mag"]["cases"])


def mag_bag_case(tag, training):
    """The bags of the MAG fixture as an augment_cases.Case for emb_ref / bag_manual64."""
    d = load("train_mag.npz")
    W = t(d[tag + "__sd__embeds.weight"])
    node_idx = t(d["mag_node_idx"]).long()
    return ac.Case(H=H, V=W.shape[0], W=W, attr_idx=t(d["mag_attr_idx"]).long(), node_idx=node_idx, attr_data=t(d["mag_attr_data"]),
                   keep=t(d[tag + "__keep_in"]), p=float(d["mag_p"][1]), n_out=int(node_idx[-1]) + 1)


MAG_MODES = ("eval", "train", "train0")                # train0: training with input_droprate = 0, DropNode and hidden dropout alone


def mag_keeps(tag, mode):
    """(DropNode mask over the entries, hidden mask) of a mode; (None, None) in eval mode."""
    d = load("train_mag.npz")
    if mode == "eval":
        return None, None
    pre = "__keep_" if mode == "train" else "__keep0_"
    return t(d[tag + pre + "node"]), t(d[tag + pre + "hid"])


def mag_chain64(tag, mode, magnitudes=False):
    """emb -> random_prop -> MLP of model_mag.py through the restatements, in float64 with the recorded masks and upstream
    gradient: {"emb", "prop", "out", "demb", "dprop", "grads" by parameter name, "after" (running statistics)}.
    magnitudes: the table, the bag weights and the scores replaced by their magnitudes (the `terms` of the bounds; the
    MLP's part then means nothing)."""
    d, c = load("train_mag.npz"), meta()["mag"]["cases"][tag]
    p_node, p_in, p_hid = (float(x) for x in d["mag_p"])
    training, drop_in = mode != "eval", mode == "train"
    ref = RefMagMLP(meta()["mag"]["V"], C, H, 2, c["use_bn"], p_in, p_hid, c["node_norm"]).double()
    ref.load_state_dict(sub(d, tag + "__sd__"))
    ref.train(training)
    bag = mag_bag_case(tag, training)
    W = ref.embeds.weight
    if magnitudes:
        W = W.detach().abs().requires_grad_(True)
    k_node, k_hid = mag_keeps(tag, mode)
    data, scores = bag.attr_data, t(d["mag_scores"])
    if magnitudes:
        data, scores = data.abs(), scores.abs()
    emb = ac.emb_ref(W, bag.attr_idx, bag.node_idx, data, p_in, drop_in, bag.keep)
    emb.retain_grad()
    prop = random_prop_ref(emb, scores, t(d["mag_idx"]).long(), p_node, training, k_node)
    prop.retain_grad()
    out = ref(prop, [k_hid])
    (out * t(d["mag_G"])).sum().backward()
    return {"emb": emb.detach(), "prop": prop.detach(), "out": out.detach(), "demb": emb.grad, "dprop": prop.grad, "W": W,
            "grads": {k: p.grad for k, p in ref.named_parameters() if p.grad is not None},
            "after": {k: v for k, v in ref.state_dict().items() if "running" in k}, "ref": ref}


def mag_problem(tag, mode):
    """The MAG fixture in mag_cases' own terms, for its chain64 / manual64 / ref64: (Problem over the fixture's bags and
    resident rows, the DropNode mask on the slots [1, B * K] or None, training).  mode: "eval" or "train0" (input rate 0,
    so mag_cases' hashed input mask is never drawn)."""
    import mag_cases as gc
    d = load("train_mag.npz")
    col, val, filled, slot = rp_rows(d, "mag_")
    indptr = t(d["mag_bag_indptr"]).long()
    P = gc.Problem(W=t(d[tag + "__sd__embeds.weight"]), indptr=indptr, indices=t(d["mag_bag_attrs"]).int(), data=t(d["mag_bag_data"]),
                   col=col.reshape(B, K), val=val.reshape(B, K), filled=filled, K=K, N=indptr.numel() - 1, V=meta()["mag"]["V"], H=H,
                   S_rows=B, longest=int((indptr[1:] - indptr[:-1]).max()))
    k_node = mag_keeps(tag, mode)[0]
    return P, None if k_node is None else slot_keep(torch.from_numpy(slot), [k_node], B * K), mode != "eval"


def mag_bag_reference(tag, mode):
    """augment_cases.bag_reference of the fixture's bags under the recorded upstream gradient of emb: (out, terms, dW,
    dW terms).  train0 and eval draw no input mask."""
    d, bag = load("train_mag.npz"), mag_bag_case(tag, mode == "train")
    c = ac.Case(**{**bag.__dict__, "W": bag.W.float(), "G": t(d[f"{tag}__{mode}_demb"])})
    return ac.bag_reference(c, mode == "train")


def mag_prop_terms(tag, mode):
    """(terms of the propagated embedding, terms of the table's gradient under the recorded upstream gradient of it): the
    chain on magnitudes."""
    d = load("train_mag.npz")
    return mag_chain64(tag, mode, magnitudes=True)["prop"], _table_terms(tag, mode, t(d[f"{tag}__{mode}_dprop"]).abs())


def _table_terms(tag, mode, G):
    d = load("train_mag.npz")
    p_node, p_in, _ = (float(x) for x in d["mag_p"])
    bag = mag_bag_case(tag, mode == "train")
    W = bag.W.abs().clone().requires_grad_(True)
    emb = ac.emb_ref(W, bag.attr_idx, bag.node_idx, bag.attr_data.abs(), p_in, mode == "train", bag.keep)
    prop = random_prop_ref(emb, t(d["mag_scores"]).abs(), t(d["mag_idx"]).long(), p_node, mode != "eval", mag_keeps(tag, mode)[0])
    return torch.autograd.grad((prop * G).sum(), W)[0]


# -------------------------------------------------------------------------------------------------------------- the runs
def run_model64(name, state):
    """RefMLP in float64 of a run's configuration holding `state` (a state_dict with the reference's `mlp.` prefix)."""
    a = meta()[f"run_{name}"]
    ref = RefMLP(F, C, a["hidden"], a["nlayers"], a["use_bn"], a["input_droprate"], a["hidden_droprate"], a["node_norm"]).double()
    ref.load_state_dict({k[len("mlp."):]: v.double() for k, v in state.items()})
    return ref


def step_inputs(name, i):
    """What step i (0-based) of a run consumed: (source_idx, neighbor_idx, scores float64, labels of the batch, n_l, the
    masks as [(DropNode, input, hidden)] per sample)."""
    d, a = load(f"train_run_{name}.npz"), meta()[f"run_{name}"]
    keeps = [t(d[f"s{i}_keep{j}"]) for j in range(3 * a["sample"])]
    train = d[f"s{i}_train_index"]
    return (t(d[f"s{i}_source_idx"]).long(), t(d[f"s{i}_neighbor_idx"]).long(), t(d[f"s{i}_mat_scores"]), t(d["labels"][train]).long(),
            len(train), [keeps[3 * s:3 * s + 3] for s in range(a["sample"])])


def replay64(name, mut=None):
    """The first recorded steps through the restatements in float64: random_prop_ref -> RefMLP -> grand_loss_ref ->
    backward -> torch's clip_grad_norm_ and Adam (what optim_cases takes as the optimiser's reference), with the recorded
    selections and masks and the weight of step_weight.  Returns per step {"loss", "grad_norm", "pre", "state", "m", "v", "z"}.
    mut: "ramp_from_t" takes the weight of the next step, "sup_not_divided" does not divide the supervised sum by S."""
    from grand_plus_amd.step import step_weight
    import objective_cases as jc
    d, a = load(f"train_run_{name}.npz"), meta()[f"run_{name}"]
    ref = run_model64(name, sub(d, "r64_init__")).train()
    params = list(ref.parameters())
    opt = torch.optim.Adam(params, lr=a["lr"], weight_decay=a["weight_decay"], foreach=False)
    X = t(d["features"])
    out = []
    for i in range(a["steps_recorded"]):
        tick = int(d[f"s{i}_num_batch"]) + 1
        src, nbr, scores, y, n_l, keeps = step_inputs(name, i)
        w = float(step_weight(a["lam"], a["warmup"], tick + 1 if mut == "ramp_from_t" else tick))
        opt.zero_grad(set_to_none=True)
        z = []
        for k_node, k_in, k_hid in keeps:
            aug = random_prop_ref(X[nbr], scores, src, a["dropnode_rate"], True, k_node).detach()
            z.append(ref(aug, [k_in, k_hid]))
        if mut == "sup_not_divided":
            loss = jc.manual_terms(z, y, n_l, w, a["tem"], 2.0 / C, a["loss"], mut="sup_summed_over_samples")[0]
        else:
            loss = grand_loss_ref(z, y, n_l, w, a["tem"], 2.0 / C, a["loss"])[0]
        loss.backward()
        with_grad = [p for p in params if p.grad is not None]
        pre = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
        norm = torch.nn.utils.clip_grad_norm_(with_grad, a["clip_norm"], foreach=False)
        opt.step()
        out.append({"loss": loss.detach(), "grad_norm": norm.detach(), "pre": pre, "z": [x.detach() for x in z],
                    "state": {k: v.detach().clone() for k, v in ref.state_dict().items()},
                    "m": {k: opt.state[p]["exp_avg"].clone() for k, p in ref.named_parameters() if p in opt.state},
                    "v": {k: opt.state[p]["exp_avg_sq"].clone() for k, p in ref.named_parameters() if p in opt.state}})
    return out


def resident_rows(name):
    """The run's top-k matrix as resident rows over its seed list: (seeds int64, col int32 [S*K], val float64 [S*K], filled
    int32 [S], {node id: position})."""
    d = load(f"train_run_{name}.npz")
    seeds = np.concatenate([d["idx_train"], d["idx_val"], d["idx_sample"]]).astype(np.int64)
    topk = sp.coo_matrix((d["topk_val"], (d["topk_row"], d["topk_col"])), (len(d["labels"]),) * 2).tocsr()
    col, val, filled = np.zeros((len(seeds), K), np.int32), np.zeros((len(seeds), K), np.float64), np.zeros(len(seeds), np.int32)
    for i, s in enumerate(seeds):
        lo, hi = topk.indptr[s], topk.indptr[s + 1]
        filled[i] = hi - lo
        col[i, :hi - lo], val[i, :hi - lo] = topk.indices[lo:hi], topk.data[lo:hi]
    return seeds, t(col.reshape(-1)), t(val.reshape(-1)), t(filled), {int(s): i for i, s in enumerate(seeds)}


def adjacency(name):
    d = load(f"train_run_{name}.npz")
    n = len(d["labels"])
    return sp.csr_matrix((d["adj_data"], d["adj_indices"], d["adj_indptr"]), shape=(n, n))


def run_bound(d, key):
    """The bound of a per-step scalar of a run that has no rule of its own: four times the reference's own float32 error
    |t32 - r64| with a floor of one float32 ulp of the value (optim_cases.rule's construction).  Returns (r64, t32 error, bound)."""
    r, e = float(d["r64_" + key]), abs(float(d["t32_" + key]) - float(d["r64_" + key]))
    return r, e, 4.0 * e + 2.0 ** -23 * abs(r)


# ---------------------------------------------------------------------------------------------------- the early-stop rule
def drive_rule(mode, tie_is_bad=False):
    """fit.early_stop_rule over the scripted pairs, one evaluation per tick: (saved per evaluation, the tick it stopped at or
    None).  tie_is_bad: the misreading in which an accuracy tie with a higher loss counts towards patience."""
    from grand_plus_amd.fit import early_stop_rule, new_track
    d = load("train_stop.npz")
    track, saved = new_track(), []
    for i, (loss, acc) in enumerate(d["script"]):
        before = (track["best_loss"], track["bad_counter"])
        track = early_stop_rule(track, loss, acc, i + 1, mode, int(d["patience"]))
        if tie_is_bad and not track["copy_now"] and np.float32(acc) >= track["best_acc"] and track["bad_counter"] == before[1]:
            track["bad_counter"] += 1
            if track["bad_counter"] >= int(d["patience"]):
                track.update(stopped=1, stop_tick=i + 1)
        saved.append(bool(track["copy_now"]))
        if track["stopped"]:
            return saved, track["stop_tick"]
    return saved, None


# ------------------------------------------------------------------------------------------------------------ on the GPU
def state32(state):
    """A recorded state_dict for a float32 module: floating tensors as float32."""
    return {k: (v.float() if v.is_floating_point() else v) for k, v in state.items()}


def slot_keep(entry_slots, keeps, n_slots):
    """S masks over entries [S][M] laid out on the resident slots: uint8 [S, n_slots]."""
    out = torch.zeros((len(keeps), n_slots), dtype=torch.uint8)
    for s, k in enumerate(keeps):
        out[s, entry_slots] = k.reshape(-1)
    return out


def batch_slots(name, i):
    """Step i's batch on the resident rows: (batch_rows int32 [B], the slot of every recorded entry).  The entries were
    recorded in scipy's nonzero order, row after row with ascending columns, which is the slot order of resident_rows."""
    d = load(f"train_run_{name}.npz")
    _seeds, col, _val, filled, where = resident_rows(name)
    nodes = np.concatenate([d[f"s{i}_train_index"], d[f"s{i}_unlabel_index"]])
    rows = np.array([where[int(n)] for n in nodes])
    src = d[f"s{i}_source_idx"]
    lens = np.bincount(src, minlength=len(rows))
    assert np.array_equal(lens, filled.numpy()[rows])
    slots = rows[src] * K + (np.arange(src.size) - np.repeat(np.cumsum(lens) - lens, lens))
    assert np.array_equal(col.numpy()[slots], d[f"s{i}_neighbor_idx"])
    return t(rows.astype(np.int32)), torch.from_numpy(slots)
