"""Generate the training-side fixtures tests/golden/train_*.npz and training_meta.json from the REAL reference.

Run in the build container only (needs /root/reference and oracle/_ref, built by `make -C oracle`):
    python tests/golden/make_training_golden.py

What it does
  * imports the reference's own model.py and model_mag.py and CALLS them; nothing of their text is here.  Four stand-ins
    make the import and a CPU run possible:
      - `torch_scatter` (requirements.txt:7, not installed): a module object whose scatter(src, index, dim, dim_size,
        reduce) is index_add_ for dim = 0, reduce = 'sum', the only form model.py:83-86 and model_mag.py:52-53 use;
      - `precompute.propagation` (model.py:9): oracle/_ref, the reference's propagation.cpp compiled as it stands;
      - while the recorder runs, torch.cuda.set_device is a no-op (model.py:230 calls it before looking at args.cuda) and
        Tensor.cuda / Module.cuda return self (model_mag.py:33-34,49 call them in constructors and in emb);
      - predict (model.py:181) is handed scipy.sparse.csr_matrix(adj): `adj.sum(1).A1` (model.py:189) needs a matrix.
  * replaces the name `F` in the imported modules by a proxy of torch.nn.functional whose dropout draws its keep mask from
    a seeded generator and logs it, so that every recorded output is a function of recorded inputs and recorded masks;
  * A. calls the pieces in float64 at B = 70, F = 33, H = 17, C = 5, up to K = 8 entries per row: Grand_Plus.random_prop,
    MLP (1-3 layers, every use_bn / node_norm pair), consis_loss, and model_mag's emb, random_prop and forward;
  * B. runs main() (model.py:227-373) on a 300-node graph of this repo's generator, handed over by a stand-in for
    load_data, in two configurations, each as the reference is (float32, `t32`) and in float64 (`r64`), and records the
    first steps, every validation, every save and the end through hooks on optimizer.step, valid and torch.save;
  * C. runs main() with `valid` replaced by a script of (loss, acc) pairs, in both stop modes.
Only data is written: inputs, masks and the reference's outputs.  Every file is written with fixed zip time stamps, so a
second run gives the same bytes.
"""
import argparse
import contextlib
import copy
import io
import json
import os
import sys
import types
import zipfile

import numpy as np
import scipy.sparse as sp
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from grand_plus_amd import synth                       # noqa: E402
from oracle import pyoracle                            # noqa: E402

B, F, H, C, K = 70, 33, 17, 5, 8                       # one past a tile, wave or vector edge of the kernels
RECORDED_STEPS = 4
_REF_MODULES = ("torch_scatter", "precompute", "model", "model_mag", "utils")


def available():
    return os.path.exists(os.path.join(REF, "model.py")) and pyoracle.load_reference_module() is not None


# ------------------------------------------------------------------------------------------------------------- stand-ins
def scatter(src, index, dim=0, dim_size=None, reduce="sum"):
    """torch_scatter.scatter for dim = 0, reduce = 'sum': out[index[i]] += src[i].  `index` is [M, 1], broadcast over src."""
    assert dim == 0 and reduce == "sum" and index.dim() == 2 and index.shape[1] == 1
    out = torch.zeros((int(dim_size),) + tuple(src.shape[1:]), dtype=src.dtype)
    return out.index_add_(0, index[:, 0], src)


class Functional:
    """torch.nn.functional with a dropout that draws from its own generator and logs the mask (uint8)."""

    def __init__(self, seed):
        self.gen, self.log, self.force, self.nll = torch.Generator().manual_seed(seed), [], [], []

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)

    def nll_loss(self, *a, **k):                                       # logged: the supervised terms of a step
        self.nll.append(torch.nn.functional.nll_loss(*a, **k))
        return self.nll[-1]

    def dropout(self, x, p=0.5, training=True, inplace=False):
        if not training or p == 0:
            return x
        keep = torch.rand(x.shape, generator=self.gen) >= p            # float32 draws, whatever the dtype of x
        if self.force:                                                 # a case that needs certain entries dropped
            keep = self.force.pop(0)(keep)
        self.log.append(keep.to(torch.uint8))
        return x * keep.to(x.dtype) / (1 - p)


@contextlib.contextmanager
def reference():
    """(model, model_mag) of the reference, imported over the stand-ins; sys.modules, sys.path and torch are put back."""
    ref = pyoracle.load_reference_module()
    assert ref is not None, "oracle/_ref is not built (make -C oracle)"
    mine = lambda k: k.split(".")[0] in _REF_MODULES  # noqa: E731
    saved = {k: v for k, v in sys.modules.items() if mine(k)}
    path = list(sys.path)
    patched = (torch.Tensor.cuda, torch.nn.Module.cuda, torch.cuda.set_device)
    try:
        for k in saved:
            del sys.modules[k]
        ts, pre = types.ModuleType("torch_scatter"), types.ModuleType("precompute")
        ts.scatter, pre.propagation = scatter, ref
        sys.modules.update({"torch_scatter": ts, "precompute": pre, "precompute.propagation": ref})
        sys.path.insert(0, REF)
        torch.Tensor.cuda = lambda self, *a, **k: self
        torch.nn.Module.cuda = lambda self, *a, **k: self
        torch.cuda.set_device = lambda *a, **k: None
        import model
        import model_mag
        yield model, model_mag
    finally:
        torch.Tensor.cuda, torch.nn.Module.cuda, torch.cuda.set_device = patched
        for k in [k for k in sys.modules if mine(k)]:
            del sys.modules[k]
        sys.modules.update(saved)
        sys.path[:] = path


def np64(t):
    return t.detach().double().numpy().copy()


# ---------------------------------------------------------------------------------------------------------- A. the pieces
def coo_rows(rng, n_src, tiny_row=20):
    """B rows of up to K entries: (idx [M], nbr [M], scores float64 [M]).  Row 35 has no entry, row 10 is the one a forced
    mask drops whole, the last row has entries (so dim_size, model.py:84, is B), the scores span twelve binades and row
    `tiny_row` sums to about 1e-11, where the 1e-12 of model.py:87 is a tenth of the denominator."""
    lens = rng.integers(1, K + 1, B)
    lens[35], lens[10], lens[B - 1], lens[0] = 0, 3, K, K
    idx = np.repeat(np.arange(B), lens)
    nbr = rng.integers(0, n_src, idx.size)
    scores = np.exp2(-12 * rng.random(idx.size)).astype(np.float32).astype(np.float64)
    scores[idx == tiny_row] *= np.float64(np.float32(1e-11))
    return idx, nbr, scores.astype(np.float32).astype(np.float64)


def drop_row(idx, row):
    where = torch.from_numpy(idx == row)
    return lambda keep: keep & ~where


def piece_random_prop(model, out, meta):
    rng = np.random.default_rng(101)
    n_src = 50
    idx, nbr, scores = coo_rows(rng, n_src)
    X = rng.standard_normal((n_src, F)).astype(np.float32).astype(np.float64)
    G = rng.standard_normal((B, F)).astype(np.float32).astype(np.float64)
    out.update(rp_idx=idx, rp_nbr=nbr, rp_scores=scores, rp_X=X, rp_G=G, rp_p=np.float64(0.5))
    net = model.Grand_Plus(F, C, H, 2, False, 0.0, 0.0).double()
    fn = model.F = Functional(1)
    for mode in ("train", "eval"):
        net.train(mode == "train")
        x = torch.from_numpy(X).requires_grad_(True)
        if mode == "train":
            fn.force.append(drop_row(idx, 10))
        y = net.random_prop(x[torch.from_numpy(nbr)], torch.from_numpy(scores), torch.from_numpy(idx), 0.5)   # model.py:80-87
        (y * torch.from_numpy(G)).sum().backward()
        out[f"rp_{mode}_out"], out[f"rp_{mode}_dX"] = np64(y), np64(x.grad)
    out["rp_keep"] = fn.log[0].numpy()
    assert len(fn.log) == 1 and y.shape[0] == B and not out["rp_keep"][idx == 10].any()
    meta["random_prop"] = {"B": B, "F": F, "entries": int(idx.size), "n_src": n_src, "p": 0.5, "all_dropped_row": 10,
                           "empty_row": 35, "tiny_row": 20, "lines": "model.py:80-87"}


def piece_mlp(model, out, meta):
    rng = np.random.default_rng(202)
    X = rng.standard_normal((B, F)).astype(np.float32).astype(np.float64) * 1.5 + 0.25
    G = rng.standard_normal((B, C)).astype(np.float32).astype(np.float64)
    out.update(mlp_X=X, mlp_G=G, mlp_p=np.array([0.3, 0.4]))
    cases = {}
    for nl in (1, 2, 3):
        for bn in (False, True):
            for nn_ in (False, True):
                tag = f"mlp_L{nl}_bn{int(bn)}_nn{int(nn_)}"
                torch.manual_seed(1000 + 100 * nl + 10 * bn + nn_)
                net = model.MLP(F, C, H, nl, bn, 0.3, 0.4, nn_)                           # model.py:17-39
                with torch.no_grad():                                                     # BatchNorm away from its defaults
                    for b in net.bns:
                        b.weight.uniform_(0.5, 1.5); b.bias.uniform_(-0.5, 0.5)
                        b.running_mean.uniform_(-0.5, 0.5); b.running_var.uniform_(0.5, 2.0)
                net = net.double()                                                        # float64 that holds float32 values
                for k, v in net.state_dict().items():
                    out[f"{tag}__sd__{k}"] = v.numpy().copy()
                fn = model.F = Functional(nl * 8 + bn * 2 + nn_)
                net.eval()
                out[f"{tag}__eval_out"] = np64(net(torch.from_numpy(X)))                  # model.py:48-67, from the initial state
                net.train()
                x = torch.from_numpy(X).requires_grad_(True)
                y = net(x)
                (y * torch.from_numpy(G)).sum().backward()
                out[f"{tag}__train_out"] = np64(y)
                assert len(fn.log) == nl
                for i, k in enumerate(fn.log):
                    out[f"{tag}__keep{i}"] = k.numpy()
                for k, v in net.state_dict().items():
                    if "running" in k or "num_batches" in k:
                        out[f"{tag}__after__{k}"] = v.numpy().copy()
                for k, p in net.named_parameters():
                    if p.grad is not None:
                        out[f"{tag}__grad__{k}"] = np64(p.grad)
                if x.grad is not None:                                                    # node_norm detaches X (model.py:50)
                    out[f"{tag}__dX"] = np64(x.grad)
                cases[tag] = {"nlayers": nl, "use_bn": bn, "node_norm": nn_}
    meta["mlp"] = {"B": B, "F": F, "H": H, "C": C, "input_droprate": 0.3, "hidden_droprate": 0.4, "cases": cases,
                   "lines": "model.py:17-67"}


def piece_consis(model, out, meta):
    rng = np.random.default_rng(303)
    cases = {}
    for S in (1, 2, 4):
        z = torch.from_numpy(rng.standard_normal((S, B, C)) * 1.2)
        z[:, :, 0] += torch.from_numpy(rng.standard_normal(B)) * 1.5            # rows that agree across samples: some confident
        lp = torch.log_softmax(z, dim=-1).float().double()             # what a float32 caller hands over, widened
        out[f"cl_S{S}_logp"] = np64(lp)
        # our own arithmetic, not the reference's: the largest averaged probability of every row, for the choice of conf
        top = (sum(torch.exp(p) for p in lp) / S).max(1)[0]
        tie_row = int(torch.argsort(top)[B // 2])
        confs = {"some": 0.4, "none": 1.0, "tie": float(top[tie_row])}           # tie: one row sits exactly on conf
        assert 5 < int((top > 0.4).sum()) < B - 5 and float((top - 0.4).abs().min()) > 1e-3
        out[f"cl_S{S}_conf_tie"] = np.float64(confs["tie"])
        for kind in ("kl", "l2"):
            for tem in (0.5, 0.1):
                for cname, conf in confs.items():
                    leaves = [lp[s].clone().requires_grad_(True) for s in range(S)]
                    loss = model.consis_loss(argparse.Namespace(loss=kind), leaves, tem, conf)      # model.py:123-140
                    loss.backward()
                    tag = f"cl_S{S}_{kind}_t{tem}_{cname}"
                    out[f"{tag}__loss"] = np64(loss)
                    out[f"{tag}__grad"] = np.stack([np64(t.grad) for t in leaves])
                    cases[tag] = {"S": S, "kind": kind, "tem": tem, "conf": conf, "passing": int((top > conf).sum()),
                                  "nan": bool(torch.isnan(loss))}
                    assert bool(torch.isnan(loss)) == (cname == "none")
    meta["consis_loss"] = {"B": B, "C": C, "cases": cases, "lines": "model.py:123-140"}


def piece_mag(model_mag, out, meta):
    rng = np.random.default_rng(404)
    V, n_src = 40, 30
    idx, nbr, scores = coo_rows(rng, n_src)
    # the bags of the source nodes: node 3 has one attribute, node 14 none, node 7 the same attribute three times, node 21
    # weights at the scale of the 1e-10 of model_mag.py:54
    lens = rng.integers(2, 7, n_src)
    lens[3], lens[14], lens[7] = 1, 0, 4
    indptr = np.concatenate([[0], np.cumsum(lens)])
    attrs = rng.integers(0, V, indptr[-1])
    attrs[indptr[7]:indptr[7] + 3] = 5
    data = (rng.random(indptr[-1]) + 0.1).astype(np.float32).astype(np.float64)
    data[indptr[21]:indptr[22]] *= np.float64(np.float32(1e-10))
    data = data.astype(np.float32).astype(np.float64)
    nbr[nbr == 14] = 15
    nbr[idx == 30] = 14                                                # the empty bag: every entry of a row in the middle
    nbr[-1], nbr[5] = 2, 21
    # the COO of the batch's bags as main_mag builds it (model_mag.py:345-349): one bag per entry of the batch
    blen = lens[nbr]
    node_idx = np.repeat(np.arange(idx.size), blen)
    attr_idx = np.concatenate([attrs[indptr[n]:indptr[n + 1]] for n in nbr])
    attr_data = np.concatenate([data[indptr[n]:indptr[n + 1]] for n in nbr])
    assert node_idx[-1] == idx.size - 1
    G = rng.standard_normal((B, C)).astype(np.float32).astype(np.float64)
    out.update(mag_idx=idx, mag_nbr=nbr, mag_scores=scores, mag_bag_indptr=indptr, mag_bag_attrs=attrs, mag_bag_data=data,
               mag_node_idx=node_idx, mag_attr_idx=attr_idx, mag_attr_data=attr_data, mag_G=G, mag_p=np.array([0.5, 0.3, 0.4]))
    cases = {}
    for bn, nn_ in ((False, False), (True, True)):
        tag = f"mag_bn{int(bn)}_nn{int(nn_)}"
        torch.manual_seed(77 + bn)
        net = model_mag.Grand_Plus(V, C, H, 2, bn, 0.3, 0.4, 0.5, nn_)                     # model_mag.py:17-39, 70-75
        with torch.no_grad():
            for b in net.mlp.bns:
                b.weight.uniform_(0.5, 1.5); b.bias.uniform_(-0.5, 0.5)
                b.running_mean.uniform_(-0.5, 0.5); b.running_var.uniform_(0.5, 2.0)
        net = net.double()
        initial = copy.deepcopy(net.state_dict())
        for k, v in net.mlp.state_dict().items():
            out[f"{tag}__sd__{k}"] = v.numpy().copy()
        fn = model_mag.F = Functional(50 + bn)
        a_i, n_i, a_d = torch.from_numpy(attr_idx), torch.from_numpy(node_idx), torch.from_numpy(attr_data)
        # train0: training without input dropout (our kernel of the whole front end takes the DropNode mask alone); it starts
        # from the initial state again, so that its BatchNorm sees what `train` saw
        for mode in ("eval", "train", "train0"):
            net.train(mode != "eval")
            net.zero_grad()
            if mode == "train0":
                net.load_state_dict(initial)
                net.mlp.input_droprate = 0.0
            emb = net.emb(a_i, n_i, a_d)                                                   # model_mag.py:48-55, 88-90
            emb.retain_grad()
            prop = net.random_prop(emb, torch.from_numpy(scores), torch.from_numpy(idx), 0.5)      # model_mag.py:80-86
            prop.retain_grad()
            y = net(prop)                                                                  # model_mag.py:57-67
            (y * torch.from_numpy(G)).sum().backward()
            out[f"{tag}__{mode}_emb"], out[f"{tag}__{mode}_prop"], out[f"{tag}__{mode}_out"] = np64(emb), np64(prop), np64(y)
            out[f"{tag}__{mode}_demb"], out[f"{tag}__{mode}_dprop"] = np64(emb.grad), np64(prop.grad)
            if mode == "train":
                for k, v in net.mlp.state_dict().items():
                    if "running" in k or "num_batches" in k:
                        out[f"{tag}__after__{k}"] = v.numpy().copy()
            for k, p in net.mlp.named_parameters():
                if p.grad is not None:
                    out[f"{tag}__{mode}_grad__{k}"] = np64(p.grad)
        assert len(fn.log) == 5                                        # input dropout, DropNode, hidden dropout; train0's two
        for name, k in zip(("keep_in", "keep_node", "keep_hid", "keep0_node", "keep0_hid"), fn.log):
            out[f"{tag}__{name}"] = k.numpy()
        cases[tag] = {"use_bn": bn, "node_norm": nn_}
    meta["mag"] = {"B": B, "H": H, "C": C, "V": V, "n_src": n_src, "entries": int(idx.size), "bag_entries": int(attr_idx.size),
                   "one_attribute_node": 3, "empty_bag_node": 14, "repeated_attribute_node": 7, "tiny_bag_node": 21,
                   "cases": cases, "lines": "model_mag.py:17-90"}


# ------------------------------------------------------------------------------------------------------ B. whole runs
def dataset():
    """What the stand-in for load_data returns (utils/data_loader.py:15): adj, features, one-hot labels, three index arrays."""
    n = 300
    indptr, indices = synth.powerlaw_csr(n, 900, 7, 10)
    adj = sp.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    adj.setdiag(0)                                                     # main() adds the identity itself (model.py:243)
    adj.eliminate_zeros()
    rng = np.random.default_rng(505)
    y = rng.integers(0, C, n)
    centres = rng.standard_normal((C, F))
    features = (1.5 * centres[y] + rng.standard_normal((n, F))).astype(np.float32).astype(np.float64)
    order = rng.permutation(n)
    return sp.csr_matrix(adj), features, np.eye(C, dtype=np.int64)[y], np.sort(order[:50]), np.sort(order[50:110]), np.sort(order[110:260])


CONFIGS = {
    # the Cora script's flags (scripts/run_cora.sh) at the fixtures' sizes; clip_norm and weight_decay > 0
    "plain": dict(use_bn=False, node_norm=False, loss="l2", input_droprate=0.5, hidden_droprate=0.7),
    "bn": dict(use_bn=True, node_norm=True, loss="kl", input_droprate=0.2, hidden_droprate=0.5),
}


def run_args(**kw):
    a = dict(model="grandpp", dataset="synth300", no_cuda=True, cuda_device="cpu", seed1=0, seed2=0, epochs=4, lr=0.01,
             weight_decay=5e-4, stop_mode="both", warmup=8.0, clip_norm=0.5, eval_batch=2, batch_size=20, unlabel_batch_size=40,
             nlayers=2, hidden=H, dropnode_rate=0.5, patience=3, sample=2, tem=0.5, lam=1.0, alpha=0.2, top_k=K, rmax=1e-5,
             order=4, unlabel_num=-1, prop_mode="ppr", visible=False)
    a.update(kw)
    return argparse.Namespace(**a)


class TorchProxy:
    """The name `torch` inside the reference module: save and load stay in memory; with wide=True what main(), valid and
    get_local_logits build as float32 (model.py:151, 175, 315) is rounded to float32 as there and then widened to float64."""

    def __init__(self, rec, wide):
        self._rec, self._wide, self._saved = rec, wide, {}

    def __getattr__(self, name):
        return getattr(torch, name)

    def tensor(self, data, dtype=None, **kw):                         # the float32 rounding is the reference's; then widened
        out = torch.tensor(data, dtype=dtype, **kw)
        return out.double() if (self._wide and dtype == torch.float32) else out

    def FloatTensor(self, data):
        out = torch.tensor(np.asarray(data), dtype=torch.float32)
        return out.double() if self._wide else out

    def save(self, state, name):                                      # model.py:350
        self._saved[name] = copy.deepcopy(state)
        self._rec["saves"].append(sys._getframe(1).f_locals["num_batch"])

    def load(self, name):                                             # model.py:368
        return self._saved[name]


def run_main(mod, args, wide, script=None, data=None):
    """One main(args) of the reference module `mod` with the hooks in place: the record as a dict of lists."""
    rec = {"steps": [], "valid": [], "saves": [], "init": None, "net": None}
    fn = Functional(900)
    own = {k: getattr(mod, k) for k in ("F", "torch", "optim", "load_data", "totensor", "Grand_Plus", "clip_grad_norm", "valid", "predict",
                                        "consis_loss", "get_local_logits")}
    data = data or dataset()
    dt = torch.float64 if wide else torch.float32

    def grand_plus(**kw):
        # built in float32 from the seed main() set (model.py:233), then widened: both runs start from the same weights
        net = own["Grand_Plus"](**kw)
        net = net.double() if wide else net
        rec["net"], rec["init"] = net, {k: v.detach().clone() for k, v in net.state_dict().items()}
        return net

    def consis(*a, **k):                                              # model.py:123-140
        rec["con"] = own["consis_loss"](*a, **k)
        return rec["con"]

    def local_logits(mlp, attr_mat, *a, **k):                         # model.py:169-178; attr_mat: what predict propagated
        rec["prop"] = np.array(attr_mat, dtype=np.float64)
        return own["get_local_logits"](mlp, attr_mat, *a, **k)

    def clip(params, max_norm):                                       # model.py:116-120
        params = list(params)
        rec["pre"] = [None if p.grad is None else p.grad.detach().clone() for p in params]   # without use_bn, bns get none
        return own["clip_grad_norm"](params, max_norm)

    class Optim:
        @staticmethod
        def Adam(params, **kw):                                       # model.py:288
            params = list(params)
            opt = torch.optim.Adam(params, **kw)
            step = opt.step

            def recording_step():                                     # model.py:334
                loc = sys._getframe(1).f_locals
                step()
                if len(rec["steps"]) < RECORDED_STEPS:
                    st = {k: loc[k] for k in ("num_batch", "train_index", "unlabel_index_batch", "source_idx", "neighbor_idx")}
                    st.update(mat_scores=loc["mat_scores"].detach().clone(), loss=loc["loss_train"].detach().clone(),
                              grad_norm=torch.as_tensor(loc["grad_norm"]).detach().clone(), pre=rec["pre"], keeps=list(fn.log),
                              con=rec["con"].detach().clone(), sup=torch.stack(fn.nll[-loc["K"]:]).detach().clone(),
                              state={k: v.detach().clone() for k, v in rec["net"].state_dict().items()},
                              exp_avg=[opt.state[p]["exp_avg"].clone() if p in opt.state else None for p in params],
                              exp_avg_sq=[opt.state[p]["exp_avg_sq"].clone() if p in opt.state else None for p in params])
                    rec["steps"].append(st)
                fn.log.clear()
            opt.step = recording_step
            rec["param_names"] = [k for k, _ in rec["net"].named_parameters()]
            return opt

    def valid(*a, **k):                                               # model.py:143-166, or the script of part C
        loc = sys._getframe(1).f_locals
        nb = loc["num_batch"]
        rec["topk"], rec["idx_sample"] = a[2], loc["idx_sample"]      # the topk_adj and the sample main() built (model.py:244-272)
        loss, acc = script[len(rec["valid"])] if script is not None else own["valid"](*a, **k)
        rec["valid"].append((nb, loss, acc))
        return loss, acc

    mod.F, mod.torch, mod.optim = fn, TorchProxy(rec, wide), Optim
    mod.load_data = lambda dataset_str, split_seed: data + (None,)
    mod.totensor = lambda f, l: (torch.tensor(f, dtype=dt), torch.LongTensor(np.argmax(l, -1)))   # utils/data_loader.py:146-150
    mod.Grand_Plus, mod.clip_grad_norm, mod.valid, mod.consis_loss = grand_plus, clip, valid, consis
    mod.get_local_logits = local_logits

    def predict(a, adj, *rest, **k):                                  # model.py:181; adj: main()'s adj + I (model.py:243)
        rec["adj"] = sp.csr_matrix(adj)
        return own["predict"](a, rec["adj"], *rest, **k)

    mod.predict = predict
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            _t, test_acc, _bt, num_batch = mod.main(args)
    finally:
        for k, v in own.items():
            setattr(mod, k, v)
    rec.update(test_acc=float(test_acc), num_batch=int(num_batch),
               final={k: v.detach().clone() for k, v in rec["net"].state_dict().items()})
    return rec


def whole_run(model, name, meta):
    cfg = CONFIGS[name]
    args, data = run_args(**cfg), dataset()
    adj, features, labels, idx_train, idx_val, idx_test = data
    out = dict(features=features, labels=np.argmax(labels, -1), idx_train=idx_train, idx_val=idx_val, idx_test=idx_test)
    recs = {}
    for kind, wide in (("t32", False), ("r64", True)):
        rec = recs[kind] = run_main(model, run_args(**cfg), wide, data=dataset())
        assert rec["steps"] and all(torch.isfinite(s["loss"]) for s in rec["steps"]), name
        out[f"{kind}_test_acc"], out[f"{kind}_num_batch"] = np.float64(rec["test_acc"]), np.int64(rec["num_batch"])
        out[f"{kind}_valid"] = np.array(rec["valid"], dtype=np.float64)                    # rows of (num_batch, loss, acc)
        out[f"{kind}_saves"] = np.array(rec["saves"], dtype=np.int64)
        for k, v in rec["init"].items():
            out[f"{kind}_init__{k}"] = v.numpy()
        for k, v in rec["final"].items():
            out[f"{kind}_final__{k}"] = v.numpy()
        for t, st in enumerate(rec["steps"]):
            p = f"{kind}_s{t}"
            out[f"{p}_loss"], out[f"{p}_grad_norm"] = st["loss"].numpy(), st["grad_norm"].numpy()
            out[f"{p}_con"], out[f"{p}_sup"] = st["con"].numpy(), st["sup"].numpy()      # consis_loss's value; nll_loss per sample
            for k, v in st["state"].items():
                out[f"{p}_state__{k}"] = v.numpy()
            for n_, g, m, v in zip(rec["param_names"], st["pre"], st["exp_avg"], st["exp_avg_sq"]):
                assert (g is None) == (m is None) == (v is None)
                if g is not None:
                    out[f"{p}_pre__{n_}"], out[f"{p}_m__{n_}"], out[f"{p}_v__{n_}"] = g.numpy(), m.numpy(), v.numpy()
    # what main() itself built and handed to valid and predict, the same in both runs: topk_adj without its explicit zeros
    # (the slots gfpush_omp left unfilled), the unlabelled sample and adj + I
    ta, tb = (sp.csr_matrix(recs[k]["topk"], copy=True) for k in ("t32", "r64"))
    for m in (ta, tb):
        m.eliminate_zeros()
    assert (ta != tb).nnz == 0 and (recs["t32"]["adj"] != recs["r64"]["adj"]).nnz == 0
    assert np.array_equal(recs["t32"]["idx_sample"], recs["r64"]["idx_sample"])
    coo, adj_i = tb.tocoo(), recs["r64"]["adj"]
    out.update(idx_sample=np.asarray(recs["r64"]["idx_sample"]), topk_row=coo.row.astype(np.int32), topk_col=coo.col.astype(np.int32),
               topk_val=coo.data, adj_indptr=np.array(adj_i.indptr, np.int32), adj_indices=np.array(adj_i.indices, np.int32),
               adj_data=np.array(adj_i.data, np.float64))
    assert np.array_equal(recs["t32"]["prop"], recs["r64"]["prop"])   # numpy float64 in both runs (model.py:186-194)
    out["propagated"] = recs["r64"]["prop"]
    a, b = recs["t32"]["steps"], recs["r64"]["steps"]
    for t, (sa, sb) in enumerate(zip(a, b)):                          # both runs consumed the same selections and masks
        for k in ("num_batch", "train_index", "unlabel_index_batch", "source_idx", "neighbor_idx"):
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), (name, t, k)
        assert len(sa["keeps"]) == len(sb["keeps"]) and all(torch.equal(x, y) for x, y in zip(sa["keeps"], sb["keeps"]))
        out[f"s{t}_num_batch"] = np.int64(sa["num_batch"])
        out[f"s{t}_train_index"], out[f"s{t}_unlabel_index"] = np.asarray(sa["train_index"]), np.asarray(sa["unlabel_index_batch"])
        out[f"s{t}_source_idx"], out[f"s{t}_neighbor_idx"] = sa["source_idx"].numpy(), np.asarray(sa["neighbor_idx"])
        assert torch.equal(sa["mat_scores"].double(), sb["mat_scores"])
        out[f"s{t}_mat_scores"] = sb["mat_scores"].numpy()            # float64 that holds the float32 of model.py:315
        for j, k in enumerate(sa["keeps"]):
            out[f"s{t}_keep{j}"] = k.numpy()                          # per sample: DropNode, input, hidden
    meta[f"run_{name}"] = dict(vars(args), steps_recorded=len(a), n_nodes=int(features.shape[0]), F=F, C=C,
                               valid_at=[int(v[0]) for v in recs["r64"]["valid"]], saves_at=[int(s) for s in recs["r64"]["saves"]],
                               num_batch={k: r["num_batch"] for k, r in recs.items()}, lines="model.py:227-373")
    return out


# --------------------------------------------------------------------------------------------- C. the early-stop rule
# (loss, acc), dyadic so that float32 holds them: the first evaluation; an accuracy tie with lower loss; a tie with higher
# loss; higher accuracy with higher loss; lower accuracy; a new best; two bad ones; a tie with higher loss between bad
# ones; then bad ones until patience = 3 is reached exactly
SCRIPT = [(1.0, 0.5), (0.875, 0.5), (0.9375, 0.5), (1.25, 0.625), (0.75, 0.375), (0.6875, 0.625), (0.5, 0.25), (0.5, 0.25),
          (0.71875, 0.625), (0.5, 0.25), (0.5, 0.25), (0.5, 0.25), (0.5, 0.25), (0.5, 0.25), (0.5, 0.25), (0.5, 0.25)]


def scripted_stops(model, meta):
    out = {"script": np.array(SCRIPT, dtype=np.float64), "patience": np.int64(3)}
    for mode in ("both", "acc"):
        args = run_args(stop_mode=mode, eval_batch=1, epochs=5, patience=3, **CONFIGS["plain"])
        rec = run_main(model, args, False, script=SCRIPT)
        evals = [v[0] for v in rec["valid"]]
        assert len(evals) < len(SCRIPT), "the script ran out before the rule stopped the run"
        out[f"{mode}_eval_at"] = np.array(evals, dtype=np.int64)
        out[f"{mode}_saved"] = np.array([nb in rec["saves"] for nb in evals], dtype=np.bool_)
        out[f"{mode}_stop_at"] = np.int64(rec["num_batch"])           # num_batch is not advanced after the break (model.py:359-360)
        meta[f"stop_{mode}"] = {"evaluations": len(evals), "saves_at": [int(s) for s in rec["saves"]], "stop_at": rec["num_batch"],
                                "patience": 3, "lines": "model.py:336-362"}
    return out


# ---------------------------------------------------------------------------------------------------------------- files
def record():
    """({file name: {key: array}}, meta), everything computed in memory."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                                          # one summation order
    try:
        return _record()
    finally:
        torch.set_num_threads(threads)


def _record():
    meta = {"generator": "tests/golden/make_training_golden.py",
            "reference": "model.py, model_mag.py and oracle/_ref (compiled precompute/propagation.cpp) of the reference tree"}
    files = {}
    with reference() as (model, model_mag):
        pieces = {}
        piece_random_prop(model, pieces, meta)
        piece_mlp(model, pieces, meta)
        piece_consis(model, pieces, meta)
        files["train_pieces.npz"] = pieces
        mag = {}
        piece_mag(model_mag, mag, meta)
        files["train_mag.npz"] = mag
        for name in CONFIGS:
            files[f"train_run_{name}.npz"] = whole_run(model, name, meta)
        files["train_stop.npz"] = scripted_stops(model, meta)
    return {f: {k: np.asarray(v) for k, v in d.items()} for f, d in files.items()}, meta


def write_npz(path, arrays):
    """An .npz with sorted members and a fixed time stamp: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    files, meta = record()
    for name, arrays in files.items():
        write_npz(os.path.join(HERE, name), arrays)
        print(name, len(arrays), "arrays", os.path.getsize(os.path.join(HERE, name)), "bytes")
    with open(os.path.join(HERE, "training_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
