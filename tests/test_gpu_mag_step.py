"""MAG's captured training step on the GPU (grand_plus_amd/mag_step.py) at a tiny problem: V = 50, H = 8,
N = 40, K = 4, pools of 7 and 9 nodes, batches of 3 + 4, S = 2, two MLP layers with BatchNorm, hidden dropout 0.5.

In deterministic mode the contract is bitwise: a replayed step equals the eager step of the same body (`capture=False`) in
every parameter, Adam state tensor and result, and `step_sampled` equals `step` on the mirror's selection.  The atomic mode
shares the forward, so its first step's losses are the deterministic step's bit for bit; its parameters after one step lie
within the rule tests/test_gpu_mag_rows.py holds a ClipAdam step to (an element moves by at most lr in Adam's first step,
so two steps from the same state differ by at most 2 * lr)."""
import functools

import numpy as np
import pytest
import torch

import step_cases as sc

pytestmark = pytest.mark.gpu

V, H, N, K, C, S = 50, 8, 40, 4, 3, 2
N_TRAIN, N_UNLABEL, S_ROWS = 7, 9, 16
BATCH, UNLABEL_BATCH = 3, 4
BASE_SEED, LAM, WARMUP, TEM, P_NODE, CONF, LR = 0x5EED0FACADE, 0.8, 4, 0.5, 0.5, 0.22, 1e-2


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def world():
    """The CPU tensors of the problem: seeds, col, val, filled, the attribute CSR (bags of 0 .. 6 entries) and labels."""
    rng = np.random.default_rng(23)
    seeds = rng.permutation(N)[:S_ROWS].astype(np.int64)
    col = rng.integers(0, N, S_ROWS * K).astype(np.int32)
    val = np.sort(rng.random((S_ROWS, K)) ** 2 + 1e-3, axis=1)[:, ::-1].copy().reshape(-1)
    filled = rng.choice(np.array([0, 2, 4], np.int32), S_ROWS)
    filled[:3] = (4, 2, 0)
    filled[N_TRAIN:N_TRAIN + 3] = (0, 2, 4)
    lens = rng.integers(0, 7, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = rng.integers(0, V, nnz).astype(np.int32)
    data = (rng.random(nnz) + 0.05).astype(np.float32)
    labels = rng.integers(0, C, N)
    t = torch.from_numpy
    return seeds, t(col), t(val), t(filled), (t(indptr), t(indices), t(data)), t(labels), int(lens.max())


def mag_step(capture, deterministic, nlayers=2, max_entries=None):
    """(MagTrainStep, model, optimizer) over the shared problem, from the same initial state every time."""
    import optim_cases as oc
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels, _longest = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    rm = RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N)
    torch.manual_seed(7)
    m = MagMLP(V, C, H, nlayers, True, 0.0, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=5e-4, clip_norm=0.1, capturable=True,
                   state=StepState("cuda"))
    ts = MagTrainStep(m, opt, rm, *(a.cuda() for a in attrs), labels.cuda(), seeds[:N_TRAIN], seeds[N_TRAIN:], samples=S,
                      dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM, conf=CONF, kind="l2", seed=BASE_SEED, capture=capture,
                      deterministic=deterministic, max_entries=max_entries)
    return ts, m, opt


def selection(t, n_l=BATCH, n_u=UNLABEL_BATCH):
    rng = np.random.default_rng(2000 + t)
    return rng.choice(N_TRAIN, n_l, replace=False), rng.choice(N_UNLABEL, n_u, replace=False)


def _assert_twins(a, b, what):
    (ra, ma, oa), (rb, mb, ob) = a, b
    for name, x, y in zip(ra._fields, ra, rb):
        assert _same(x, y), f"{what}: {name} differs: {x.item()} vs {y.item()}"
    sa, sb = sc.snapshot(ma, oa), sc.snapshot(mb, ob)
    assert len(sa) == len(sb)
    for i, (x, y) in enumerate(zip(sa, sb)):
        assert _same(x, y), f"{what}: tensor {i} of the snapshot differs"


# ---- deterministic mode
def test_three_replayed_steps_equal_three_eager_steps_bit_for_bit():
    cap, cm, co = mag_step(True, True)
    eag, em, eo = mag_step(False, True)
    assert 1 <= cap.longest_bag <= world()[6] and cap._max_entries(7) == 7 * K * cap.longest_bag
    w0 = cm.embeds.weight.detach().clone()
    losses = []
    for t in range(1, 4):
        sel = selection(t)
        rc, re = cap.step(*sel), eag.step(*sel)
        _assert_twins((rc, cm, co), (re, em, eo), f"step {t}")
        losses.append(float(rc.loss))
    assert cap.state.read().tick == eag.state.read().tick == 3
    assert len(cap._shapes) == 1 and cap._shapes[(7, 3)] is not None and not eag._shapes
    assert all(np.isfinite(x) for x in losses) and not torch.equal(w0, cm.embeds.weight)       # the table is trained
    for ts in (cap, eag):
        ts.check_entries_flag()                                                  # B * K * Lmax cannot overflow: silent
    # a fourth step, a replay, waits for nothing
    sel = selection(4)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rc = tuple(x.clone() for x in cap.step(*sel))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    re = eag.step(*sel)
    for name, x, y in zip(re._fields, rc, re):
        assert _same(x, y), f"step 4: {name} differs"
    _assert_twins((re, cm, co), (re, em, eo), "step 4")


def test_step_sampled_is_step_on_the_mirrors_selection_and_each_shape_gets_its_graph():
    """Three epochs of 3 + 3 + 1 labelled nodes: the short last batch is a second shape with a graph of its own."""
    from grand_plus_amd import Sampler
    from grand_plus_amd._common import step_seed
    s = Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, 11)
    got, gm, go = mag_step(True, True)
    ref, rm_, ro = mag_step(False, True)
    shapes = []
    for t in range(1, 10):
        a = got.step_sampled(s, t)
        b = ref.step(*s.selection(t, step_seed(BASE_SEED, t)))
        _assert_twins((a, gm, go), (b, rm_, ro), f"step {t}")
        shapes.append(s.shape(t))
    assert shapes[:3] == [(3, 4), (3, 4), (1, 4)]
    assert len(got._sampled) == 2 and all(v is not None for v in got._sampled.values())
    got.check_selection_flag()
    got.check_entries_flag()


def test_a_tight_max_entries_sets_the_flag_and_the_check_raises():
    ts, _m, _o = mag_step(True, True, max_entries=1)
    for t in range(1, 4):                                                        # eager, captured, replayed
        ts.step(*selection(t))
    with pytest.raises(RuntimeError, match="more entries than max_entries = 1"):
        ts.check_entries_flag()


def test_one_layer_runs_a_captured_step():
    """nlayers = 1: no fcs, the embedding is the logits."""
    cap, cm, co = mag_step(True, True, nlayers=1)
    eag, em, eo = mag_step(False, True, nlayers=1)
    assert not len(cm.fcs) and len(co.param_groups[0]["params"]) == 1
    for t in range(1, 4):
        sel = selection(t)
        _assert_twins((cap.step(*sel), cm, co), (eag.step(*sel), em, eo), f"one layer, step {t}")
    assert cap._shapes[(7, 3)] is not None


# ---- atomic mode
def test_the_atomic_step_shares_the_forward_and_its_replay_runs():
    det, dm, do = mag_step(False, True)
    ato, am, ao = mag_step(True, False)
    sel = selection(1)
    rd, ra = det.step(*sel), ato.step(*sel)
    for name in ("sup", "con", "loss", "n_conf", "n_correct"):
        assert _same(getattr(rd, name), getattr(ra, name)), name                 # the forward is shared
    for i, (x, y) in enumerate(zip(sc.snapshot(dm, do), sc.snapshot(am, ao))):
        if x.dtype == torch.float32 and i < len(do.param_groups[0]["params"]):
            assert float((x - y).abs().max()) <= 2 * LR + 1e-6, f"parameter {i}"
    losses = [float(ato.step(*selection(t)).loss) for t in range(2, 5)]          # captured, then replayed twice
    assert ato._shapes[(7, 3)] is not None and all(np.isfinite(x) for x in losses)
    assert ato.state.read().tick == 4
    ato.check_entries_flag()
