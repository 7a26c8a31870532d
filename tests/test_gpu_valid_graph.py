"""The one-pass validation, ValidGraph and their wiring into `fit` on the GPU, at a small problem of its own:
120 nodes, 64 seed rows of K = 8 -- 9 labelled in batches of 4, 18 unlabelled with 5 per step, 37 validation nodes --, F = 48,
hidden 64, C = 7, two layers, BatchNorm and node_norm on and off; MAG's twin reads a V = 50, H = 16 attribute CSR.

Every contract is bitwise: the one-pass validation is the eager composition gather -> infer -> eval_head -> eval_reduce,
whatever the batch size; a ValidGraph run -- eager, capturing or replayed -- is an eager pass + tracker.update on a twin that
took the same training steps; fit with valid_capture is fit without it."""
import functools

import numpy as np
import pytest
import torch

import optim_cases as oc
import step_cases as sc

pytestmark = pytest.mark.gpu

N, ROWS, K, F, HID, C = 120, 64, 8, 48, 64, 7
V, H = 50, 16
N_TRAIN, N_UNLABEL, N_VAL, BATCH, UNLABEL_BATCH = 9, 18, 37, 4, 5
SAMPLER_SEED, P_NODE = 0xF17, 0.5
LAYOUTS = {"plain": False, "bn_norm": True}                  # use_bn and node_norm
KINDS = ("grand", "mag", "mag_dirty")
BATCHES = (1, 5, 37, 10000)


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _same_state(ma, mb):
    sa, sb = ma.state_dict(), mb.state_dict()
    return list(sa) == list(sb) and all(_same(sa[k], sb[k]) for k in sa)


@functools.lru_cache(maxsize=None)
def world():
    rng = np.random.default_rng(31)
    seeds = rng.permutation(N)[:ROWS].astype(np.int64)
    col = rng.integers(0, N, ROWS * K).astype(np.int32)
    val = np.sort(rng.random((ROWS, K)) ** 2 + 1e-3, axis=1)[:, ::-1].copy().reshape(-1)
    filled = rng.choice(np.array([0, 3, 8], np.int32), ROWS, p=[0.1, 0.3, 0.6])
    filled[N_TRAIN + N_UNLABEL:] = np.maximum(filled[N_TRAIN + N_UNLABEL:], 3)
    filled[N_TRAIN + N_UNLABEL] = 0                            # one validation row without neighbours
    gen = torch.Generator().manual_seed(32)
    X = torch.randn((N, F), generator=gen)
    labels = torch.randint(0, C, (N,), generator=gen)
    lens = rng.integers(0, 7, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    attrs = (torch.from_numpy(indptr), torch.from_numpy(rng.integers(0, V, nnz).astype(np.int32)),
             torch.from_numpy((rng.random(nnz) + 0.05).astype(np.float32)))
    return seeds, torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(filled), X, labels, attrs


def pools():
    seeds = world()[0]
    return seeds[:N_TRAIN], seeds[N_TRAIN:N_TRAIN + N_UNLABEL], seeds[N_TRAIN + N_UNLABEL:]


@functools.lru_cache(maxsize=None)
def resident():
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, X, labels, attrs = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    return RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N), X.cuda(), labels.cuda(), tuple(a.cuda() for a in attrs)


def make_step(kind, bn=True, capture=True):
    """(step, model) of a kind over the shared problem, from the same initial state every time."""
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, TrainStep, mag_trained_parameters
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    from grand_plus_amd.step import trained_parameters
    rmx, X, labels, attrs = resident()
    tr, un, _val = pools()
    torch.manual_seed(5)
    common = dict(samples=2, dropnode_rate=P_NODE, lam=sc.LAM, warmup=sc.WARMUP, tem=sc.TEM, conf=sc.CONF, kind="l2", seed=sc.BASE_SEED,
                  capture=capture)
    if kind == "grand":
        m = GrandPlusMLP(F, C, HID, 2, bn, 0.0, 0.5, bn).cuda().train()
        return TrainStep(m, sc.optimizer(trained_parameters(m), True), rmx, X, labels, tr, un, **common), m
    m = MagMLP(V, C, H, 2, bn, 0.0, 0.5, bn).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=1e-2, betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, clip_norm=0.1, capturable=True,
                   state=StepState("cuda"))
    mode = dict(deterministic=True, table_step="lazy", dirty_rows=kind == "mag_dirty")
    return MagTrainStep(m, opt, rmx, *attrs, labels, tr, un, **common, **mode), m


def sampler():
    from grand_plus_amd import Sampler
    return Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, SAMPLER_SEED)


def _modes(m):
    return m.training, torch.is_grad_enabled(), torch.cuda.get_sync_debug_mode()


# ---- 1. the one-pass validation is the eager composition, whatever the batch size
def _composition(kind, m):
    """random_prop_rows (or MAG's emb_rows) -> infer -> eval_head -> eval_reduce over the whole validation set, by hand."""
    from grand_plus_amd import eval_head, eval_reduce
    from grand_plus_amd.augment import random_prop_rows
    rmx, X, labels, attrs = resident()
    idx = torch.from_numpy(pools()[2]).cuda()
    pos = rmx.batch_positions(idx, check=True)
    was = m.training
    m.eval()
    with torch.no_grad():
        if kind == "grand":
            aug = random_prop_rows(X, rmx.col, rmx.val, rmx.filled, rmx.K, batch_rows=pos, dropnode_rate=P_NODE, training=False)
        else:
            aug = m.emb_rows(*attrs, rmx, batch_rows=pos, dropnode_rate=P_NODE)
        buf = eval_head(m.infer(aug), labels, label_rows=idx)
        loss, acc, counts = eval_reduce(buf)
    m.train(was)
    return loss, acc, counts, buf


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["grand", "mag"])
def test_one_pass_is_the_eager_composition_at_every_batch_size(kind, layout):
    step, m = make_step(kind, LAYOUTS[layout], capture=False)
    s = sampler()
    for t in (1, 2, 3):                                        # the BatchNorm statistics are no longer their initial values
        step.step_sampled(s, t)
    want = _composition(kind, m)
    assert want[2].tolist()[0] == N_VAL and want[2].tolist()[2:] == [0, 0]
    _rmx, X, labels, attrs = resident()
    for batch in BATCHES:
        for fused in (False, True):
            if kind == "grand":
                from grand_plus_amd.evaluate import valid, valid_pass, valid_plan
                plan = valid_plan(m, step.rows, X, pools()[2], labels, batch, one_pass=True, fused=fused)
            else:
                from grand_plus_amd.mag import valid_mag_pass as valid_pass, valid_mag_plan
                plan = valid_mag_plan(m, step.rows, *attrs, pools()[2], labels, batch, one_pass=True, fused=fused)
            assert plan.one is not None and plan.one.fused is fused and plan.one.logits.shape == (N_VAL, C)
            before = _modes(m)
            if fused and len(m._layers()) < 2:                 # the fused kernel is two blocks: `infer` refuses, the modes are restored
                with pytest.raises(ValueError):
                    valid_pass(plan, P_NODE)
                assert _modes(m) == before
                continue
            ptrs = [t.data_ptr() for t in (*plan.buf, plan.one.logits, plan.one.out2, plan.one.counts, plan.one.workspace)]
            for again in range(2):                             # the plan's buffers are reused, the ticket counter is back at zero
                got = valid_pass(plan, P_NODE)
                what = f"{kind} {layout} batch={batch} fused={fused} pass {again}"
                assert all(_same(a, b) for a, b in zip(got, want[:3])), what
                assert all(_same(a, b) for a, b in zip(plan.buf, want[3])), what
                assert got[0].data_ptr() == plan.one.out2.data_ptr() and got[2].data_ptr() == plan.one.counts.data_ptr()
                assert _modes(m) == before and not plan.one.workspace.any()
            assert ptrs == [t.data_ptr() for t in (*plan.buf, plan.one.logits, plan.one.out2, plan.one.counts, plan.one.workspace)]
            if kind == "grand" and batch == 5 and not fused:   # `valid` itself, and the batched pass over the same plan
                loss, acc, counts = valid(m, step.rows, X, pools()[2], labels, batch, P_NODE, return_counts=True, one_pass=True)
                assert all(_same(a, b) for a, b in zip((loss, acc, counts), want[:3]))
                batched = valid_pass(plan, P_NODE, one_pass=False)
                ref = valid(m, step.rows, X, pools()[2], labels, batch, P_NODE, return_counts=True)
                assert all(_same(a, b) for a, b in zip(batched, ref))
                print(f"[valid_graph] {layout}: one-pass loss {float(got[0])!r}, batched loss {float(ref[0])!r}")


# ---- 2. ValidGraph: eager, capturing and replayed runs equal an eager pass + tracker.update on a twin
def _plan_of(step, batch, one_pass):
    return step._valid_plan(pools()[2], batch, one_pass=True) if one_pass else step._valid_plan(pools()[2], batch)


def _tracker(step, m, patience=100):                      # never stops in five validations: every update counts
    from grand_plus_amd import BestTracker
    return BestTracker(m, step.device, "both", patience, row_grad=step.row_grad if getattr(step, "dirty_rows", False) else None)


@pytest.mark.parametrize("one_pass", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_every_run_of_a_valid_graph_is_the_eager_pass_and_update_of_a_twin(kind, one_pass):
    from grand_plus_amd import ValidGraph
    (got, gm), (ref, rm_) = make_step(kind), make_step(kind)
    s = sampler()
    gplan, rplan = _plan_of(got, 10, one_pass), _plan_of(ref, 10, one_pass)
    gtrk, rtrk = _tracker(got, gm), _tracker(ref, rm_)
    vg = ValidGraph(gplan, P_NODE, gtrk, got.state)
    assert vg.runs == 0
    took = []
    for t in range(1, 6):                                      # a training step in between changes weights and statistics in place
        got.step_sampled(s, t)
        ref.step_sampled(s, t)
        before = _modes(gm)
        assert before[0] is True
        if t == 5:                                             # a replay under the strictest mode: nothing in it synchronises
            torch.cuda.set_sync_debug_mode("error")
        try:
            a = vg.run()
        finally:
            torch.cuda.set_sync_debug_mode(before[2])
        assert _modes(gm) == before and vg.runs == t
        loss, acc, counts = ref._valid_pass(rplan)
        rtrk.update(loss, acc, ref.state)
        what = f"{kind} one_pass={one_pass} run {t}"
        assert all(_same(x, y) for x, y in zip(a, (loss, acc, counts))), what
        gi, ri = gtrk.read(), rtrk.read()
        assert gi == ri and gi.n_evals == t, (what, gi, ri)
        assert all(_same(x, y) for x, y in zip(gtrk.snapshot, rtrk.snapshot)), what
        assert _same_state(gm, rm_), what
        if kind == "mag_dirty":
            assert _same(got.row_grad.dirty, ref.row_grad.dirty), what
        took.append(gi.copy_now)
        if t >= 3:                                             # replays hand back the static tensors of the capture
            assert a[0].data_ptr() == first[0].data_ptr() and a[2].data_ptr() == first[2].data_ptr()
        elif t == 2:
            first = a
    assert vg._graph is not None and 1 in took
    if kind == "mag_dirty":
        table = gm.embeds.weight
        snap = gtrk.snapshot[[i for i, x in enumerate(gtrk.tensors) if x.data_ptr() == table.data_ptr()][0]]
        assert _same(snap, rtrk.snapshot[[i for i, x in enumerate(rtrk.tensors) if x.data_ptr() == rm_.embeds.weight.data_ptr()][0]])


def test_a_valid_graph_without_a_tracker_and_a_moved_parameter():
    from grand_plus_amd import ValidGraph
    from grand_plus_amd.evaluate import valid_pass
    step, m = make_step("grand")
    plan = _plan_of(step, 10, True)
    vg = ValidGraph(plan, P_NODE)
    s = sampler()
    for t in (1, 2, 3):
        step.step_sampled(s, t)
        got = vg.run()
        assert all(_same(a, b) for a, b in zip(got, valid_pass(_plan_of(step, 10, True), P_NODE))), t
    with torch.no_grad():
        m.fcs[0].weight.mul_(0.5)                              # in place: the graph sees it
    got = vg.run()
    assert all(_same(a, b) for a, b in zip(got, valid_pass(_plan_of(step, 10, True), P_NODE)))
    m.fcs[0].weight.data = m.fcs[0].weight.data.clone()        # moved: the graph would read the old storage
    before = _modes(m)
    with pytest.raises(RuntimeError, match=r"fcs\.0\.weight moved since the validation pass was captured"):
        vg.run()
    assert _modes(m) == before


# ---- 3. fit with the validation captured is fit
def _fit(kind, poll_every, **kw):
    from grand_plus_amd import fit
    step, m = make_step(kind)
    res = fit(step, sampler(), pools()[2], epochs=14, eval_batch=5, stop_mode="both", patience=1, poll_every=poll_every, max_steps=40,
              valid_batch=10, **kw)
    assert m.training and torch.is_grad_enabled() and torch.cuda.get_sync_debug_mode() == 0
    return res, m


@pytest.mark.parametrize("poll_every", [1, 4])
@pytest.mark.parametrize("kind", ["grand", "mag_dirty"])
def test_fit_with_the_validation_captured_is_fit(kind, poll_every):
    plain, pm = _fit(kind, poll_every)
    captured, cm = _fit(kind, poll_every, valid_capture=True)
    assert plain == captured and _same_state(pm, cm), (plain, captured)
    assert plain.stop_tick is not None and plain.best_tick is not None and plain.steps < 40      # the rule stopped the run
    one, om = _fit(kind, poll_every, valid_one_pass=True)
    both, bm = _fit(kind, poll_every, valid_one_pass=True, valid_capture=True)
    assert one == both and _same_state(om, bm), (one, both)
    print(f"[valid_graph] fit {kind} poll_every={poll_every}: batched {plain}, one-pass {one}")
