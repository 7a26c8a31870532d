"""`fit` over a MagTrainStep on the GPU at a tiny problem of its own: V = 50, H = 8, N = 40, K = 4, S = 2, two MLP
layers with BatchNorm; 24 seed rows -- 7 labelled in batches of 3 (so every epoch ends on a short batch), then 9 unlabelled
with 4 per step, then 8 validation nodes.  The one parameter group has weight_decay = 0, so the lazy table step is allowed.

In the deterministic modes the contract is bitwise: `valid_mag` is its plan and pass, and `fit` is the hand-written loop of
`step` + `valid_mag` + the host rule, whatever the table step, `dirty_rows` and `poll_every` are.  The atomic mode is not
reproducible from run to run, so there the restored table is held to a clone taken in the same run, exactly, and to a twin
run within a bound derived below."""
import functools
import types

import numpy as np
import pytest
import torch

import optim_cases as oc
import row_mark_cases as rm

pytestmark = pytest.mark.gpu

V, H, N, K, C, S = 50, 8, 40, 4, 3, 2
N_TRAIN, N_UNLABEL, N_VAL, S_ROWS = 7, 9, 8, 24
BATCH, UNLABEL_BATCH = 3, 4
BASE_SEED, SAMPLER_SEED, LAM, WARMUP, TEM, P_NODE, CONF, LR = 0xFAB1E5EED, 0xF17, 0.8, 4, 0.5, 0.5, 0.22, 1e-2
EPOCHS = 8
LAST = EPOCHS * 3                 # three steps an epoch: 3 + 3 + 1 labelled nodes
MODES = {"dense": dict(deterministic=True), "exact": dict(deterministic=True, table_step="exact"),
         "lazy": dict(deterministic=True, table_step="lazy"), "lazy_dirty": dict(deterministic=True, table_step="lazy", dirty_rows=True)}
ATOMIC = dict(deterministic=False, table_step="lazy", row_list="bitmap")


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
    """The CPU tensors of the problem: seeds, col, val, filled, the attribute CSR (bags of 0 .. 6 entries) and labels."""
    rng = np.random.default_rng(29)
    seeds = rng.permutation(N)[:S_ROWS].astype(np.int64)
    col = rng.integers(0, N, S_ROWS * K).astype(np.int32)
    val = np.sort(rng.random((S_ROWS, K)) ** 2 + 1e-3, axis=1)[:, ::-1].copy().reshape(-1)
    filled = rng.choice(np.array([0, 2, 4], np.int32), S_ROWS, p=[0.1, 0.3, 0.6])
    filled[:3] = (4, 2, 0)
    filled[N_TRAIN:N_TRAIN + 3] = (0, 2, 4)
    filled[N_TRAIN + N_UNLABEL:] = np.maximum(filled[N_TRAIN + N_UNLABEL:], 2)      # every validation row has neighbours
    lens = rng.integers(0, 7, N)
    indptr = np.zeros(N + 1, np.int64)
    np.cumsum(lens, out=indptr[1:])
    nnz = int(indptr[-1])
    indices = rng.integers(0, V, nnz).astype(np.int32)
    data = (rng.random(nnz) + 0.05).astype(np.float32)
    labels = rng.integers(0, C, N)
    t = torch.from_numpy
    return seeds, t(col), t(val), t(filled), (t(indptr), t(indices), t(data)), t(labels)


def pools():
    seeds = world()[0]
    return seeds[:N_TRAIN], seeds[N_TRAIN:N_TRAIN + N_UNLABEL], seeds[N_TRAIN + N_UNLABEL:]


@functools.lru_cache(maxsize=None)
def resident():
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    return RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N), tuple(a.cuda() for a in attrs), labels.cuda()


def mag_step(capture, **mode):
    """(MagTrainStep, model, optimizer) over the shared problem, from the same initial state every time."""
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    rmx, attrs, labels = resident()
    torch.manual_seed(7)
    m = MagMLP(V, C, H, 2, True, 0.0, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, clip_norm=0.1, capturable=True,
                   state=StepState("cuda"))
    tr, un, _val = pools()
    ts = MagTrainStep(m, opt, rmx, *attrs, labels, tr, un, samples=S, dropnode_rate=P_NODE, lam=LAM, warmup=WARMUP, tem=TEM, conf=CONF,
                      kind="l2", seed=BASE_SEED, capture=capture, **mode)
    return ts, m, opt


def sampler():
    from grand_plus_amd import Sampler
    return Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, SAMPLER_SEED)


def selection(t):
    from grand_plus_amd._common import step_seed
    return sampler().selection(t, step_seed(BASE_SEED, t))


def named_rows(ts, t):
    """The table rows the bags of step t's batch name, from the mirror of the row list (tests/row_mark_cases.py)."""
    _seeds, col, _val, filled, (indptr, indices, _data), _labels = world()
    a, b = selection(t)
    batch = ts._pos.cpu().numpy()[np.concatenate([a, b + N_TRAIN])]
    P = types.SimpleNamespace(col=col, K=K, indptr=indptr, indices=indices, filled=filled, S_rows=S_ROWS, N=N, V=V)
    return rm.marked_rows(P, batch.tolist())


def _valid(m, batch_size=100, **kw):
    from grand_plus_amd import valid_mag
    rmx, attrs, labels = resident()
    return valid_mag(m, rmx, *attrs, pools()[2], labels, batch_size=batch_size, dropnode_rate=P_NODE, **kw)


# ---- 1. valid_mag is its plan and its pass
def test_plan_and_pass_are_valid_mag_bit_for_bit_and_the_plan_caches_no_weights():
    from grand_plus_amd import valid_mag_pass, valid_mag_plan
    rmx, attrs, labels = resident()
    ts, m, _o = mag_step(False, **MODES["lazy"])
    for batch_size in (3, 100):                                                     # three batches, the last short; one batch
        plan = valid_mag_plan(m, rmx, *attrs, pools()[2], labels, batch_size)
        assert plan.batch_size == batch_size and plan.idx.is_cuda and plan.pos.is_cuda and plan.idx.numel() == N_VAL
        first = tuple(x.clone() for x in valid_mag_pass(plan, P_NODE))
        want = _valid(m, batch_size, return_counts=True)
        assert len(first) == 3 and all(_same(x, y) for x, y in zip(first, want))
        assert m.training
        ts.step(*selection(int(ts.state.read().tick) + 1))                           # the weights move; the plan stays
        second = tuple(x.clone() for x in valid_mag_pass(plan, P_NODE))
        assert not _same(first[0], second[0]), "the pass after a training step gave the same loss: the plan holds old weights"
        want = _valid(m, batch_size, return_counts=True)
        assert all(_same(x, y) for x, y in zip(second, want)), "the second pass is not a fresh valid_mag"
        assert int(second[2][0]) == N_VAL and int(second[2][3]) == 0
    stranger = next(i for i in range(N) if i not in set(world()[0].tolist()))
    with pytest.raises(KeyError):
        valid_mag_plan(m, rmx, *attrs, np.array([int(pools()[2][0]), stranger]), labels, 3)


# ---- 2. fit against the hand-written loop
def hand_loop(mode, eval_batch, stop_mode, patience):
    """The loop a MAG caller writes without `fit`: step() on the mirror's selection, valid_mag(), two .item()s, the host
    rule, a clone of the state_dict on every improvement and a load at the end.  Returns (steps, track, model, the table
    after every step)."""
    from grand_plus_amd.fit import early_stop_rule, new_track
    ts, m, _o = mag_step(False, **{k: v for k, v in mode.items() if k != "dirty_rows"})
    track, saved, steps, tables = new_track(), None, 0, {0: m.embeds.weight.detach().clone()}
    for t in range(1, LAST + 1):
        ts.step(*selection(t))
        steps += 1
        tables[t] = m.embeds.weight.detach().clone()
        if (t - 1) % eval_batch == 0:
            loss, acc = _valid(m)
            early_stop_rule(track, loss.item(), acc.item(), t, stop_mode, patience)
            if track["copy_now"]:
                saved = {k: v.clone() for k, v in m.state_dict().items()}
            if track["stopped"]:
                break
    if saved is not None:
        m.load_state_dict(saved)
    ts.check_entries_flag()
    return steps, track, m, tables


@functools.lru_cache(maxsize=None)
def hand(name, eval_batch, stop_mode, patience):
    return hand_loop(MODES[name], eval_batch, stop_mode, patience)


CONFIGS = [("dense", 2, "both", 3), ("exact", 2, "acc", 1), ("lazy", 3, "both", 100), ("lazy_dirty", 1, "acc", 100),
           ("lazy_dirty", 1, "both", 3), ("lazy_dirty", 2, "acc", 3), ("lazy", 1, "both", 1)]
LATER_BEST = CONFIGS[3]           # ties in accuracy count under `acc`: the best is taken again after step 1
DRIFT = CONFIGS[4]                # the rule stops the run some validations after its best


@pytest.mark.parametrize("name,eval_batch,stop_mode,patience", CONFIGS)
@pytest.mark.parametrize("poll_every", [1, 4])
def test_fit_is_the_hand_written_loop(name, eval_batch, stop_mode, patience, poll_every):
    import grand_plus_amd
    steps, track, hm, _tables = hand(name, eval_batch, stop_mode, patience)
    if (name, eval_batch, stop_mode, patience) == LATER_BEST:         # a precondition of the case, read off the hand-written loop
        assert track["best_tick"] > 1, "this case is here to restore a snapshot taken after earlier ones"
    ts, m, _o = mag_step(True, **MODES[name])
    assert (ts.row_grad is not None and ts.row_grad.dirty is not None) == (name == "lazy_dirty")
    res = grand_plus_amd.fit(ts, sampler(), pools()[2], epochs=EPOCHS, eval_batch=eval_batch, stop_mode=stop_mode, patience=patience,
                             poll_every=poll_every)
    print(f"{name} eval_batch={eval_batch} {stop_mode} patience={patience} poll_every={poll_every}: hand {steps} steps, "
          f"best {track['best_tick']}, stop {track['stop_tick']}; fit {res}")
    assert res.best_tick == (track["best_tick"] or None)
    assert res.stop_tick == (track["stop_tick"] if track["stopped"] else None)
    assert np.float32(res.best_loss).view(np.int32) == np.float32(track["best_loss"]).view(np.int32)
    assert np.float32(res.best_acc).view(np.int32) == np.float32(track["best_acc"]).view(np.int32)
    if poll_every == 1:
        assert res.steps == steps                                    # the reference's step
    else:
        assert steps <= res.steps <= min(steps + poll_every * eval_batch, LAST)
    assert _same_state(m, hm), "the restored state_dict differs from the hand-written loop's"
    assert m.training and ts.state.read().tick == res.steps
    if patience == 100:
        assert res.stop_tick is None and res.steps == LAST
    else:
        assert res.best_tick is not None
    ts.check_entries_flag()


def test_a_row_that_drifts_after_the_best_comes_back_as_of_the_best_tick():
    import grand_plus_amd
    name, eval_batch, stop_mode, patience = DRIFT
    steps, track, _hm, tables = hand(name, eval_batch, stop_mode, patience)
    best = track["best_tick"]
    assert 1 <= best < steps, "this case needs steps after the best tick"
    moved = (_bits(tables[best]) != _bits(tables[steps])).any(dim=1)
    assert bool(moved.any()) and not bool(moved.all()), "this case needs a table row that changes after the best tick, and one that does not"
    ts, m, _o = mag_step(True, **MODES[name])
    res = grand_plus_amd.fit(ts, sampler(), pools()[2], epochs=EPOCHS, eval_batch=eval_batch, stop_mode=stop_mode, patience=patience)
    assert res.best_tick == best and res.steps == steps
    w = m.embeds.weight.detach()
    assert _same(w, tables[best]), "the restored table is not the table of the best tick"
    assert bool((_bits(w)[moved] != _bits(tables[steps])[moved]).any(dim=1).all()), "a row that drifted came back as trained"


# ---- 3. the atomic lazy step with a bitmap row list
def _adam_move_bound(t):
    """An upper bound of |m_hat| / sqrt(v_hat) at Adam step t, for any gradient sequence: by Cauchy-Schwarz over the t terms,
    |m_t| <= (1 - b1) sqrt(sum_k (b1^2 / b2)^k) sqrt(v_t / (1 - b2)), and the bias corrections multiply by
    sqrt(1 - b2^t) / (1 - b1^t).  It is 1 at t = 1, the rule of tests/test_gpu_mag_step.py (an element moves by at most lr in
    Adam's first step).  A row the lazy step touched fewer than t times has fewer terms in the sum: the bound still holds."""
    b1, b2 = oc.BETAS
    return (1 - b1) / np.sqrt(1 - b2) * np.sqrt(sum((b1 * b1 / b2) ** k for k in range(t))) * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)


def test_the_atomic_lazy_bitmap_step_restores_the_table_of_its_best_tick():
    from grand_plus_amd.fit import FitLoop
    ts, m, _o = mag_step(True, dirty_rows=True, **ATOMIC)
    loop = FitLoop(ts, sampler(), pools()[2], eval_batch=1, stop_mode="both", patience=3)
    assert loop.valid_batch == 100 and loop.tracker.row_grad is ts.row_grad
    first = m.embeds.weight.detach().clone()
    clone, image = None, None
    while loop.t < LAST:
        assert loop.advance()
        image = loop.poll()
        if image.best_tick == loop.t:
            assert image.copy_now == 1
            clone = m.embeds.weight.detach().clone()                  # the twin of the snapshot, taken whole in the same run
        else:
            assert image.copy_now == 0
        if image.stopped:
            break
    best = image.best_tick
    # the tracker's fields agree with each other
    assert clone is not None and 1 <= best <= loop.t and image.n_evals == loop.t and 0 <= image.bad_counter <= 3
    assert (image.stopped == 1) == (image.bad_counter >= 3) and (image.stop_tick == loop.t if image.stopped else image.stop_tick == 0)
    assert np.isfinite(image.best_loss) and 0.0 <= image.best_acc <= 1.0
    trained = m.embeds.weight.detach().clone()
    later = np.zeros(V, bool)
    for t in range(best + 1, loop.t + 1):
        later[named_rows(ts, t)] = True
    quiet = torch.from_numpy(~later)
    assert _same(trained[quiet], clone[quiet]), "a row no batch named after the best tick moved all the same"
    res = loop.finish()
    assert res.best_tick == best and res.steps == loop.t
    assert _same(m.embeds.weight.detach(), clone), "the restored table is not the table of the best tick"
    ts.check_entries_flag()
    # a twin run: the atomics sum in another order, so only rows no batch has named yet are equal bit for bit; every
    # other element lies within twice the way one run can have moved it
    twin, tm, _to = mag_step(False, **ATOMIC)
    ever = np.zeros(V, bool)
    for t in range(1, best + 1):
        twin.step(*selection(t))
        ever[named_rows(twin, t)] = True
    got, want = m.embeds.weight.detach(), tm.embeds.weight.detach()
    untouched = torch.from_numpy(~ever)
    assert _same(got[untouched], want[untouched]) and _same(got[untouched], first[untouched])
    bound = 2 * LR * sum(_adam_move_bound(t) for t in range(1, best + 1)) + 1e-6
    assert float((got - want).abs().max()) <= bound, f"the twin's table differs by more than {bound}"


# ---- 4. the steady state does not synchronise
def test_the_steady_state_loop_does_not_synchronise():
    import grand_plus_amd
    from grand_plus_amd.fit import FitLoop
    ts, m, _o = mag_step(True, **MODES["lazy_dirty"])
    loop = FitLoop(ts, sampler(), pools()[2], eval_batch=2, stop_mode="both", patience=10 ** 6)
    for _ in range(9):                                               # warm-up: code load, both shapes captured, a few validations
        loop.advance()
    assert all(v is not None for v in ts._sampled.values()) and len(ts._sampled) == 2
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        evaluated = [loop.advance() for _ in range(12)]              # replays, validations, tracker updates: nothing may wait
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert sum(evaluated) == 6 and loop.t == 21
    image = loop.poll()
    assert image.n_evals == 11 and image.stopped == 0
    res = loop.finish()
    assert res.steps == 21 and res.stop_tick is None
    ts2, _m2, _o2 = mag_step(True, dirty_rows=True, **ATOMIC)          # fit itself, polling never, over the atomic step
    res = grand_plus_amd.fit(ts2, sampler(), pools()[2], epochs=100, eval_batch=2, patience=10 ** 6, poll_every=10 ** 6, max_steps=12)
    assert res.steps == 12 and res.stop_tick is None and ts2.state.read().tick == 12


# ---- 5. the mark is part of every graph
@pytest.mark.parametrize("mode", [MODES["lazy_dirty"], dict(ATOMIC, dirty_rows=True)], ids=["deterministic", "atomic-bitmap"])
def test_each_replayed_step_marks_the_rows_of_its_own_batch(mode):
    """Two batch shapes, two graphs, one RowGrad: `RowGrad.keys` describes the graph captured last, so a mark issued outside
    the graphs from those attributes would mark the wrong rows on every replay of the other shape."""
    ts, _m, _o = mag_step(True, **mode)
    s = sampler()
    dirty = ts.row_grad.dirty
    assert dirty is not None and dirty.shape == (rm.words(V),) and not bool(dirty.any())
    shapes = []
    for t in range(1, 13):
        dirty.zero_()
        ts.step_sampled(s, t)
        got = rm.rows_of(dirty.cpu().numpy().view(np.uint32), V)
        want = named_rows(ts, t)
        assert 0 < len(want) < V and np.array_equal(got, want), f"step {t} (shape {s.shape(t)}): the marked rows are not its batch's"
        shapes.append(s.shape(t))
    assert len(ts._sampled) == 2 and all(v is not None for v in ts._sampled.values())
    assert shapes[-3:] == [(3, 4), (3, 4), (1, 4)] and len({tuple(named_rows(ts, t)) for t in range(10, 13)}) == 3
    # without a snapshot in between the bits accumulate
    dirty.zero_()
    union = np.zeros(V, bool)
    for t in range(13, 16):
        ts.step_sampled(s, t)
        union[named_rows(ts, t)] = True
    assert np.array_equal(rm.rows_of(dirty.cpu().numpy().view(np.uint32), V), np.flatnonzero(union))
    ts.check_selection_flag()
    ts.check_entries_flag()


# ---- 6. without dirty_rows nothing changes
@pytest.mark.parametrize("mode", [MODES["lazy"], MODES["dense"]], ids=["lazy", "dense"])
def test_a_step_without_dirty_rows_is_the_step_it_was(mode, monkeypatch):
    import step_cases as sc
    from grand_plus_amd import fit as gfit
    monkeypatch.setattr(gfit, "rows_mark", lambda *a: pytest.fail("a step without dirty_rows marked rows"))
    got, gm, go = mag_step(True, dirty_rows=False, **mode)
    ref, rm_, ro = mag_step(True, **mode)                            # built as before this keyword existed
    assert got.dirty_rows is False and ref.dirty_rows is False
    assert got.row_grad is None or got.row_grad.dirty is None
    s = sampler()
    for t in range(1, 8):                                            # eager, captured, then replays of both shapes
        a, b = got.step_sampled(s, t), ref.step_sampled(s, t)
        for field, x, y in zip(a._fields, a, b):
            assert _same(x, y), f"step {t}: {field} differs"
    for i, (x, y) in enumerate(zip(sc.snapshot(gm, go), sc.snapshot(rm_, ro))):
        assert _same(x, y), f"tensor {i} of the snapshot differs"
    assert len(got._sampled) == 2 and all(v is not None for v in got._sampled.values())
