"""The fit loop on the GPU, on a synthetic problem: 200 nodes, F = 8, C = 3, 7 labelled nodes in batches of
3 (so every epoch ends on a short batch), 4 of 30 unlabelled nodes per step, 20 validation nodes; one model without
BatchNorm and one with.

The contracts are bitwise: `step_sampled` is `step` on the mirror's selection, and `fit` is the hand-written loop of
`step` + `valid` + the host rule, whatever `poll_every` is."""
import functools

import numpy as np
import pytest
import torch

import step_cases as sc

pytestmark = pytest.mark.gpu

N, ROWS, K, F, C, H = 200, 64, 4, 8, 3, 8
N_TRAIN, N_UNLABEL, N_VAL, BATCH, UNLABEL_BATCH = 7, 30, 20, 3, 4
SAMPLER_SEED = 0xF17
LAYOUTS = {"plain": (False, 0.5, 0.5, "l2"), "bn": (True, 0.0, 0.5, "kl")}       # use_bn / node_norm, dropouts, loss


@functools.lru_cache(maxsize=None)
def problem():
    rng = np.random.default_rng(21)
    seeds = rng.permutation(N)[:ROWS].astype(np.int64)
    col = rng.integers(0, N, ROWS * K).astype(np.int32)
    val = np.sort(rng.random((ROWS, K)) ** 2, axis=1)[:, ::-1].copy().reshape(-1)
    filled = rng.choice(np.array([0, 2, 4], np.int32), ROWS, p=[0.1, 0.3, 0.6])
    gen = torch.Generator().manual_seed(22)
    X = torch.randn((N, F), generator=gen)
    labels = torch.randint(0, C, (N,), generator=gen)
    return seeds, torch.from_numpy(col), torch.from_numpy(val), torch.from_numpy(filled), X, labels


def pools():
    seeds = problem()[0]
    return seeds[:N_TRAIN], seeds[N_TRAIN:N_TRAIN + N_UNLABEL], seeds[N_TRAIN + N_UNLABEL:N_TRAIN + N_UNLABEL + N_VAL]


@functools.lru_cache(maxsize=None)
def resident():
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, X, labels = problem()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    return RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N), X.cuda(), labels.cuda()


def train_step(name, capture):
    from grand_plus_amd import TrainStep
    from grand_plus_amd.mlp import GrandPlusMLP
    from grand_plus_amd.step import trained_parameters
    bn, p_in, p_hid, kind = LAYOUTS[name]
    rm, X, labels = resident()
    torch.manual_seed(5)
    m = GrandPlusMLP(F, C, H, 2, bn, p_in, p_hid, bn).cuda().train()
    opt = sc.optimizer(trained_parameters(m), True)
    tr, un, _val = pools()
    ts = TrainStep(m, opt, rm, X, labels, tr, un, samples=2, dropnode_rate=sc.P_NODE, lam=sc.LAM, warmup=sc.WARMUP, tem=sc.TEM,
                   conf=sc.CONF, kind=kind, seed=sc.BASE_SEED, capture=capture)
    return ts, m, opt


def sampler():
    from grand_plus_amd import Sampler
    return Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, SAMPLER_SEED)


def _bits(a):
    a = a.detach().contiguous()
    return a.view(torch.int32) if a.dtype == torch.float32 else a


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _same_state(ma, mb):
    sa, sb = ma.state_dict(), mb.state_dict()
    return list(sa) == list(sb) and all(_same(sa[k], sb[k]) for k in sa)


# ---- 1. step_sampled is step on the mirror's selection
@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("capture", [False, True])
def test_step_sampled_equals_step_on_the_mirrors_selection(name, capture):
    from grand_plus_amd._common import step_seed
    s = sampler()
    got, gm, go = train_step(name, capture)
    ref, rm_, ro = train_step(name, False)
    shapes = []
    for t in range(1, 10):                                          # three epochs: each of the two shapes three times and more
        a = got.step_sampled(s, t)
        b = ref.step(*s.selection(t, step_seed(sc.BASE_SEED, t)))
        for field, x, y in zip(a._fields, a, b):
            assert _same(x, y), f"{name} capture={capture} step {t}: {field} differs: {x.item()} vs {y.item()}"
        if t in (7, 9):
            for i, (x, y) in enumerate(zip(sc.snapshot(gm, go), sc.snapshot(rm_, ro))):
                assert _same(x, y), f"{name} capture={capture} after step {t}: tensor {i} of the snapshot differs"
        shapes.append(s.shape(t))
    assert got.state.read().tick == ref.state.read().tick == 9
    assert shapes.count((3, 4)) == 6 and shapes.count((1, 4)) == 3
    got.check_selection_flag()
    assert not got._shapes                                           # step()'s graphs are apart from step_sampled()'s
    if capture:
        assert len(got._sampled) == 2 and all(v is not None for v in got._sampled.values())
        assert sorted(k[:2] for k in got._sampled) == [(5, 1), (7, 3)]
    else:
        assert not got._sampled


def test_a_wrong_tick_is_flagged_and_a_foreign_sampler_refused():
    from grand_plus_amd import Sampler
    ts, _m, _o = train_step("plain", False)
    s = sampler()
    ts.step_sampled(s, 1)
    ts.check_selection_flag()
    ts.step_sampled(s, 3)                                            # the state is at step 2: a full batch, not step 3's short one
    with pytest.raises(RuntimeError, match="the batch shape of another step"):
        ts.check_selection_flag()
    assert ts.state.read().tick == 2
    with pytest.raises(ValueError, match="the sampler draws from pools of 8 and 30"):
        ts.step_sampled(Sampler(8, N_UNLABEL, BATCH, UNLABEL_BATCH), 3)
    ts.model.eval()
    with pytest.raises(RuntimeError, match="train mode"):
        ts.step_sampled(s, 3)


# ---- 2. fit against the hand-written loop
def hand_loop(name, epochs, eval_batch, mode, patience):
    """The loop a caller writes today: step() on the mirror's selection, valid(), two .item()s, the host rule, a clone of
    the state_dict on every improvement and a load at the end.  Returns (steps, track, model)."""
    from grand_plus_amd import valid
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.fit import early_stop_rule, new_track
    ts, m, _o = train_step(name, False)
    s = sampler()
    rm, X, labels = resident()
    idx_val = pools()[2]
    track, saved, steps = new_track(), None, 0
    for t in range(1, epochs * s.n_batches + 1):
        ts.step(*s.selection(t, step_seed(sc.BASE_SEED, t)))
        steps += 1
        if (t - 1) % eval_batch == 0:
            loss, acc = valid(m, rm, X, idx_val, labels, batch_size=BATCH, dropnode_rate=sc.P_NODE)
            early_stop_rule(track, loss.item(), acc.item(), t, mode, patience)
            if track["copy_now"]:
                saved = {k: v.clone() for k, v in m.state_dict().items()}
            if track["stopped"]:
                break
    if saved is not None:
        m.load_state_dict(saved)
    return steps, track, m


CONFIGS = [("plain", 2, "both", 2), ("bn", 2, "acc", 1), ("bn", 3, "both", 100), ("plain", 1, "acc", 100), ("bn", 1, "both", 3)]
LATER_BEST = CONFIGS[3]           # ties in accuracy count under `acc`: the hand-written loop's best is step 7 there, not step 1
EPOCHS = 8


@functools.lru_cache(maxsize=None)
def hand(name, eval_batch, mode, patience):
    return hand_loop(name, EPOCHS, eval_batch, mode, patience)


@pytest.mark.parametrize("name,eval_batch,mode,patience", CONFIGS)
@pytest.mark.parametrize("poll_every", [1, 4])
def test_fit_is_the_hand_written_loop(name, eval_batch, mode, patience, poll_every):
    import grand_plus_amd
    steps, track, hm = hand(name, eval_batch, mode, patience)
    if (name, eval_batch, mode, patience) == LATER_BEST:             # a precondition of the case, read off the hand-written loop
        assert track["best_tick"] > 1, "this case is here to restore a snapshot taken after earlier ones"
    ts, m, _o = train_step(name, True)
    res = grand_plus_amd.fit(ts, sampler(), pools()[2], epochs=EPOCHS, eval_batch=eval_batch, stop_mode=mode, patience=patience,
                             poll_every=poll_every)
    print(f"{name} eval_batch={eval_batch} {mode} patience={patience} poll_every={poll_every}: hand {steps} steps, "
          f"best {track['best_tick']}, stop {track['stop_tick']}; fit {res}")
    assert res.best_tick == (track["best_tick"] or None)
    assert res.stop_tick == (track["stop_tick"] if track["stopped"] else None)
    assert np.float32(res.best_loss).view(np.int32) == np.float32(track["best_loss"]).view(np.int32)
    assert np.float32(res.best_acc).view(np.int32) == np.float32(track["best_acc"]).view(np.int32)
    if poll_every == 1:
        assert res.steps == steps                                    # the reference's step
    else:
        assert steps <= res.steps <= min(steps + poll_every * eval_batch, EPOCHS * 3)
    assert _same_state(m, hm), "the restored state_dict differs from the hand-written loop's"
    assert m.training and ts.state.read().tick == res.steps
    if patience == 100:
        assert res.stop_tick is None and res.steps == EPOCHS * 3
    else:
        assert res.best_tick is not None


# ---- 3. the steady state does not synchronise
def test_the_steady_state_loop_does_not_synchronise():
    import grand_plus_amd
    from grand_plus_amd.fit import FitLoop
    ts, m, _o = train_step("bn", True)
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
    # fit itself, polling never: it ends at max_steps and reads the tracker once, at the end
    ts2, _m2, _o2 = train_step("plain", True)
    res = grand_plus_amd.fit(ts2, sampler(), pools()[2], epochs=100, eval_batch=2, patience=10 ** 6, poll_every=10 ** 6, max_steps=12)
    assert res.steps == 12 and res.stop_tick is None and ts2.state.read().tick == 12
