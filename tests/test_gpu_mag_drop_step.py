"""MAG's captured training step with input dropout on the GPU (grand_plus_amd/mag_step.py) in the world of
tests/test_gpu_mag_step.py: V = 50, H = 8, N = 40, K = 4, S = 2, batches of 3 + 4, a MagMLP with input_droprate = 0.5 and
MagTrainStep(input_dropout=True).

The front end reads the step state's seed from device memory, so a replayed step draws the input-dropout mask of its own
tick.  In deterministic mode the contract is bitwise: a replayed step equals the eager step of the same body in every
parameter, Adam tensor and result, with every table step and with chunked segment sums, and `fit` equals the host-driven
loop.  The atomic mode shares the forward; its parameters are held to the 2 * lr rule of tests/test_gpu_mag_step.py."""
import numpy as np
import pytest
import torch

import mag_cases as mc
import step_cases as sc
import test_gpu_mag_step as base
from test_gpu_mag_step import BASE_SEED, BATCH, C, H, K, LR, N, N_TRAIN, N_UNLABEL, S, S_ROWS, UNLABEL_BATCH, V, _assert_twins, _same, selection, world

pytestmark = pytest.mark.gpu

P_IN = 0.5


def mag_step(capture, deterministic, p_in=P_IN, weight_decay=5e-4, **kw):
    """(MagTrainStep, model, optimizer) over test_gpu_mag_step.py's problem, from the same initial state every time."""
    import optim_cases as oc
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels, _longest = world()
    row = torch.from_numpy(np.repeat(seeds, K).astype(np.int32))
    rm = RowMatrix(seeds, K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), N)
    torch.manual_seed(7)
    m = MagMLP(V, C, H, 2, True, p_in, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=weight_decay, clip_norm=0.1, capturable=True,
                   state=StepState("cuda"))
    ts = MagTrainStep(m, opt, rm, *(a.cuda() for a in attrs), labels.cuda(), seeds[:N_TRAIN], seeds[N_TRAIN:], samples=S,
                      dropnode_rate=base.P_NODE, lam=base.LAM, warmup=base.WARMUP, tem=base.TEM, conf=base.CONF, kind="l2", seed=BASE_SEED,
                      capture=capture, deterministic=deterministic, **kw)
    return ts, m, opt


def _front_of_the_last_step(ts, m, sel, other_tick=None):
    """The front end's output for the batch of the step that has just run, from the state as that step left it (its tick's
    seed, its DropNode mask), the int-seed call of that seed (or of other_tick's), and mag_cases.emulate's float32 walk of the
    same call with the seed on the host."""
    from grand_plus_amd._common import step_seed
    _seeds, col, val, filled, (indptr, indices, data), _labels, longest = world()
    pos = ts._pos.index_select(0, torch.from_numpy(np.concatenate([sel[0], sel[1] + N_TRAIN])).cuda())
    with torch.no_grad():
        X = ts._front(pos).clone()
    t = int(ts.state.read().tick)
    assert ts.state.read().seed == step_seed(BASE_SEED, t)
    P = mc.Problem(W=m.embeds.weight.detach().cpu(), indptr=indptr, indices=indices, data=data, col=col.reshape(S_ROWS, K),
                   val=val.reshape(S_ROWS, K), filled=filled, K=K, N=N, V=V, H=H, S_rows=S_ROWS, longest=longest)
    keep = ts._node_keep.cpu()
    walk = mc.emulate(P, pos.cpu(), S, base.P_NODE, P_IN, True, keep, step_seed(BASE_SEED, t))
    Pa = mc.Problem(**dict(P.__dict__, W=P.W.abs()))
    terms = mc.emulate(Pa, pos.cpu(), S, base.P_NODE, P_IN, True, keep, step_seed(BASE_SEED, t))
    from grand_plus_amd import mag_prop_rows
    eager = mag_prop_rows(m.embeds.weight.detach(), *ts.attr, ts.rows.col, ts.rows.val, ts.rows.filled, K, pos, samples=S,
                          dropnode_rate=base.P_NODE, input_droprate=P_IN, training=True, seed=step_seed(BASE_SEED, other_tick or t), keep=ts._node_keep)
    return X, eager, walk, terms, K + longest + S + 8


# ---- deterministic mode
def test_three_replayed_steps_equal_three_eager_steps_bit_for_bit_and_each_tick_draws_its_mask():
    cap, cm, co = mag_step(True, True, input_dropout=True)
    eag, em, eo = mag_step(False, True, input_dropout=True)
    assert cap.input_dropout and cap.deterministic and float(cm.input_droprate) == P_IN
    fronts = []
    for t in range(1, 4):
        sel = selection(t)
        rc, re = cap.step(*sel), eag.step(*sel)
        _assert_twins((rc, cm, co), (re, em, eo), f"step {t}")
        assert np.isfinite(float(rc.loss))
        # the front end at tick t: bit for bit the int-seed call with step_seed(BASE_SEED, t), and mag_cases.emulate's walk of
        # it within twice mag_cases' bound (the kernel and the walk each round inside it)
        X, eager, walk, terms, roundings = _front_of_the_last_step(cap, cm, sel)
        assert _same(X, eager), f"step {t}: the front end is not the int-seed call of the tick's seed"
        ratio = float(((X.double().cpu() - walk.double()).abs() / (2 * mc.bound(terms, roundings))).max())
        print(f"[mag drop step] tick {t}: front end against the float32 walk, error / bound {ratio:.3g}")
        assert ratio <= 1.0 and bool(X.any())
        fronts.append((X, sel))
    assert not _same(fronts[0][0], fronts[1][0])
    assert cap.state.read().tick == eag.state.read().tick == 3
    assert len(cap._shapes) == 1 and cap._shapes[(7, 3)] is not None and not eag._shapes
    # the same batch at another tick has another input-dropout mask: run tick 1's batch again at tick 4
    sel = fronts[0][1]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                      # a fourth step, a replay, waits for nothing
    try:
        rc = tuple(x.clone() for x in cap.step(*sel))
    finally:
        torch.cuda.set_sync_debug_mode(0)
    re = eag.step(*sel)
    for name, x, y in zip(re._fields, rc, re):
        assert _same(x, y), f"step 4: {name} differs"
    _assert_twins((re, cm, co), (re, em, eo), "step 4")
    X4, eager4, _walk, _terms, _r = _front_of_the_last_step(cap, cm, sel)
    _X4, as_tick1, _walk, _terms, _r = _front_of_the_last_step(cap, cm, sel, other_tick=1)
    assert _same(X4, eager4) and not _same(X4, as_tick1)                         # same weights, same DropNode mask: the seed alone differs
    for ts in (cap, eag):
        ts.check_entries_flag()


@pytest.mark.parametrize("mode", [dict(table_step="exact"), dict(table_step="lazy"), dict(segment_chunk=64),
                                  dict(table_step="lazy", dirty_rows=True, segment_chunk=64)],
                         ids=["exact", "lazy", "chunk64", "lazy-dirty-chunk64"])
def test_each_table_step_and_the_chunked_sums_replay_as_their_eager_twin(mode):
    wd = 0.0 if mode.get("table_step") == "lazy" else 5e-4
    cap, cm, co = mag_step(True, True, weight_decay=wd, input_dropout=True, **mode)
    eag, em, eo = mag_step(False, True, weight_decay=wd, input_dropout=True, **mode)
    w0 = cm.embeds.weight.detach().clone()
    for t in range(1, 5):                                                        # eager, captured, two replays
        sel = selection(t)
        _assert_twins((cap.step(*sel), cm, co), (eag.step(*sel), em, eo), f"{mode}, step {t}")
    assert cap._shapes[(7, 3)] is not None and not torch.equal(w0, cm.embeds.weight)
    cap.check_entries_flag()


# ---- atomic mode
@pytest.mark.parametrize("mode", [dict(), dict(table_step="lazy", row_list="bitmap"), dict(table_step="exact", row_list="bitmap")],
                         ids=["dense", "lazy-bitmap", "exact-bitmap"])
def test_the_atomic_step_shares_the_forward_and_its_replay_runs(mode):
    wd = 0.0 if mode.get("table_step") == "lazy" else 5e-4
    det, dm, do = mag_step(False, True, weight_decay=wd, input_dropout=True, **({"table_step": mode["table_step"]} if mode else {}))
    ato, am, ao = mag_step(True, False, weight_decay=wd, input_dropout=True, **mode)
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


# ---- a model without input dropout
@pytest.mark.parametrize("deterministic", [True, False])
def test_the_keyword_on_a_model_at_rate_zero_is_the_step_without_it(deterministic):
    """Bit for bit in the deterministic mode; in the atomic mode the forward (the first step's results) bit for bit."""
    new, nm, no = mag_step(True, deterministic, p_in=0.0, input_dropout=True)
    old, om, oo = mag_step(True, deterministic, p_in=0.0)
    assert new.input_dropout is False and old.input_dropout is False
    for t in range(1, 5):
        sel = selection(t)
        a, b = new.step(*sel), old.step(*sel)
        if deterministic:
            _assert_twins((a, nm, no), (b, om, oo), f"step {t}")
        elif t == 1:
            for name in ("sup", "con", "loss", "n_conf", "n_correct"):
                assert _same(getattr(a, name), getattr(b, name)), name
    with pytest.raises(ValueError, match=r"input_droprate = 0.*DESIGN §9"):
        mag_step(True, True, p_in=0.5)


# ---- fit
def test_fit_over_the_lazy_dirty_step_is_the_host_driven_loop():
    """Twenty steps with a validation every five (steps 1, 6, 11, 16), as tests/test_gpu_mag_fit.py holds `fit` to the
    hand-written loop: step() on the sampler's mirror selection, valid_mag, the host rule, a clone on every improvement."""
    import grand_plus_amd
    from grand_plus_amd import Sampler, valid_mag
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.fit import early_stop_rule, new_track
    mode = dict(table_step="lazy", dirty_rows=True)
    seeds = world()[0]
    idx_val = seeds[N_TRAIN + 1:N_TRAIN + 7]                                      # six seed rows stand in as the validation set
    s = Sampler(N_TRAIN, N_UNLABEL, BATCH, UNLABEL_BATCH, 11)
    hand, hm, _ho = mag_step(False, True, weight_decay=0.0, input_dropout=True, table_step="lazy")
    track, saved, steps = new_track(), None, 0
    for t in range(1, 21):
        hand.step(*s.selection(t, step_seed(BASE_SEED, t)))
        steps += 1
        if (t - 1) % 5 == 0:
            loss, acc = valid_mag(hm, hand.rows, *hand.attr, idx_val, hand.labels, batch_size=100, dropnode_rate=base.P_NODE)
            early_stop_rule(track, loss.item(), acc.item(), t, "both", 100)
            if track["copy_now"]:
                saved = {k: v.clone() for k, v in hm.state_dict().items()}
    assert saved is not None and track["n_evals"] == 4
    hm.load_state_dict(saved)
    ts, m, _o = mag_step(True, True, weight_decay=0.0, input_dropout=True, **mode)
    assert ts.row_grad.dirty is not None
    res = grand_plus_amd.fit(ts, s, idx_val, epochs=7, eval_batch=5, stop_mode="both", patience=100, max_steps=20)
    print(f"[mag drop step] fit {res}; hand best {track['best_tick']}")
    assert res.steps == steps == 20 and res.stop_tick is None and res.best_tick == track["best_tick"]
    assert np.float32(res.best_loss).view(np.int32) == np.float32(track["best_loss"]).view(np.int32)
    assert np.float32(res.best_acc).view(np.int32) == np.float32(track["best_acc"]).view(np.int32)
    sa, sb = m.state_dict(), hm.state_dict()
    assert list(sa) == list(sb) and all(_same(sa[k], sb[k]) for k in sa), "the restored state_dict differs from the hand-written loop's"
    assert m.training and ts.state.read().tick == 20
    ts.check_entries_flag()
    ts.check_selection_flag()
