"""The deferred exact Adam step of MAG's embedding table on the GPU.  There are no tolerances, and the yardstick
is parent code, never the new kernels.  Kernel level: gp_optim_defer_catch_up / _step / _flush over the scenarios of
tests/optim_defer_cases.py against the DENSE TWIN -- gp_clip_adam_rows_dev in exact mode on a clone, fed the same lists and
gradients -- bit for bit after every flush and, row by row, after every catch-up; `last` and the flag word against the numpy
mirror of the bookkeeping.  Step level: MagTrainStep(table_step="deferred") against table_step="exact", and `fit` over both."""
import copy
import functools

import numpy as np
import pytest
import torch

import optim_defer_cases as dc
import optim_rows_cases as rc
from test_gpu_optim_rows import _Buf, _workspace

pytestmark = pytest.mark.gpu

GUARD = 64
MARK = -77


class _Ints:
    """An int32 device buffer of n elements holding `value` between two guard bands."""

    def __init__(self, n, value):
        self.full = torch.full((n + 2 * GUARD,), MARK, dtype=torch.int32, device="cuda")
        self.view = self.full[GUARD:GUARD + n]
        self.view.fill_(value)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        full = self.full.cpu().numpy()
        assert (full[:GUARD] == MARK).all() and (full[-GUARD:] == MARK).all(), "a guard band was written"
        return full[GUARD:-GUARD].copy()


def _equal(a, b, nan_aware):
    """Bit for bit; nan_aware (the poisoned run): NaN in the same places and equal bits everywhere else."""
    if not nan_aware:
        return rc.same_bits(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and rc.same_bits(np.where(na, np.float32(0), a), np.where(nb, np.float32(0), b))


class _Run:
    """One table under the deferred kernels beside its dense twin, and the mirror of the books."""

    def __init__(self, V, H, capacity, max_norm, weight_decay, seed=3):
        from grand_plus_amd import _native
        self.L, self.V, self.H, self.capacity = _native.lib(), V, H, capacity
        self.max_norm, self.wd = float(max_norm), float(weight_decay)
        state = rc.state(V, H, seed)
        self.deferred = [_Buf(x) for x in state]
        self.twin = [_Buf(x) for x in state]
        self.last, self.hist = _Ints(V, 0), _Ints(capacity * 4, 0)
        self.flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.tick = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.corr = torch.zeros(2, dtype=torch.float32, device="cuda")
        self.norms = [_Buf(np.zeros(1, np.float32)), _Buf(np.zeros(1, np.float32))]
        self.ws_full, self.ws = _workspace()
        self.stream = torch.cuda.current_stream().cuda_stream
        self.book = dc.Book(V, capacity)
        self.keep = []                                                           # the device tensors of launches in flight

    def table(self, which):
        return tuple(b.get() for b in which)

    def _state(self):
        return (self.tick.data_ptr(), self.last.ptr(), self.hist.ptr(), self.capacity, self.flag.data_ptr())

    def _constants(self):
        return (dc.BETAS[0], dc.BETAS[1], dc.EPS, self.wd)

    def _keys(self, keys):
        k = torch.from_numpy(np.concatenate([[-99], keys, [-99]]).astype(np.int64)).cuda()   # a list of 0 keys still has an address
        self.keep.append(k)
        return k.data_ptr() + 8

    def begin(self, T):
        self.tick.fill_(T)
        self.corr.copy_(torch.tensor(rc.corrections(dc.LR, dc.BETAS, T), dtype=torch.float32))

    def catch_up(self, keys):
        from grand_plus_amd import _native
        rcode = self.L.gp_optim_defer_catch_up(0, *(b.ptr() for b in self.deferred), self._keys(keys), len(keys), self.V, self.H,
                                               *self._constants(), *self._state(), self.stream)
        _native.raise_for_status(rcode)

    def step(self, keys, dW):
        """The norm of (keys, dW) once, then the twin's exact step and the deferred step from the same workspace."""
        from grand_plus_amd import _native
        from grand_plus_amd import optim_rows as orows
        g = torch.from_numpy(dW).cuda()
        self.keep.append(g)
        kp, n, c = self._keys(keys), len(keys), self.corr.data_ptr()
        _native.raise_for_status(self.L.gp_optim_rows_sqnorm(0, kp, n, self.V, self.H, g.data_ptr(), 0, self.ws.data_ptr(), self.stream))
        hyper = (self.max_norm, dc.LR, *self._constants())
        rcode = self.L.gp_clip_adam_rows_dev(0, *(b.ptr() for b in self.twin), g.data_ptr(), kp, n, self.V, self.H, orows.MODES["exact"],
                                             *hyper, c, c + 4, self.ws.data_ptr(), self.norms[0].ptr(), self.stream)
        _native.raise_for_status(rcode)
        rcode = self.L.gp_optim_defer_step(0, *(b.ptr() for b in self.deferred), g.data_ptr(), kp, n, self.V, self.H, *hyper, c, c + 4,
                                           *self._state(), self.ws.data_ptr(), self.norms[1].ptr(), self.stream)
        _native.raise_for_status(rcode)

    def flush(self):
        from grand_plus_amd import _native
        rcode = self.L.gp_optim_defer_flush(0, *(b.ptr() for b in self.deferred), self.V, self.H, *self._constants(), *self._state(),
                                            self.stream)
        _native.raise_for_status(rcode)

    def check_books(self, what):
        torch.cuda.synchronize()
        self.keep.clear()
        assert self.last.get().tolist() == self.book.last.tolist(), f"{what}: last is not the mirror's"
        assert int(self.flag.item()) == self.book.flag, f"{what}: the flag word is {int(self.flag.item())}, the mirror's {self.book.flag}"
        self.hist.get()


def _drive(sc, H, kind, max_norm, weight_decay, pre_forward=True, poison_at=None, tamper=None):
    """The scenario through the kernels, the twin and the mirror; every check of the module's docstring on the way.  Rows the
    mirror says are unserved must keep their bits; every other comparison is to the twin.  tamper=(t, step, tag): after step t
    the tag of the ring slot of `step` is overwritten.  Returns the _Run and the twin's norm of every step."""
    run = _Run(sc.V, H, sc.capacity, max_norm, weight_decay)
    nan_aware, norms = poison_at is not None, []
    for T in range(1, sc.n_steps + 1):
        rows = sc.touches[T]
        keys = dc.key_list(rows, sc.V, kind, T)
        run.begin(T)
        if pre_forward:
            before, twin = run.table(run.deferred), run.table(run.twin)
            behind = run.book.last.copy()
            run.catch_up(keys)
            run.book.catch_up(T, rows)
            run.check_books(f"catch-up {T}")
            after = run.table(run.deferred)
            served = np.zeros(sc.V, bool)
            served[rows] = run.book.last[rows] >= T - 1
            for name, a, b, t in zip("pmv", after, before, twin):
                assert _equal(a[served], t[served], nan_aware), f"catch-up {T}: a listed row of {name} is not the twin's of step {T - 1}"
                assert rc.same_bits(a[~served], b[~served]), f"catch-up {T}: a row of {name} that was not served changed"
            lagged = served & (behind < T - 1)
            if lagged.any() and not nan_aware:
                assert not rc.same_bits(after[0][lagged], before[0][lagged]), f"catch-up {T}: the rows that lagged did not move"
        dW = dc.gradient(keys, sc.V, H, T, poisoned=poison_at == T)
        before = run.table(run.deferred)
        run.step(keys, dW)
        run.book.step(T, rows)
        run.check_books(f"step {T}")
        assert rc.same_bits(run.norms[0].get(), run.norms[1].get()), f"step {T}: the norm differs from the twin's"
        norms.append(float(run.norms[0].get()[0]))
        after, twin = run.table(run.deferred), run.table(run.twin)
        stepped = run.book.last == T
        for name, a, b, t in zip("pmv", after, before, twin):
            assert _equal(a[stepped], t[stepped], nan_aware), f"step {T}: a touched row of {name} is not the twin's"
            assert rc.same_bits(a[~stepped], b[~stepped]), f"step {T}: an untouched row of {name} changed"
        if tamper and tamper[0] == T:
            slot = tamper[1] % sc.capacity
            run.hist.view[4 * slot + 3] = tamper[2]
            run.book.tags[slot] = tamper[2]
        if T in sc.flush_after:
            before = after
            run.flush()
            run.book.flush(T)
            run.check_books(f"flush {T}")
            after = run.table(run.deferred)
            current = run.book.last == T
            for name, a, b, t in zip("pmv", after, before, twin):
                assert _equal(a[current], t[current], nan_aware), f"flush {T}: {name} is not the twin's"
                assert rc.same_bits(a[~current], b[~current]), f"flush {T}: an unserved row of {name} changed"
            run.flush()                                                          # a second flush changes no bit
            run.check_books(f"second flush {T}")
            for name, a, b in zip("pmv", run.table(run.deferred), after):
                assert rc.same_bits(a, b), f"flush {T}: the second flush changed {name}"
    return run, norms


# ---- 1. kernel level
@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("H", dc.HS)
def test_every_flush_and_every_catch_up_is_the_dense_twin_bit_for_bit(H, kind):
    """V = 97, capacity 8, 24 steps: a row touched at every step, one never, gaps of 1, 2, capacity - 1 and capacity, an empty
    list, sentinel tails, both list kinds; clipping on (coef below 1 at some steps, 1 at others) and off, weight decay 0 and 1e-3."""
    sc = dc.main()
    for max_norm, wd in dc.SETTINGS:
        run, norms = _drive(sc, H, kind, max_norm, wd)
        assert run.book.flag == 0 and (run.book.last == sc.n_steps).all()
        assert all(a == list(range(1, sc.n_steps + 1)) for a in run.book.applied)
        if max_norm > 0:
            assert any(n > 2 * max_norm for n in norms) and any(0 < n < max_norm / 2 for n in norms), norms
        p, _m, _v = run.table(run.deferred)
        assert np.isfinite(p).all() and not rc.same_bits(p, rc.state(sc.V, H, 3)[0])


@pytest.mark.parametrize("kind", dc.KINDS)
@pytest.mark.parametrize("H", [3, 68])
def test_the_step_catches_up_inline_when_the_pre_forward_call_is_skipped(H, kind):
    sc = dc.main()
    for max_norm, wd in dc.SETTINGS[1:]:
        with_call, _ = _drive(sc, H, kind, max_norm, wd)
        without, _ = _drive(sc, H, kind, max_norm, wd, pre_forward=False)
        assert without.book.flag == 0
        for name, a, b in zip("pmv", without.table(without.deferred), with_call.table(with_call.deferred)):
            assert rc.same_bits(a, b), f"{name} differs with and without the pre-forward call"


@pytest.mark.parametrize("H", [8, 68])
def test_a_poisoned_step_poisons_what_it_poisons_in_the_twin(H):
    """A NaN gradient at step 3 makes the clip coefficient NaN and with it the twin's whole table.  After every flush the
    deferred table has NaN in the same places and equal bits elsewhere."""
    sc = dc.main()
    run, norms = _drive(sc, H, "det", 0.5, 1e-3, poison_at=3)
    assert np.isnan(norms[2]) and np.isfinite(norms[1]) and run.book.flag == 0
    assert all(np.isnan(x).all() for x in run.table(run.twin)[:1]) and all(np.isnan(x).all() for x in run.table(run.deferred)[:1])
    # with clipping off only the touched row's column is poisoned: the rest of the table stays on the trajectory
    run, _ = _drive(sc, H, "bitmap", 0.0, 1e-3, poison_at=3)
    p = run.table(run.deferred)[0]
    assert np.isnan(p).any() and not np.isnan(p).all()


@pytest.mark.parametrize("kind", dc.KINDS)
def test_one_step_past_the_served_gap_is_a_flag_and_a_row_left_alone(kind):
    """Row 1 is touched when it is capacity (served) or capacity + 1 (not served) steps behind.  Unserved: the flag bit is set,
    the row's p, m, v and last keep their bits through the catch-up, the step and the flush, and every other row is served.
    An error code path, not a fault."""
    served, _ = _drive(dc.past_the_gap(0), 8, kind, 0.5, 1e-3)
    assert served.book.flag == 0 and (served.book.last == dc.CAPACITY + 1).all()
    sc = dc.past_the_gap(1)
    for pre_forward in (True, False):
        run, _ = _drive(sc, 8, kind, 0.5, 1e-3, pre_forward=pre_forward)
        T = dc.CAPACITY + 2
        assert int(run.flag.item()) == dc.FLAG_BIT and run.last.get().tolist() == [T if r != 1 else 1 for r in range(sc.V)]
        init = rc.state(sc.V, 8, 3)
        for name, a, t, first in zip("pmv", run.table(run.deferred), run.table(run.twin), init):
            assert rc.same_bits(np.delete(a, 1, 0), np.delete(t, 1, 0)), f"{name}: a served row is not the twin's"
            assert not rc.same_bits(a[1], t[1]) and not rc.same_bits(a[1], first[1])      # it was current through step 1 and stayed there


def test_a_slot_that_does_not_carry_its_steps_tag_is_never_replayed():
    """The tag of step 11's slot is overwritten after step 11: every row whose replay would read it is flagged and left alone,
    the rows touched at step 12 (their replay ends at 11 -- or they were current) go on."""
    sc = dc.main()
    run, _ = _drive(sc, 8, "det", 0.5, 0.0, tamper=(11, 11, 12345))
    assert run.book.flag == dc.FLAG_BIT and int(run.flag.item()) == dc.FLAG_BIT
    last = run.last.get()
    assert (last == sc.n_steps).any() and (last < 11).any() and last[0] == sc.n_steps
    stuck = last < 11
    for name, a, t in zip("pmv", run.table(run.deferred), run.table(run.twin)):
        assert rc.same_bits(a[~stuck], t[~stuck]), name


@pytest.mark.parametrize("kind", dc.KINDS)
def test_replays_that_straddle_the_rings_wrap(kind):
    sc = dc.wrap()
    assert sc.n_steps > 2 * sc.capacity
    for pre_forward in (True, False):
        run, _ = _drive(sc, 64, kind, 0.5, 1e-3, pre_forward=pre_forward)
        assert run.book.flag == 0 and (run.book.last == sc.n_steps).all()


def test_a_table_of_one_row():
    sc = dc.single_row()
    for H in (3, 64):
        run, _ = _drive(sc, H, "bitmap", 0.5, 1e-3)
        assert run.book.flag == 0 and run.book.last.tolist() == [sc.n_steps]


def test_every_capped_grid_goes_round_its_stride_loop_twice():
    """DESIGN §7p's rule at H = 3: more rows than twice the flush's capped grid takes per trip, and a list whose positions
    exceed twice the catch-up's and whose windows exceed twice the step's.  Steps 1, 3 and 5 touch the list, steps 2 and 4 a
    few rows: the catch-up of step 3 replays step 2 on every listed row, and step 5, without the pre-forward call, replays
    step 4 inline; then the flush."""
    H = 3
    Vn = 2 * dc.FLUSH_GRID * dc.WAVES * dc.WINDOW + 5 * dc.WINDOW + 3
    rows = np.arange(1, Vn, 2, dtype=np.int64)
    keys = dc.key_list(rows, Vn, "bitmap")
    assert len(keys) > 2 * dc.STEP_GRID * dc.WAVES * dc.WINDOW and len(keys) > 2 * dc.CATCH_GRID * dc.WAVES
    few = dc.key_list(np.array([0, 5, Vn - 1]), Vn, "det")
    run = _Run(Vn, H, dc.CAPACITY, 0.5, 1e-3)
    rng = np.random.default_rng(5)
    for T, (k, pre_forward) in enumerate([(keys, True), (few, True), (keys, True), (few, True), (keys, False)], 1):
        run.begin(T)
        if pre_forward:
            run.catch_up(k)
        dW = np.full((Vn, H), np.nan, dtype=np.float32)
        touched = rc.touched(k, Vn)
        dW[touched] = rng.standard_normal((int(touched.sum()), H)).astype(np.float32)
        run.step(k, dW)
        torch.cuda.synchronize()
        run.keep.clear()
    last = run.last.get()
    assert (last[1::2] == 5).all() and last[0] == last[-1] == 4 and (last[2:-1:2] == 0).all() and int(run.flag.item()) == 0
    before = run.table(run.deferred)
    run.flush()
    torch.cuda.synchronize()
    assert (run.last.get() == 5).all() and int(run.flag.item()) == 0
    for name, a, b, t in zip("pmv", run.table(run.deferred), before, run.table(run.twin)):
        assert rc.same_bits(a, t), f"{name} is not the twin's after the flush"
        assert rc.same_bits(a[1::2], b[1::2]) and not rc.same_bits(a[2:-1:2], b[2:-1:2])   # the flush moved the rows that lagged, alone


# ---- 2. step level: MagTrainStep(table_step="deferred") against table_step="exact"
STEPS = 12


def _mag_step(capture, table_step, bitmap=False, **kw):
    """tests/test_gpu_mag_table_step.py's step (deterministic, clip_norm = -1, weight decay 5e-4) or, bitmap=True,
    tests/test_gpu_mag_atomic_rows.py's (the atomic backward with row_list="bitmap"), with further keywords of MagTrainStep."""
    import optim_cases as oc
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    import test_gpu_mag_step as g
    seeds, col, val, filled, attrs, labels, _longest = g.world()
    row = torch.from_numpy(np.repeat(seeds, g.K).astype(np.int32))
    rmx = RowMatrix(seeds, g.K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), g.N)
    torch.manual_seed(7)
    m = MagMLP(g.V, g.C, g.H, 2, True, 0.0, 0.5, True).cuda().train()
    opt = ClipAdam(mag_trained_parameters(m), lr=g.LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=5e-4, clip_norm=kw.pop("clip_norm", -1.0),
                   capturable=True, state=StepState("cuda"))
    mode = dict(deterministic=False, row_list="bitmap") if bitmap else dict(deterministic=True)
    ts = MagTrainStep(m, opt, rmx, *(a.cuda() for a in attrs), labels.cuda(), seeds[:g.N_TRAIN], seeds[g.N_TRAIN:], samples=g.S,
                      dropnode_rate=g.P_NODE, lam=g.LAM, warmup=g.WARMUP, tem=g.TEM, conf=g.CONF, kind="l2", seed=g.BASE_SEED,
                      capture=capture, table_step=table_step, **mode, **kw)
    return ts, m, opt


@functools.lru_cache(maxsize=None)
def _exact_run(clip_norm):
    """STEPS eager steps of table_step="exact": the results of every step and the final snapshot, computed once."""
    import step_cases as scs
    from test_gpu_mag_step import selection
    ts, m, opt = _mag_step(False, "exact", clip_norm=clip_norm)
    results = [tuple(x.clone() for x in ts.step(*selection(t))) for t in range(1, STEPS + 1)]
    return results, [x.clone() for x in scs.snapshot(m, opt)]


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("clip_norm,capacity", [(-1.0, None), (0.1, 4)], ids=["default-ring", "clipped-capacity-4"])
def test_twelve_deferred_steps_then_a_flush_are_twelve_exact_steps_bit_for_bit(capture, clip_norm, capacity):
    """The deterministic backward: every result of every step, and after flush_table() the table, both moments and every other
    parameter and Adam tensor.  With defer_capacity = 4 the wrapper's own flush fires, from its host count, twice on the way."""
    import step_cases as scs
    from test_gpu_mag_step import _same, selection
    want_results, want = _exact_run(clip_norm)
    ts, m, opt = _mag_step(capture, "deferred", clip_norm=clip_norm, defer_capacity=capacity)
    assert ts.deferred is opt.deferred_rows(m.embeds.weight) and ts.deferred.capacity == (capacity or 1024)
    flushes, lagging = 0, False
    for t in range(1, STEPS + 1):
        before = ts._since_flush
        r = ts.step(*selection(t))
        flushes += ts._since_flush <= before
        for name, x, y in zip(r._fields, r, want_results[t - 1]):
            assert _same(x, y), f"step {t}: {name} differs from the exact step's"
        lagging = lagging or bool((ts.deferred.last != t).any())
    assert lagging, "no row ever lagged: the steps deferred nothing"
    assert flushes == (0 if capacity is None else 2) and (ts._shapes.get((7, 3)) is not None) == capture
    assert not all(_same(x, y) for x, y in zip(scs.snapshot(m, opt), want)), "the table was current without a flush"
    ts.flush_table()
    assert ts._since_flush == 0 and bool((ts.deferred.last == STEPS).all())
    for i, (x, y) in enumerate(zip(scs.snapshot(m, opt), want)):
        assert _same(x, y), f"tensor {i} of the snapshot differs from the exact step's"
    ts.check_entries_flag()
    assert m.embeds.weight.grad is None


def test_state_dict_returns_a_current_table_and_a_loaded_one_is_current_through_its_tick():
    import step_cases as scs
    from test_gpu_mag_step import _same, selection
    _results, want = _exact_run(-1.0)
    ts, m, opt = _mag_step(True, "deferred")
    for t in range(1, STEPS + 1):
        ts.step(*selection(t))
    assert bool((ts.deferred.last != STEPS).any())
    sd = opt.state_dict()                                                       # flushes first
    assert bool((ts.deferred.last == STEPS).all()) and {s["step"] for s in sd["state"].values()} == {STEPS}
    for i, (x, y) in enumerate(zip(scs.snapshot(m, opt), want)):
        assert _same(x, y), f"tensor {i} of the snapshot differs from the exact step's"
    # a fresh optimiser that loads it: every row is current through the loaded tick, and the next steps are the exact step's
    ex, xm, xo = _mag_step(False, "exact")
    new, nm, no = _mag_step(False, "deferred", defer_capacity=8)
    for model, o in ((xm, xo), (nm, no)):
        model.load_state_dict(m.state_dict())
        o.load_state_dict(copy.deepcopy(sd))                                    # torch may take the checkpoint's tensors over as they are
    assert bool((new.deferred.last == STEPS).all()) and not bool(new.deferred.hist.any())
    for t in range(STEPS + 1, STEPS + 4):
        a, b = new.step(*selection(t)), ex.step(*selection(t))
        assert _same(a.loss, b.loss), f"step {t} after the checkpoint"
    new.flush_table()
    for i, (x, y) in enumerate(zip(scs.snapshot(nm, no), scs.snapshot(xm, xo))):
        assert _same(x, y), f"after the checkpoint: tensor {i} differs"
    new.check_entries_flag()


def test_the_flag_bit_has_its_own_message():
    from test_gpu_mag_step import selection
    ts, _m, _o = _mag_step(False, "deferred", defer_capacity=4)
    ts.step(*selection(1))
    ts.check_entries_flag()
    ts.state.set_tick(7)                                                         # the count moves without a reset: every row is 7 behind
    ts.step(*selection(2))
    with pytest.raises(RuntimeError, match="lagged more than defer_capacity = 4 steps"):
        ts.check_entries_flag()


@pytest.mark.parametrize("capture", [False, True], ids=["eager", "replayed"])
def test_the_deferred_bitmap_step_is_the_dense_kernel_on_its_own_rows_and_within_the_atomic_rule(capture):
    """row_list="bitmap": the atomic gradient is not reproducible, so deferred is held to exact + bitmap by the rule
    tests/test_gpu_mag_step.py holds the atomic mode to (one state, one forward: the first step's losses bit for bit, and the
    parameters after it within 2 lr, LR being that file's).  Beyond it, bit for bit on the step's own gradient: the dense kernel
    (tests/test_gpu_mag_atomic_rows.py's _dense_table_step) run over the rows and keys every step left in its RowGrad, from the
    initial table, is the flushed table after STEPS steps; and the list the backward took over is the list it makes itself."""
    import step_cases as scs
    from test_gpu_mag_atomic_rows import _dense_table_step
    from test_gpu_mag_step import LR, V, H, _same, selection
    from grand_plus_amd.optim_rows import BitmapRowGrad
    ts, m, opt = _mag_step(capture, "deferred", bitmap=True, defer_capacity=8)
    ex, xm, xo = _mag_step(capture, "exact", bitmap=True)
    assert type(ts.row_grad) is BitmapRowGrad
    w = m.embeds.weight
    table = (w.detach().cpu().numpy().copy(), np.zeros((V, H), np.float32), np.zeros((V, H), np.float32))
    for t in range(1, STEPS + 1):
        ts.row_grad.values.fill_(float("nan"))
        a, b = ts.step(*selection(t)), ex.step(*selection(t))
        if t == 1:
            for name in ("sup", "con", "loss", "n_conf", "n_correct"):
                assert _same(getattr(a, name), getattr(b, name)), name            # the forward is shared
            ts.flush_table()
            for i, (x, y) in enumerate(zip(scs.snapshot(m, opt), scs.snapshot(xm, xo))):
                if x.dtype == torch.float32 and i < len(opt.param_groups[0]["params"]):
                    assert float((x - y).abs().max()) <= 2 * LR + 1e-6, f"parameter {i}"
        keys, values = ts.row_grad.keys.cpu().numpy(), ts.row_grad.values.cpu().numpy()
        assert np.array_equal(keys, ex.row_grad.keys.cpu().numpy()), f"step {t}: the list taken over is not the backward's own"
        touched = rc.touched(keys, V)
        assert touched.any() and np.isnan(values[~touched]).all() and np.isfinite(values[touched]).all(), f"step {t}"
        img = ts.state.read()
        table = _dense_table_step(table, rc.dense_gradient(values, keys), (float(img.step_size[0]), float(img.rsqrt_bc2[0])), 5e-4)
        assert ts.row_grad.prelisted is None and not bool(ts.row_grad.bitmap.any()) and not bool(ts.deferred.bitmap.any())
    ts.flush_table()
    got = (w.detach().cpu().numpy(), opt.state[w]["exp_avg"].cpu().numpy(), opt.state[w]["exp_avg_sq"].cpu().numpy())
    for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), got, table):
        assert rc.same_bits(x, y), f"{name} is not the dense kernel's on the step's own rows"
    assert (ts._shapes.get((7, 3)) is not None) == capture
    ts.check_entries_flag()


def test_a_replayed_deferred_step_waits_for_nothing():
    from test_gpu_mag_step import selection
    ts, m, _o = _mag_step(True, "deferred", defer_capacity=4)
    for t in range(1, 4):
        ts.step(*selection(t))
    sels = [selection(t) for t in range(4, 8)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for sel in sels:                                                         # the wrapper's flush fires in here too
            ts.step(*sel)
        ts.flush_table()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert bool(torch.isfinite(m.embeds.weight).all()) and bool((ts.deferred.last == 7).all())


# ---- 3. fit
def _fit(mode, valid_capture, eval_batch=5):
    """`fit` of tests/test_gpu_mag_fit.py's problem as grand_plus_amd.fit runs it; returns the FitResult, the tracker's struct and
    the model."""
    import test_gpu_mag_fit as f
    from grand_plus_amd.fit import FitLoop
    ts, m, _o = f.mag_step(True, **mode)
    loop = FitLoop(ts, f.sampler(), f.pools()[2], eval_batch=eval_batch, stop_mode="both", patience=100, valid_capture=valid_capture)
    while loop.t < f.LAST:
        loop.advance()
    image = loop.tracker.read()
    result = loop.finish()
    ts.check_entries_flag()
    return result, image, m, ts


@pytest.mark.parametrize("valid_capture", [False, True], ids=["eager-valid", "captured-valid"])
def test_fit_over_a_deferred_table_is_fit_over_the_exact_one(valid_capture):
    """Deterministic mode, validation every 5 steps over a ring of 4: the wrapper's own flush and the validation's both fire.
    The same tracker struct, the same best weights bit for bit."""
    import test_gpu_mag_fit as f
    want, want_image, xm, _ = _fit(dict(deterministic=True, table_step="exact"), valid_capture)
    got, image, m, ts = _fit(dict(deterministic=True, table_step="deferred", defer_capacity=4), valid_capture)
    assert image == want_image and got == want and want.best_tick is not None and want.steps == f.LAST
    assert f._same_state(m, xm), "the restored state_dict differs from the exact step's"
    assert bool((ts.deferred.last == f.LAST).all())
