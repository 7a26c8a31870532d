"""gp_fit_track_update and gp_fit_snapshot on the GPU: the device applies the early-stop rule that
tests/test_host_fit.py holds to the reference, field for field on scripted sequences, and the snapshot is bitwise the
source as of the best tick, inside its destinations, and untouched when the rule did not ask for a copy."""
import ctypes

import numpy as np
import pytest
import torch

import fit_cases as fc
import step_cases as sc

pytestmark = pytest.mark.gpu

GUARD, MARK = 256, 0x5A5A5A5A


def _val(loss, acc):
    return torch.tensor([loss, acc], dtype=torch.float32, device="cuda")


def _tracker(mode, patience, model=None):
    from grand_plus_amd import BestTracker
    return BestTracker(model if model is not None else torch.nn.Linear(3, 2).cuda(), "cuda", mode, patience)


# ---- 1. the rule
@pytest.mark.parametrize("name,mode,patience", fc.RULE_CASES)
def test_the_device_applies_the_host_rule_field_for_field(name, mode, patience):
    """Ties in accuracy, a better accuracy with a worse loss, NaN loss and NaN accuracy, both modes, patience 1 and 3; three
    further, better results after the sequence, which a stopped track ignores and a running one takes."""
    from grand_plus_amd import StepState
    from grand_plus_amd.fit import new_track
    images, _copies = fc.run_rule(fc.SCRIPTS[name], mode, patience, extra=3)
    tr = _tracker(mode, patience)
    st = StepState("cuda", 1, 0.0, 1.0)
    assert fc.bits(tr.read()) == fc.bits(new_track())
    for want, (loss, acc) in zip(images, list(fc.SCRIPTS[name]) + [fc.EXTRA] * 3):
        st.advance()
        v = _val(loss, acc)
        tr.update(v[0], v[1], st)
        assert fc.bits(tr.read()) == fc.bits(want), (name, mode, patience, want["n_evals"])
    assert tr.read().n_evals <= len(images) and st.read().tick == len(images)


def test_loss_and_acc_may_live_apart_and_the_tick_is_the_states():
    from grand_plus_amd import StepState
    tr = _tracker("both", 2)
    st = StepState("cuda", 1, 0.0, 1.0)
    st.set_tick(40)
    st.advance()
    loss, acc = torch.tensor(0.5, device="cuda"), torch.tensor([0.25], device="cuda")
    tr.update(loss, acc, st)
    got = tr.read()
    assert (got.best_loss, got.best_acc, got.best_tick, got.copy_now, got.n_evals) == (np.float32(0.5), np.float32(0.25), 41, 1, 1)
    st.advance()
    tr.update(torch.tensor(0.6, device="cuda"), torch.tensor(0.1, device="cuda"), st)
    st.advance()
    tr.update(torch.tensor(0.6, device="cuda"), torch.tensor(0.1, device="cuda"), st)
    got = tr.read()
    assert (got.best_tick, got.stop_tick, got.stopped, got.bad_counter, got.copy_now) == (41, 43, 1, 2, 0)
    with pytest.raises(TypeError, match="float32 tensor of one element"):
        tr.update(torch.tensor(0.5, device="cuda", dtype=torch.float64), acc, st)
    with pytest.raises(TypeError, match="float32 tensor of one element"):
        tr.update(loss, torch.tensor(0.5), st)


# ---- 2. the snapshot, through the entry point: 33 tensors, so two launches
WORDS = [0, 1, 4095, 4096, 4097]


class Arena:
    """33 sources and 33 guarded destinations in two int32 arenas; source 7 is an int64 tensor of 2049 elements."""

    def __init__(self):
        from grand_plus_amd._native import GpFitCopy
        self.words = [WORDS[i % len(WORDS)] for i in range(33)]
        self.words[7] = 2 * 2049
        self.src_at = np.concatenate([[0], np.cumsum(self.words)]).astype(np.int64)
        self.dst_at = np.array([GUARD + i * GUARD + int(self.src_at[i]) for i in range(33)], dtype=np.int64)
        self.src = torch.zeros(int(self.src_at[-1]), dtype=torch.int32, device="cuda")
        self.dst = torch.full((int(self.dst_at[-1]) + self.words[-1] + GUARD,), MARK, dtype=torch.int32, device="cuda")
        self.long = self.src[int(self.src_at[7]):int(self.src_at[8])].view(torch.int64)
        assert self.long.numel() == 2049 and self.long.dtype == torch.int64
        self.table = (GpFitCopy * 33)(*[GpFitCopy(src=self.src.data_ptr() + 4 * int(self.src_at[i]),
                                                  dst=self.dst.data_ptr() + 4 * int(self.dst_at[i]), n_words=self.words[i])
                                        for i in range(33)])
        self.round = 0

    def overwrite(self):
        self.round += 1
        gen = torch.Generator(device="cuda").manual_seed(100 + self.round)
        self.src.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, self.src.shape, generator=gen, device="cuda", dtype=torch.int64).to(torch.int32))
        self.long.copy_(torch.randint(-2 ** 62, 2 ** 62, (2049,), generator=gen, device="cuda", dtype=torch.int64))
        return self.src.cpu().numpy().copy()

    def snapshot(self, track_buf):
        from grand_plus_amd import _native
        rc = _native.lib().gp_fit_snapshot(0, track_buf.data_ptr(), self.table, 33, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        _native.raise_for_status(rc)

    def check(self, want):
        """Every destination equals its slice of `want` (None: still the mark) and every word between them is the mark."""
        got = self.dst.cpu().numpy()
        expect = np.full_like(got, np.int32(MARK))
        if want is not None:
            for i in range(33):
                expect[self.dst_at[i]:self.dst_at[i] + self.words[i]] = want[self.src_at[i]:self.src_at[i + 1]]
        assert np.array_equal(got, expect)


def test_the_snapshot_is_bitwise_the_source_as_of_the_best_tick():
    from grand_plus_amd import StepState
    a = Arena()
    tr = _tracker("both", 1)
    st = StepState("cuda", 1, 0.0, 1.0)

    def evaluate(loss, acc):
        st.advance()
        v = _val(loss, acc)
        tr.update(v[0], v[1], st)          # (the tracker's own table covers its dummy model; the arena's is launched here)
        a.snapshot(tr.buf)
        return tr.read()

    v0 = a.overwrite()
    a.snapshot(tr.buf)                      # nothing evaluated yet: copy_now == 0
    a.check(None)
    assert evaluate(1.0, 0.5).copy_now == 1
    a.check(v0)
    a.overwrite()
    assert evaluate(0.9, 0.5).copy_now == 1                                      # a tie in accuracy with a better loss
    v1 = a.src.cpu().numpy().copy()
    a.check(v1)
    a.overwrite()
    got = evaluate(1.5, 0.9)                                                     # the gap: neither taken nor counted
    assert (got.copy_now, got.best_tick, got.bad_counter, got.stopped) == (0, 2, 0, 0)
    a.check(v1)
    v3 = a.overwrite()
    assert evaluate(0.8, 0.9).best_tick == 4
    a.check(v3)
    assert np.array_equal(a.long.cpu().numpy(), v3[a.src_at[7]:a.src_at[8]].view(np.int64))
    a.overwrite()
    got = evaluate(0.7, 0.1)                                                     # worse: patience 1 stops the run
    assert (got.copy_now, got.stopped, got.stop_tick, got.best_tick) == (0, 1, 5, 4)
    a.check(v3)
    a.overwrite()
    got = evaluate(0.0, 1.0)                                                     # better than the best, after the stop
    assert (got.copy_now, got.stopped, got.stop_tick, got.best_tick, got.n_evals) == (0, 1, 5, 4, 5)
    a.check(v3)


# ---- 3. the tracker over a model with BatchNorm: parameters, running statistics and the int64 counter
def test_the_tracker_snapshots_and_restores_a_whole_state_dict():
    from grand_plus_amd import StepState
    m = sc.model("reddit")
    tr = _tracker("acc", 3, m)
    names = list(m.state_dict())
    assert len(tr.tensors) == len(names) and any(t.dtype == torch.int64 for t in tr.tensors)
    assert any("running_mean" in n for n in names) and any("num_batches_tracked" in n for n in names)
    st = StepState("cuda", 1, 0.0, 1.0)

    def scramble(k):
        with torch.no_grad():
            for t in m.state_dict().values():
                t.copy_((torch.arange(t.numel(), device="cuda").reshape(t.shape) * k + k).to(t.dtype))
        return {n: t.clone() for n, t in m.state_dict().items()}

    first = scramble(1)
    assert tr.restore().best_tick == 0                                           # no best yet: restore leaves the model alone
    assert all(torch.equal(t, first[n]) for n, t in m.state_dict().items())
    st.advance()
    v = _val(1.0, 0.5)
    tr.update(v[0], v[1], st)
    scramble(2)
    st.advance()
    v = _val(0.5, 0.4)
    tr.update(v[0], v[1], st)                                                    # worse accuracy: the snapshot stays the first
    third = scramble(3)
    assert all(torch.equal(s, first[n]) for n, s in zip(names, tr.snapshot))
    assert all(torch.equal(t, third[n]) for n, t in m.state_dict().items())
    image = tr.restore()
    assert (image.best_tick, image.n_evals, image.bad_counter) == (1, 2, 1)
    for n, t in m.state_dict().items():
        assert t.dtype == first[n].dtype and torch.equal(t, first[n]), n
