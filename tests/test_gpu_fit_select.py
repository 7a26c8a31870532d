"""gp_fit_select on the GPU: the selection a step draws from its device-resident state equals the numpy
mirror `Sampler.selection` bit for bit, over every pool and batch geometry of the grid and at the ticks where the
labelled slice changes kind; a wrong captured shape is flagged and still stays inside the pools; nothing is written
outside the selection and the flag."""
import functools

import numpy as np
import pytest
import torch

from grand_plus_amd._common import step_seed

pytestmark = pytest.mark.gpu

BASE, SAMPLER_SEED = 0x5EED0FACADE, 0xC0FFEE
GUARD, MARK = 512, -7777
N_UNLABEL = (1, 3, 100, 65537)


@functools.lru_cache(maxsize=None)
def _unlabelled(n_unlabel, u, seed):
    """The mirror's unlabelled half: it depends on the pool, u and the step's seed alone, so the cases share it."""
    from grand_plus_amd.fit import Sampler
    return Sampler(1, n_unlabel, 1, u).unlabelled(seed)


class Device:
    """One step state and guarded output buffers, reused by every launch of a test."""

    def __init__(self):
        from grand_plus_amd import StepState
        self.state = StepState("cuda", BASE, 0.0, 1.0)
        self.sel = torch.empty(GUARD + 64 + 65537 + GUARD, dtype=torch.int64, device="cuda")
        self.flag = torch.empty(2 * GUARD + 1, dtype=torch.int32, device="cuda")

    def at(self, t):
        self.state.set_tick(t - 1)
        self.state.advance()

    def select(self, sampler, n_l, flag=0):
        """(the selection, the flag afterwards) of the step the state is at; asserts the guard bands."""
        from grand_plus_amd.fit import fit_select
        B = n_l + sampler.u
        self.sel.fill_(MARK)
        self.flag.fill_(MARK)
        self.flag[GUARD] = flag
        fit_select(self.state, sampler, n_l, self.sel[GUARD:GUARD + B], self.flag[GUARD:GUARD + 1])
        sel, fl = self.sel[:GUARD + B + GUARD].cpu().numpy(), self.flag.cpu().numpy()
        assert (sel[:GUARD] == MARK).all() and (sel[GUARD + B:] == MARK).all(), "the selection's guard bands were written"
        assert (fl[:GUARD] == MARK).all() and (fl[GUARD + 1:] == MARK).all(), "the flag's guard bands were written"
        return sel[GUARD:GUARD + B], int(fl[GUARD])


@pytest.fixture(scope="module")
def dev():
    return Device()


@pytest.mark.parametrize("n_train", [1, 5, 7, 64])
@pytest.mark.parametrize("batch_size", [1, 3, 5, 50])
def test_the_selection_equals_the_mirror_bit_for_bit(dev, n_train, batch_size):
    from grand_plus_amd.fit import Sampler
    nb = -(-n_train // batch_size)
    ticks = sorted({1, nb, nb + 1, 2 * nb + 2})            # the first step, the (short) last batch of an epoch, the next epoch's first
    for t in ticks:
        dev.at(t)
        seed = step_seed(BASE, t)
        assert dev.state.read().seed == seed
        for n_unlabel in N_UNLABEL:
            for unlabel_batch in (1, n_unlabel, n_unlabel + 7):
                s = Sampler(n_train, n_unlabel, batch_size, unlabel_batch, SAMPLER_SEED)
                n_l, u = s.shape(t)
                assert u == min(unlabel_batch, n_unlabel) and n_l == min(batch_size, n_train - ((t - 1) % nb) * batch_size)
                got, flag = dev.select(s, n_l)
                what = (n_train, batch_size, n_unlabel, unlabel_batch, t)
                assert flag == 0, what
                assert np.array_equal(got[:n_l], s.labelled(t)), what
                assert np.array_equal(got[n_l:] - n_train, _unlabelled(n_unlabel, u, seed)), what
                if n_unlabel <= 100:                                   # the whole mirror in one call, where that is cheap
                    tr, un = s.selection(t, seed)
                    assert np.array_equal(got, np.concatenate([tr, un + n_train])), what
                if u == n_unlabel:                                     # the whole pool, each node once
                    assert np.array_equal(np.sort(got[n_l:]), np.arange(n_train, n_train + n_unlabel)), what
    assert dev.state.read().tick == ticks[-1]                          # the selection reads the state, it does not move it


@pytest.mark.parametrize("n_train,batch_size", [(1, 1), (5, 3), (7, 3), (7, 50), (64, 5), (64, 1)])
def test_the_labelled_batches_of_an_epoch_are_one_permutation(dev, n_train, batch_size):
    from grand_plus_amd.fit import Sampler
    s = Sampler(n_train, 100, batch_size, 4, SAMPLER_SEED)
    epochs = []
    for epoch in range(3):
        seen, unlabelled = [], []
        for t in range(epoch * s.n_batches + 1, (epoch + 1) * s.n_batches + 1):
            dev.at(t)
            n_l, u = s.shape(t)
            got, flag = dev.select(s, n_l)
            assert flag == 0
            seen += got[:n_l].tolist()
            unlabelled.append(tuple(got[n_l:].tolist()))
            assert len(set(got[n_l:].tolist())) == u and got[n_l:].min() >= n_train and got[n_l:].max() < n_train + 100
        assert sorted(seen) == list(range(n_train)), (epoch, seen)
        assert s.n_batches < 3 or len(set(unlabelled)) > 1                   # a fresh unlabelled draw every step
        epochs.append(seen)
    assert n_train < 5 or not epochs[0] == epochs[1] == epochs[2]             # a fresh labelled order every epoch


@pytest.mark.parametrize("n_train,batch_size,n_unlabel", [(7, 3, 100), (5, 5, 3), (64, 50, 65537), (1, 1, 1)])
def test_a_wrong_shape_sets_the_flag_and_stays_inside_the_pools(dev, n_train, batch_size, n_unlabel):
    from grand_plus_amd.fit import Sampler
    s = Sampler(n_train, n_unlabel, batch_size, 4, SAMPLER_SEED)
    for t in sorted({1, s.n_batches, s.n_batches + 1}):
        dev.at(t)
        right = s.shape(t)[0]
        for n_l in sorted({1, 2, right + 1, batch_size + 3, 2 * n_train + 1, 200} - {right}):
            got, flag = dev.select(s, n_l)
            assert flag == 1, (t, n_l)
            assert got[:n_l].min() >= 0 and got[:n_l].max() < n_train, (t, n_l)
            assert got[n_l:].min() >= n_train and got[n_l:].max() < n_train + n_unlabel, (t, n_l)
            if n_l < right:                                            # a shorter batch is still the head of the right one
                assert np.array_equal(got[:n_l], s.labelled(t)[:n_l])
        # the flag is a bit that is set, never cleared: the other bits and an earlier 1 survive a right shape
        assert dev.select(s, right, flag=6)[1] == 6 and dev.select(s, right, flag=1)[1] == 1
        wrong = right + 1
        assert dev.select(s, wrong, flag=6)[1] == 7
