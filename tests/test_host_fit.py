"""CPU tests of the fit loop: the keyed permutation's Python mirror against csrc/fit_perm.hpp itself
(tests/native/fit_perm_check.cpp, built with the address and undefined-behaviour sanitizers), the entry points' error
codes before any GPU work, and the host rules: the sampler's shapes and the early-stop rule against a transcription of model.py:344-359."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import native_check
from fit_cases import RULE_CASES, SCRIPTS, bits as _bits, run_rule
from grand_plus_amd import _common, _native
from grand_plus_amd import fit as gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
M = 2 ** 64 - 1
KEYS = (0, 0x5EED0FACADE, M)
SIZES = list(range(1, 301)) + [1000, 4095, 4096, 4097, 65537]
P = ctypes.c_void_p(16)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """ask(lines) -> one list of ints per line.  Nothing is preloaded: the sanitizers are linked into the program itself."""
    exe = native_check.build(tmp_path_factory, "fit_perm_check")
    return lambda lines: native_check.ints(native_check.run(exe, lines))


# ---- 1. the permutation
def test_the_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_perm.cpp"
    src.write_text('#include "fit_perm.hpp"\nstatic uint64_t id(uint64_t x) { return x; }\n'
                   "int main() { return (int)gp_fit::perm(id, 1, 5u, 4u) >= 5; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_perm"), str(src)], check=True,
                   timeout=120)
    text = open(os.path.join(CSRC, "fit_perm.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", text) == ["cstdint"]


@pytest.mark.parametrize("key", KEYS)
def test_perm_index_is_the_header_and_a_permutation_at_every_size(checker, key):
    """Exhaustive: every i of every n in 1..300 and of 1000, 4095, 4096, 4097 (around a power of four) and 65537."""
    got = checker([f"all {key} {n}" for n in SIZES])
    assert len(got) == len(SIZES)
    for n, image in zip(SIZES, got):
        assert sorted(image) == list(range(n)), (key, n)
        assert image == [_common.perm_index(key, n, i) for i in range(n)], (key, n)


def test_known_answers_and_the_domain(checker):
    """Values printed once by the check program: a change of the formula shows here."""
    known = {(0, 1, 0): 0, (0, 2, 0): KNOWN[0], (0, 7, 3): KNOWN[1], (0x5EED, 10000, 0): KNOWN[2], (0x5EED, 10000, 9999): KNOWN[3],
             (M, 65537, 65536): KNOWN[4], (123456789, 2 ** 31 - 1, 2 ** 31 - 2): KNOWN[5], (1, 2 ** 30 + 1, 0): KNOWN[6]}
    got = checker([f"perm {k} {n} {i}" for k, n, i in known])
    for (k, n, i), want, (g,) in zip(known, known.values(), got):
        assert g == want == _common.perm_index(k, n, i), (k, n, i, g)
    assert _common.perm_index(M + 1 + 0x5EED, 10000, 0) == KNOWN[2]                       # the key is taken modulo 2^64
    for n, i in ((0, 0), (2 ** 31, 0), (5, 5), (5, -1)):
        with pytest.raises(ValueError):
            _common.perm_index(1, n, i)
    # different keys give different permutations, and a permutation is no identity
    a, b = ([_common.perm_index(k, 100, i) for i in range(100)] for k in (1, 2))
    assert a != b and a != list(range(100))


KNOWN = (0, 1, 50, 6642, 35048, 1362380606, 554691899)


def test_the_multipliers_are_new_odd_and_stated_once(checker):
    text = open(os.path.join(CSRC, "fit_perm.hpp")).read()
    muls = {name: re.search(r"#define %s (0x[0-9A-F]{16})ull\n" % name, text).group(1)
            for name in ("GP_FIT_ROUND_MUL", "GP_FIT_EPOCH_MUL", "GP_FIT_UNLABEL_MUL")}
    values = [int(v, 16) for v in muls.values()]
    assert len(set(values)) == 3 and all(v % 2 == 1 and v >> 32 for v in values)
    assert checker(["consts"]) == [values + [4]]
    assert values == [_common._FIT_ROUND_MUL, _common._FIT_EPOCH_MUL, _common._FIT_UNLABEL_MUL]
    others = [p for p in glob.glob(os.path.join(CSRC, "*")) + glob.glob(os.path.join(ROOT, "include", "*"))
              if os.path.basename(p) != "fit_perm.hpp"]
    assert len(others) > 20
    for path in others:
        body = open(path, errors="replace").read().upper()
        for name, lit in muls.items():
            assert lit[2:] not in body, f"{os.path.basename(path)} holds the value of {name}"
    hip = open(os.path.join(CSRC, "fit.hip")).read()
    assert '#include "fit_perm.hpp"' in hip and '#include "gp_common.hpp"' in hip
    for name in ("fmix64", "mix64", "perm", "perm_bits", "step_slice", "epoch_key", "unlabel_key"):
        assert not re.search(r"\b%s\s*\([^;{]*\)\s*\{" % name, hip), f"fit.hip restates {name}"
    for name in ("mix64", "gp_fit::perm", "gp_fit::step_slice", "gp_fit::epoch_key", "gp_fit::unlabel_key"):
        assert re.search(r"\b%s\(" % name, hip), f"fit.hip does not call {name}"
    assert "0x9E3779B97F4A7C15" not in hip and "0xBF58476D1CE4E5B9" not in hip
    assert not re.search(r"atomic", hip.replace("no atomics", ""), flags=re.I)
    py = open(os.path.join(ROOT, "grand_plus_amd", "_common.py")).read()
    assert len(re.findall(r"^def perm_index", py, flags=re.M)) == 1 and py.index("def step_seed") < py.index("def perm_index")


# ---- 2. the sampler
GEOMETRIES = [(1, 1), (5, 1), (5, 3), (5, 5), (7, 3), (7, 50), (64, 5), (20, 8), (2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 1000)]


def test_sampler_shapes_hold_across_epoch_boundaries(checker):
    for n_train, bs in GEOMETRIES:
        s = gf.Sampler(n_train, 9, bs, 4, 1)
        nb = -(-n_train // bs)
        assert s.n_batches == nb
        ticks = sorted({1, 2, nb, nb + 1, 2 * nb, 2 * nb + 1, 3 * nb - 1, 7 * nb + 2} - {0})
        got = checker([f"slice {t} {n_train} {bs}" for t in ticks])
        for t, (epoch, lo, n_l) in zip(ticks, got):
            assert s._slice(t) == (epoch, lo, n_l) and s.shape(t) == (n_l, 4), (n_train, bs, t)
            assert 1 <= n_l <= min(bs, n_train) and lo + n_l <= n_train
            assert (lo + n_l == n_train) == (t % nb == 0)                        # the last batch of an epoch ends the pool
        assert sum(s.shape(t)[0] for t in range(1, min(nb, 500) + 1)) == (n_train if nb <= 500 else 500 * bs)
    assert gf.Sampler(7, 3, 3, 4).shape(1) == (3, 3) and gf.Sampler(7, 3, 3, 4).u == 3          # u = min(unlabel_batch, n_unlabel)
    assert [gf.Sampler(7, 9, 3, 4).shape(t)[0] for t in range(1, 8)] == [3, 3, 1, 3, 3, 1, 3]
    with pytest.raises(ValueError, match="steps count from 1"):
        gf.Sampler(7, 9, 3, 4).shape(0)
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (2 ** 31, 1, 1, 1), (1, 1, 1, 2 ** 31), (1.0, 1, 1, 1), (True, 1, 1, 1)):
        with pytest.raises(ValueError, match=r"must be an int in \[1, 2\*\*31\)"):
            gf.Sampler(*bad)


def test_sampler_selection_follows_its_definition(checker):
    s = gf.Sampler(7, 100, 3, 4, base_seed=0xABCDEF)
    epoch_images = {}
    for t in range(1, 10):
        seed = _common.step_seed(99, t)
        epoch, lo, n_l = s._slice(t)
        (k_l, k_u), = checker([f"keys {s.base_seed} {epoch} {seed}"])
        assert k_l == _common._mix(s.base_seed ^ ((epoch + 1) * _common._FIT_EPOCH_MUL & M))
        assert k_u == _common._mix(seed ^ _common._FIT_UNLABEL_MUL)
        tr, un = s.selection(t, seed)
        assert tr.dtype == un.dtype == np.int64 and tr.shape == (n_l,) and un.shape == (4,)
        assert tr.tolist() == [_common.perm_index(k_l, 7, lo + i) for i in range(n_l)]
        assert un.tolist() == [_common.perm_index(k_u, 100, i) for i in range(4)] and len(set(un.tolist())) == 4
        epoch_images.setdefault(epoch, []).extend(tr.tolist())
    assert all(sorted(v) == list(range(7)) for v in epoch_images.values()) and len(epoch_images) == 3
    assert epoch_images[0] != epoch_images[1]
    # the unlabelled batch changes with the step's seed alone, the labelled one with the sampler's
    assert s.selection(1, 5)[1].tolist() != s.selection(1, 6)[1].tolist()
    assert s.selection(1, 5)[0].tolist() == s.selection(1, 6)[0].tolist()
    whole = gf.Sampler(7, 5, 3, 9, 1).selection(2, 3)[1]                          # unlabel_batch above the pool: the whole pool, once
    assert sorted(whole.tolist()) == list(range(5))


# ---- 3. the host images of gp_fit_track (the binding itself is held in tests/test_host_abi.py)
def test_the_track_images_carry_the_structs_fields():
    assert gf.TrackImage._fields == tuple(n for n, _ in _native.GpFitTrack._fields_)
    init = gf.new_track()
    assert set(init) == set(gf.TrackImage._fields) and init["best_loss"] == np.inf and sum(v for k, v in init.items() if k != "best_loss") == 0


# ---- 4. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def select(st=P, n_train=7, n_unlabel=9, bs=3, ub=4, n_l=3, sel=P, flag=P):
        return L.gp_fit_select(0, st, 1, n_train, n_unlabel, bs, ub, n_l, sel, flag, None)

    for bad in (0, -1, 2 ** 31, 2 ** 40):
        for kw in ("n_train", "n_unlabel", "bs", "ub", "n_l"):
            assert select(**{kw: bad}) == E, (kw, bad)
    assert "gp_fit_select" in L.gp_last_error().decode()
    assert select(st=None) == N and select(sel=None) == N and select(flag=None) == N
    assert select(st=None, n_train=0) == E                                      # sizes are judged first

    def update(tr=P, val=P, st=P, mode=_native.GP_FIT_STOP_BOTH, patience=3):
        return L.gp_fit_track_update(0, tr, val, st, mode, patience, None)

    assert update(mode=2) == E and update(mode=-1) == E and update(patience=0) == E and update(patience=-5) == E
    assert "gp_fit_track_update" in L.gp_last_error().decode()
    assert update(tr=None) == N and update(val=None) == N and update(st=None) == N

    def snap(entries, tr=P, n=None, null=False):
        tab = (_native.GpFitCopy * max(len(entries), 1))(*[_native.GpFitCopy(*e) for e in entries])
        return L.gp_fit_snapshot(0, tr, None if null else tab, len(entries) if n is None else n, None)

    assert snap([(16, 32, 1)], n=-1) == E
    assert "gp_fit_snapshot" in L.gp_last_error().decode()
    assert snap([(16, 32, -1)]) == E and snap([(18, 32, 1)]) == E and snap([(16, 33, 1)]) == E
    assert snap([(16, 32, 1)], tr=None) == N and snap([(16, 32, 1)], null=True) == N
    assert snap([(None, 32, 1)]) == N and snap([(16, None, 1)]) == N
    assert snap([(16, 32, 0)] * 40 + [(None, 32, 1)]) == N                      # every entry is checked, past the first launch's 32 too
    # nothing to do: GP_OK with nothing launched
    assert snap([]) == OK and snap([(16, 32, 0), (None, None, 0)]) == OK and snap([(16, 32, 0)] * 70) == OK


def test_the_python_layer_refuses_before_any_device_call(monkeypatch):
    import torch
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    model = torch.nn.Linear(3, 2)
    for kw, msg in ((dict(stop_mode="loss"), "stop_mode"), (dict(patience=0), "patience"), (dict(patience=2.0), "patience"),
                    (dict(device="cpu"), "no CPU fallback")):
        with pytest.raises(ValueError, match=msg):
            gf.BestTracker(model, **{**dict(device="cuda:0", stop_mode="both", patience=3), **kw})
    with pytest.raises(TypeError, match="a TrainStep and a Sampler"):
        gf.fit(object(), gf.Sampler(7, 9, 3, 4), [1], epochs=1)
    for kw in (dict(epochs=0), dict(epochs=1, poll_every=0), dict(epochs=1, max_steps=-1), dict(epochs=1.5)):
        with pytest.raises(ValueError):
            gf.fit(object(), gf.Sampler(7, 9, 3, 4), [1], **kw)


# ---- 5. the early-stop rule
def _reference_loop(seq, stop_mode, patience):
    """model.py:344-359 transcribed, one validation per entry of seq (num_batch counts them): the tick of the last
    checkpoint written, the tick it broke at, the final loss_mn / acc_mx / bad_counter, every tick that wrote a checkpoint."""
    loss_values, acc_values, saved = [], [], []
    bad_counter, loss_mn, acc_mx, best_batch, stop = 0, np.inf, 0.0, None, None
    for num_batch, (loss_val, acc_val) in enumerate(seq):
        loss_values.append(loss_val)
        acc_values.append(acc_val)
        if acc_values[-1] >= acc_mx:
            if stop_mode == 'acc' or (stop_mode == 'both' and loss_values[-1] <= loss_mn):
                loss_mn = loss_values[-1]
                acc_mx = acc_values[-1]
                best_batch = num_batch
                saved.append(num_batch + 1)
                bad_counter = 0
        else:
            bad_counter += 1
        if bad_counter >= patience:
            stop = num_batch + 1
            break
    return (best_batch + 1 if best_batch is not None else 0), stop, loss_mn, acc_mx, bad_counter, saved


@pytest.mark.parametrize("name,mode,patience", RULE_CASES)
def test_the_rule_is_the_references_on_scripted_sequences(name, mode, patience):
    seq = [(float(np.float32(l)), float(np.float32(a))) for l, a in SCRIPTS[name]]
    best, stop, loss_mn, acc_mx, bad, saved = _reference_loop(seq, mode, patience)
    images, copies = run_rule(seq, mode, patience, extra=0)
    n = stop if stop is not None else len(seq)                              # the reference breaks there; the rule freezes
    at = images[n - 1]
    assert at["best_tick"] == best and bool(at["stopped"]) == (stop is not None) and at["stop_tick"] == (stop or 0)
    assert at["bad_counter"] == bad and at["n_evals"] == n
    assert (at["best_loss"] == np.float32(loss_mn) or (np.isnan(loss_mn) and np.isnan(at["best_loss"]))) and at["best_acc"] == np.float32(acc_mx)
    assert [t for t in copies if t <= n] == saved
    # frozen after the stop: later results, however good, change nothing but copy_now = 0
    images, copies = run_rule(seq, mode, patience, extra=3)
    if stop is not None:
        for later in images[n:]:
            assert _bits(later) == _bits({**at, "copy_now": 0})
        assert [t for t in copies if t > n] == []
    else:                                                                   # still running: the next better result is taken
        assert images[n]["best_tick"] == n + 1 and images[n]["copy_now"] == 1 and images[n]["bad_counter"] == 0


def test_the_scripts_reach_every_branch():
    seen = set()
    for name, mode, patience in RULE_CASES:
        images, copies = run_rule(SCRIPTS[name], mode, patience, extra=0)
        seen |= {("stopped", bool(images[-1]["stopped"])), ("took", bool(copies)), ("gap", mode == "both" and any(
            a["bad_counter"] == b["bad_counter"] and not b["copy_now"] and not a["stopped"] for a, b in zip(images, images[1:])))}
    assert seen == {("stopped", True), ("stopped", False), ("took", True), ("took", False), ("gap", True), ("gap", False)}


# ---- 6. the package
def test_the_names_are_reachable_from_the_package_and_stay_out_of_all():
    import grand_plus_amd
    assert grand_plus_amd.Sampler is gf.Sampler and grand_plus_amd.BestTracker is gf.BestTracker
    assert callable(grand_plus_amd.fit) and grand_plus_amd.fit.fit is gf.fit
    assert not {"fit", "Sampler", "BestTracker"} & set(grand_plus_amd.__all__)
    assert gf.FitResult._fields == ("steps", "best_tick", "stop_tick", "best_loss", "best_acc")
    from grand_plus_amd import step
    assert hasattr(step.TrainStep, "step_sampled") and step.MAX_GRAPHS == 4
