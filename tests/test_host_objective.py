"""CPU tests of the S-sample random_prop and fused-objective entries: bad arguments are refused before any
device work, the Python wrappers refuse CPU tensors (no CPU fallback), sample_seed follows the header's formula, and the
cases of the objective's edge tests (objective_cases.py) hold their margin and leave the tolerance room for fp32."""
import ctypes
import math

import pytest

import objective_cases as oc
from grand_plus_amd import _native

NULL = None
P, S0 = ctypes.c_void_p(16), ctypes.c_void_p(0)
SEED = ctypes.c_uint64(1)


def _lib():
    return _native.lib()


@pytest.mark.parametrize("S", [0, 17, -1])
def test_multi_entries_refuse_a_sample_count_outside_1_16(S):
    L = _lib()
    assert L.gp_random_prop_rows_multi(0, P, 10, 8, P, P, P, 16, P, 4, S, 0.5, 1, SEED, NULL, 0, P, S0) == _native.GP_ERR_INVALID_ARG
    assert "gp_random_prop_rows_multi" in L.gp_last_error().decode()
    assert L.gp_random_prop_coo_multi(0, P, 8, 8, P, P, 4, S, 0.5, 1, SEED, NULL, P, S0) == _native.GP_ERR_INVALID_ARG
    assert "gp_random_prop_coo_multi" in L.gp_last_error().decode()
    assert L.gp_random_prop_coo_multi_backward(0, P, 4, 8, P, P, 8, S, 0.5, 1, SEED, NULL, P, S0) == _native.GP_ERR_INVALID_ARG
    assert "gp_random_prop_coo_multi_backward" in L.gp_last_error().decode()
    assert L.gp_random_prop_rows_multi_backward(0, P, 4, 8, P, P, P, 16, P, S, 0.5, 1, SEED, NULL, 0, P, 10, S0) == _native.GP_ERR_INVALID_ARG
    assert "gp_random_prop_rows_multi_backward" in L.gp_last_error().decode()


def test_multi_entries_check_sizes_and_pointers_before_the_device():
    L = _lib()
    E = _native.GP_ERR_INVALID_ARG
    # rows: (device, x, n_nodes, F, col, val, filled, K, batch_rows, n_batch, S, rate, training, seed, keep, keep_stride, out, stream)
    rows = L.gp_random_prop_rows_multi
    assert rows(0, P, 10, 8, P, P, P, 0, P, 4, 2, 0.5, 1, SEED, NULL, 0, P, S0) == E          # K < 1
    assert rows(0, P, 10, 8, P, P, P, 1025, P, 4, 2, 0.5, 1, SEED, NULL, 0, P, S0) == E       # K > 1024
    assert rows(0, P, 10, 0, P, P, P, 16, P, 4, 2, 0.5, 1, SEED, NULL, 0, P, S0) == E         # F < 1
    assert rows(0, P, 10, 8, P, P, P, 16, P, 4, 2, 1.5, 1, SEED, NULL, 0, P, S0) == E         # rate > 1
    assert rows(0, P, 10, 8, P, P, P, 16, P, 4, 2, 0.5, 1, SEED, P, 0, P, S0) == E            # a mask without its stride
    assert rows(0, NULL, 10, 8, P, P, P, 16, P, 4, 2, 0.5, 1, SEED, NULL, 0, P, S0) == _native.GP_ERR_NULL
    assert rows(0, P, 10, 8, P, P, P, 16, P, 4, 2, 0.5, 1, SEED, NULL, 0, NULL, S0) == _native.GP_ERR_NULL
    assert rows(0, NULL, 10, 8, NULL, NULL, NULL, 16, NULL, 0, 2, 0.5, 1, SEED, NULL, 0, NULL, S0) == _native.GP_OK   # nothing to do
    coo = L.gp_random_prop_coo_multi
    assert coo(0, P, -1, 8, P, P, 4, 2, 0.5, 1, SEED, NULL, P, S0) == E                      # n_entries < 0
    assert coo(0, P, 8, 0, P, P, 4, 2, 0.5, 1, SEED, NULL, P, S0) == E                       # F < 1
    assert coo(0, P, 8, 8, P, P, -1, 2, 0.5, 1, SEED, NULL, P, S0) == E                      # n_out < 0
    assert coo(0, P, 8, 8, P, NULL, 4, 2, 0.5, 1, SEED, NULL, P, S0) == _native.GP_ERR_NULL
    assert coo(0, P, 8, 8, P, P, 4, 2, 0.5, 1, SEED, NULL, NULL, S0) == _native.GP_ERR_NULL
    assert coo(0, NULL, 0, 8, NULL, NULL, 0, 2, 0.5, 1, SEED, NULL, NULL, S0) == _native.GP_OK
    cb = L.gp_random_prop_coo_multi_backward
    assert cb(0, P, 4, 8, P, P, 8, 2, -0.5, 1, SEED, NULL, P, S0) == E
    assert cb(0, NULL, 4, 8, P, P, 8, 2, 0.5, 1, SEED, NULL, P, S0) == _native.GP_ERR_NULL
    assert cb(0, P, 4, 8, P, P, 8, 2, 0.5, 1, SEED, NULL, NULL, S0) == _native.GP_ERR_NULL
    rb = L.gp_random_prop_rows_multi_backward
    assert rb(0, P, 4, 8, P, P, P, 16, P, 2, 0.5, 1, SEED, NULL, 0, P, 0, S0) == E           # no nodes
    assert rb(0, P, 4, 8, NULL, P, P, 16, P, 2, 0.5, 1, SEED, NULL, 0, P, 10, S0) == _native.GP_ERR_NULL
    assert rb(0, P, 4, 8, P, P, P, 16, P, 2, 0.5, 1, SEED, NULL, 0, NULL, 10, S0) == _native.GP_ERR_NULL


def _loss(fn, **kw):
    a = dict(z=P, S=2, B=10, C=7, labels=P, n_l=4, ignore=-100, w=1.0, tem=0.5, conf=0.3, kind=_native.GP_LOSS_L2, logp=0)
    a.update(kw)
    head = (0, a["z"], a["S"], a["B"], a["C"], a["labels"], a["n_l"], a["ignore"], a["w"], a["tem"], a["conf"], a["kind"], a["logp"])
    if fn == "gp_grand_loss":   # (..., workspace, out, counts, stream)
        tail = (kw.get("ws", P), kw.get("out", P), kw.get("counts", P), S0)
    else:                       # (..., grad_loss, grad_sup, grad_con, counts, grad_z, stream)
        tail = (kw.get("gl", P), NULL, NULL, kw.get("counts", P), kw.get("out", P), S0)
    return getattr(_lib(), fn)(*head, *tail)


@pytest.mark.parametrize("fn", ["gp_grand_loss", "gp_grand_loss_backward"])
def test_loss_entries_check_arguments_before_the_device(fn):
    E = _native.GP_ERR_INVALID_ARG
    assert _loss(fn, S=0) == E
    assert _loss(fn, S=17) == E
    assert _loss(fn, C=0) == E
    assert _loss(fn, C=4097) == E
    assert _loss(fn, B=-1) == E
    assert _loss(fn, n_l=11) == E                       # more labelled rows than rows
    assert _loss(fn, n_l=-1) == E
    assert _loss(fn, tem=0.0) == E
    assert _loss(fn, tem=-0.1) == E
    assert _loss(fn, tem=float("nan")) == E
    assert _loss(fn, kind=2) == E
    assert _loss(fn, kind=-1) == E
    assert fn in _lib().gp_last_error().decode()
    assert _loss(fn, z=NULL) == _native.GP_ERR_NULL
    assert _loss(fn, labels=NULL) == _native.GP_ERR_NULL
    assert _loss(fn, counts=NULL) == _native.GP_ERR_NULL
    assert _loss(fn, out=NULL) == _native.GP_ERR_NULL
    assert fn in _lib().gp_last_error().decode()
    if fn == "gp_grand_loss":
        assert _loss(fn, ws=NULL) == _native.GP_ERR_NULL
    else:
        assert _loss(fn, gl=NULL) == _native.GP_ERR_NULL
        assert _loss(fn, B=0, n_l=0, z=NULL, labels=NULL, out=NULL) == _native.GP_OK    # nothing to do


@pytest.mark.parametrize("case,coeffs", oc.DRAWN, ids=[oc.case_id(c) for c, _ in oc.DRAWN])
def test_edge_cases_hold_their_margin_and_the_float32_reference_meets_the_tolerance(case, coeffs):
    """Proves the cases of test_gpu_objective.py's edge tests before a GPU sees them: the margin condition of `n_conf`,
    and that the tolerance leaves room for correct fp32 arithmetic -- the reference restated in float32 on the host is
    inside it against float64 under every upstream-gradient combination the GPU test runs.  The sharpening cases have no
    float32 reference (it is NaN, asserted here): there the float64 reference and its gradient must be finite."""
    import torch
    from oracle.objective_ref import consis_loss_ref
    z, labels, n_l, conf = oc.build(case)
    assert z.dtype == torch.float32 and tuple(z.shape) == (case.S, case.B, case.C) and labels.numel() >= n_l == case.n_l
    assert oc.margin_ok(z, n_l, conf, case.log_probs)
    if 0.0 < conf < 1.0:
        assert not bool(((oc.avg_p_max(z, n_l, case.log_probs) - conf).abs() <= 1e-4 * conf).any())
    else:
        assert oc.counts(case)["n_conf"] == (case.B - n_l if conf <= 0.0 else 0)
    if case in oc.SHARPEN:
        lps = [torch.log_softmax(z[s], -1) for s in range(case.S)]
        assert math.isnan(float(consis_loss_ref(lps, case.tem, conf, case.kind)))          # fp32 underflow: 0 / 0 or 0 * inf
        r64 = oc.reference(case)
        assert math.isfinite(r64["con"]) and bool(torch.isfinite(r64["grad"]).all())                 # n_l = 0: L_sup and the loss are NaN
        assert math.isnan(r64["loss"]) and float(r64["grad"].abs().max()) > 0
        return
    rows = 4096 if case.B > 100000 else None                                            # the float32 check of the largest case: a slice
    for k in coeffs:
        r64, r32 = oc.reference(case, k, torch.float64, rows), oc.reference(case, k, torch.float32, rows)
        oc.assert_matches(r32, r32["grad"], r64, f"float32 reference, {oc.case_id(case)} {k}")


def test_edge_case_builders_reach_what_they_are_for():
    """The special inputs are what their tests need: ties that torch.argmax resolves to the first index with both
    outcomes present, a finite float64 reference beside -inf logits, confident rows and both right and wrong predictions in the class cases,
    a last partial trip in the largest case."""
    import torch
    z, labels, n_l, _ = oc.build(oc.TIES)
    last = z[oc.TIES.S - 1, :n_l]
    for r, cols in enumerate(oc.TIE_COLUMNS):
        assert torch.nonzero(last[r] == last[r].max())[:, 0].tolist() == sorted(cols)
        assert int(last[r].argmax()) == min(cols) and int(labels[r]) == (min(cols) if r % 2 == 0 else cols[-1])
    assert oc.counts(oc.TIES)["n_correct"] == 3 and {c // 64 for cols in oc.TIE_COLUMNS for c in cols} == {0, 1, 2}
    z, labels, n_l, _ = oc.build(oc.NEGINF)
    assert int(torch.isfinite(z[:, 2]).sum()) == 2 * oc.NEGINF.S and bool(torch.isfinite(z[:, 2, int(labels[2])]).all())
    r64 = oc.reference(oc.NEGINF)
    assert math.isfinite(r64["loss"]) and bool(torch.isfinite(r64["grad"]).all())
    for case in oc.CLASSES + oc.SAMPLES + oc.UPSTREAM + oc.LOGPROB:
        assert oc.counts(case)["n_conf"] > 0, case
    for case in oc.CLASSES + [c for c in oc.SAMPLES if c.n_l]:
        if case.C > 2:
            assert 0 < oc.counts(case)["n_correct"] < oc.counts(case)["n_valid"], case
    assert oc.SECOND_TRIP.B == 65535 * 4 + 37 and oc.ALL_LABELLED.B == oc.ALL_LABELLED.n_l
    assert oc.MAX_S == _native.GP_MAX_SAMPLES


def test_sample_seed_follows_the_header_formula():
    from grand_plus_amd.augment import sample_seed
    M = 2**64 - 1

    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    for seed in (0, 1, 0x5EED, M, 0x9E3779B97F4A7C15):
        assert sample_seed(seed, 0) == seed
        seeds = [sample_seed(seed, s) for s in range(16)]
        assert len(set(seeds)) == 16
        for s in range(1, 16):
            assert seeds[s] == mix(seed ^ (s * 0xD6E8FEB86659FD93 & M))
            assert 0 <= seeds[s] <= M


def test_python_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from grand_plus_amd.augment import random_prop, random_prop_rows
    from grand_plus_amd.objective import consis_loss, grand_plus_loss
    feats = torch.randn(3, 4)
    with pytest.raises(TypeError):
        random_prop(feats, torch.ones(3), torch.tensor([0, 0, 1]), 0.5, samples=2)
    with pytest.raises(TypeError):
        random_prop(feats, torch.ones(3), torch.tensor([0, 0, 1]), 0.5, samples=2, n_out=2)
    with pytest.raises(TypeError):
        random_prop_rows(feats, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), None, 2, samples=2)
    for bad in (0, 17, 2.0):
        with pytest.raises(ValueError):
            random_prop(feats, torch.ones(3), torch.tensor([0, 0, 1]), 0.5, samples=bad)
        with pytest.raises(ValueError):
            random_prop_rows(feats, torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.float64), None, 2, samples=bad)
    z = torch.randn(2, 5, 3)
    with pytest.raises(TypeError):
        grand_plus_loss(z, torch.zeros(2, dtype=torch.int64), 2, 1.0)
    with pytest.raises(TypeError):
        grand_plus_loss([z[0], z[1]], None, 0, 1.0)
    with pytest.raises(TypeError):
        consis_loss([torch.log_softmax(z[0], -1)], 0.5, 0.1)
    with pytest.raises(ValueError):
        grand_plus_loss(z, None, 0, 1.0, kind="ce")
