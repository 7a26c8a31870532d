"""The deterministic table gradient of mag_prop_rows on the GPU (csrc/mag_det.hip; cases in
tests/mag_det_cases.py).

The contract is bitwise: gp_mag_det_keys writes the brute-force entry order's keys and prefix sums, and W.grad equals
the numpy float32 walk of the order contract of csrc/mag_det_abi.hpp.  Against float64 autograd the gradient is held to
§7i's derived bound (n + 8) * 2^-24 * sum|terms| + 1e-7 with n = the destination row's contributions + the longest bag + S:
a destination is a sequential sum of that many products, each reached through the bag's and the row's denominators."""
import ctypes

import numpy as np
import pytest
import torch

import mag_cases as mc
import mag_det_cases as dc

pytestmark = pytest.mark.gpu

GUARD = 96                  # elements of guard band on each side of a buffer
G64, G32 = -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cuda(t):
    return None if t is None else t.cuda()


def _call(P, batch, kw, W=None, **over):
    """mag_prop_rows on the tensors of P: [S, B, H]."""
    from grand_plus_amd import mag_prop_rows
    w, ip, ix, dt, col, val, filled, K = P.cuda()
    kw = dict(kw)
    kw.update(over)
    kw["keep"] = _cuda(kw.get("keep"))
    out = mag_prop_rows(w if W is None else W, ip, ix, dt, col, val, filled, K, _cuda(batch), **kw)
    return out[None] if kw["samples"] == 1 else out


def _grad(P, batch, kw, G, **over):
    """(out, W.grad) of sum(out * G): grad_out is G itself, bit for bit."""
    W = P.W.cuda().requires_grad_(True)
    out = _call(P, batch, kw, W=W, **over)
    (out * G.cuda()).sum().backward()
    return out.detach(), W.grad


# ---- 1. the keys
@pytest.mark.parametrize("slack", dc.SLACK)
@pytest.mark.parametrize("n_slots", sorted(dc.GRID))
def test_keys_and_slot_base_are_the_brute_force_entry_order(n_slots, slack):
    """Slot counts 1, 1 023, 1 024, 1 025 (the scan's chunk), bags of 0, 1, 63, 64 and 65 entries, max_entries one short of
    the total, equal to it, 130 and 1 000 past it (with one slot the grid is one workgroup of 256 threads, so the tail of
    1 000 sentinels takes four passes of the key kernel's tail loop).  Every buffer sits between guard bands that must keep
    their pattern."""
    from grand_plus_amd import _native
    P = dc.grid_problem(n_slots)
    E = dc.entry_order(P, None)
    cap = E["total"] + slack
    _, ip, ix, _dt, col, _val, filled, K = P.cuda()
    base = torch.full((GUARD + n_slots + 1 + GUARD,), G64, dtype=torch.int64, device="cuda")
    keys = torch.full((GUARD + cap + GUARD,), G64, dtype=torch.int64, device="cuda")
    flag = torch.full((GUARD + 1 + GUARD,), G32, dtype=torch.int32, device="cuda")
    flag[GUARD] = 4                                                            # bit 0 clear, another bit set: it has to survive
    rc = _native.lib().gp_mag_det_keys(0, P.V, ip.data_ptr(), ix.data_ptr(), P.N, col.data_ptr(), None if filled is None else filled.data_ptr(),
                                  P.S_rows, K, None, P.S_rows, cap, base.data_ptr() + 8 * GUARD, keys.data_ptr() + 8 * GUARD,
                                  flag.data_ptr() + 4 * GUARD, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    base, keys, flag = base.cpu().numpy(), keys.cpu().numpy(), flag.cpu().numpy()
    for buf, n, g in ((base, n_slots + 1, G64), (keys, cap, G64), (flag, 1, G32)):
        assert (buf[:GUARD] == g).all() and (buf[GUARD + n:] == g).all(), "a guard band was written"
    assert (base[GUARD:GUARD + n_slots + 1] == E["slot_base"]).all()
    live = min(E["total"], cap)
    assert (keys[GUARD:GUARD + live] == E["keys"][:live]).all()
    assert (keys[GUARD + live:GUARD + cap] == P.V).all()                         # the tail is all sentinel
    assert flag[GUARD] == (5 if slack < 0 else 4)
    if slack > 0:
        assert cap - live == slack


def test_keys_of_a_batch_with_ids_columns_and_rows_out_of_range():
    from grand_plus_amd import _native
    c = dc.walk_case("bad_indices")
    P, E = c["P"], c["E"]
    n_sentinel = int((E["keys"] == P.V).sum())
    assert n_sentinel >= 4 and n_sentinel % 2 == 0 and E["total"] > 100          # node 3's bag holds the two bad ids, and it occurs often
    cap = E["total"] + 7
    _, ip, ix, _dt, col, _val, filled, K = P.cuda()
    batch = c["batch"].cuda()
    base = torch.empty(batch.numel() * K + 1, dtype=torch.int64, device="cuda")
    keys = torch.empty(cap, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = _native.lib().gp_mag_det_keys(0, P.V, ip.data_ptr(), ix.data_ptr(), P.N, col.data_ptr(), filled.data_ptr(), P.S_rows, K,
                                  batch.data_ptr(), batch.numel(), cap, base.data_ptr(), keys.data_ptr(), flag.data_ptr(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert (base.cpu().numpy() == E["slot_base"]).all()
    lens = np.diff(E["slot_base"]).reshape(batch.numel(), K)
    assert not lens[1].any() and not lens[3].any() and lens[0].any()             # the rows out of range have no entry
    assert (keys.cpu().numpy() == np.concatenate([E["keys"], np.full(7, P.V)])).all() and int(flag) == 0


# ---- 2. the gradient, bit for bit
@pytest.mark.parametrize("name", list(dc.WALKS))
def test_weight_gradient_is_the_float32_walk_of_the_order_contract(name):
    c = dc.walk_case(name)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, dW = _grad(c["P"], c["batch"], c["kw"], c["G"], deterministic=True, max_entries=c["E"]["total"] + 130, overflow=flag)
    assert dW.dtype == torch.float32 and bool(torch.isfinite(dW).all())
    diff = (dW.cpu() - c["dW"]).abs().max()
    assert _same(dW.cpu(), c["dW"]), f"{name}: max |d| {float(diff):.3e}"
    assert int(flag) == 0
    if name in ("filled0", "pnode1"):
        assert not bool(dW.any())
    else:
        assert bool(dW.any())
    # the forward is what it is without the flag, and the exact capacity gives the same gradient
    assert _same(out, _call(c["P"], c["batch"], c["kw"]))
    _, exact = _grad(c["P"], c["batch"], c["kw"], c["G"], deterministic=True, max_entries=max(c["E"]["total"], 1), overflow=flag)
    assert _same(exact, dW) and int(flag) == 0


def test_torchs_deterministic_mode_selects_the_path_and_a_short_buffer_sets_the_flag():
    c = dc.walk_case("h7_k5_s3")
    P, total = c["P"], c["E"]["total"]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.use_deterministic_algorithms(True)
    try:
        _, dW = _grad(P, c["batch"], c["kw"], c["G"], max_entries=total, overflow=flag)
    finally:
        torch.use_deterministic_algorithms(False)
    assert _same(dW.cpu(), c["dW"]) and int(flag) == 0
    H, K, S, _f, _m, p_node, training, _mask = dc.WALKS["h7_k5_s3"]
    for cap in (total - 1, total // 2, 1):
        flag.zero_()
        _, short = _grad(P, c["batch"], c["kw"], c["G"], deterministic=True, max_entries=cap, overflow=flag)
        want = dc.walk_dW32(P, c["batch"], S, p_node, training, c["kw"]["keep"], c["G"], max_entries=cap)
        assert int(flag) == 1 and _same(short.cpu(), want), cap                  # the entries below the capacity, and only they
    _grad(P, c["batch"], c["kw"], c["G"], deterministic=True, max_entries=1)     # no overflow tensor: a private one, never read


def test_segments_of_63_64_and_65_entries_and_one_that_runs_past_its_window():
    P = dc.segments_problem()
    S, p = 2, 0.5
    g = torch.Generator().manual_seed(3)
    keep = torch.ones((S, 4), dtype=torch.uint8)
    keep[1, 2] = 0                                                              # one slot dropped in one sample
    G = torch.randn((S, 2, P.H), generator=g)
    kw = dict(samples=S, dropnode_rate=p, input_droprate=0.0, training=True, seed=1, keep=keep)
    E = dc.entry_order(P, None)
    order = np.argsort(E["keys"], kind="stable")
    sk = E["keys"][order]
    assert [int((sk == a).sum()) for a in range(4)] == [63, 64, 65, 64]
    assert int(np.flatnonzero(sk == 1)[0]) == 63 and int(np.flatnonzero(sk == 1)[-1]) == 126   # starts at 63, ends in the next window
    _, dW = _grad(P, None, kw, G, deterministic=True, max_entries=E["total"])
    assert _same(dW.cpu(), dc.walk_dW32(P, None, S, p, True, keep, G)) and not bool(dW[4].any())


def test_the_sum_runs_left_to_right_in_entry_order():
    """§7i's order pin: contributions [2^25, 1, -2^25, 1, ...] to one table element.  The float32 left-to-right loop gives 1
    (each 1 added to 2^25 is lost, the one added to 0 stays); the exact sum is 4, and any regrouping gives another value."""
    P, G = dc.order_pin_problem(8)
    kw = dict(samples=1, dropnode_rate=0.5, input_droprate=0.0, training=False, seed=1)
    loop = np.float32(0.0)
    for x in G.reshape(-1).numpy():
        loop = np.float32(loop + x)
    assert loop == 1.0 and float(G.double().sum()) == 4.0
    _, dW = _grad(P, None, kw, G, deterministic=True, max_entries=8)
    assert float(dW[0, 0]) == float(loop) and float(dW[1, 0]) == 0.0
    assert _same(dW.cpu(), dc.walk_dW32(P, None, 1, 0.5, False, None, G))
    rev = torch.arange(7, -1, -1, dtype=torch.int32)                             # the batch reversed: g follows the batch, so the order stays
    _, dW = _grad(P, rev, kw, G, deterministic=True, max_entries=8)
    assert float(dW[0, 0]) == 1.0


# ---- 3. against float64
@pytest.mark.parametrize("name", ["h1_k1_s1", "h7_k5_s3", "h64_k32_s2", "h65_k5_s16", "pnode0", "hub"])
def test_weight_gradient_matches_float64_autograd_under_the_derived_bound(name):
    c = mc.case(name)
    P, S = c["P"], c["S"]
    _out64, _terms, dW64, dW_terms = c["ref"]
    E = dc.entry_order(P, c["batch"])
    if name == "hub":
        assert P.longest == 4097
    kw = dict(c["kw"], keep=c["keep"])
    _, dW = _grad(P, c["batch"], kw, c["G"], deterministic=True, max_entries=E["total"])
    n = dc.contributions(P, c["batch"]).double()[:, None] + P.longest + S
    bound = (n + 8) * 2.0 ** -24 * dW_terms + 1e-7
    err = (dW.double().cpu() - dW64).abs()
    ratio = float((err / bound).max())
    print(f"[mag det] {name}: worst error / bound {ratio:.3g}, max |d| {float(err.max()):.3e}")
    assert ratio <= 1.0


# ---- 4. reproducibility, the forward, the host
def test_five_backwards_are_bitwise_equal_and_the_atomic_path_is_untouched_by_max_entries():
    c = mc.case("h64_k32_s2")
    P = c["P"]
    kw = dict(c["kw"], keep=c["keep"])
    total = dc.entry_order(P, c["batch"])["total"]
    runs = [_grad(P, c["batch"], kw, c["G"], deterministic=True, max_entries=total + 130) for _ in range(5)]
    for out, dW in runs[1:]:
        assert _same(out, runs[0][0]) and _same(dW, runs[0][1])
    # deterministic=False: the atomic backward whether max_entries is given or not; each inside today's rule, same forward
    _o64, _t, dW64, dW_terms = c["ref"]
    with_cap = _grad(P, c["batch"], kw, c["G"], deterministic=False, max_entries=1)
    without = _grad(P, c["batch"], kw, c["G"], deterministic=False)
    assert _same(with_cap[0], without[0]) and _same(with_cap[0], runs[0][0])
    for what, (_o, dW) in (("atomic, max_entries", with_cap), ("atomic", without)):
        mc.close(dW, dW64, dW_terms, c["roundings"], what)


def test_forward_and_backward_do_not_synchronise():
    c = dc.walk_case("h64_k32_s2")
    P = c["P"]
    w, ip, ix, dt, col, val, filled, K = P.cuda()
    from grand_plus_amd import mag_prop_rows
    W = P.W.cuda().requires_grad_(True)
    G, batch = c["G"].cuda(), c["batch"].cuda()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    cap = c["E"]["total"] + 130
    warm = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, batch, deterministic=True, max_entries=cap, overflow=flag, **c["kw"])
    (warm * G).sum().backward()                                                  # loads code, fills the allocator
    W.grad = None
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, batch, deterministic=True, max_entries=cap, overflow=flag, **c["kw"])
        (out * G).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert _same(W.grad.cpu(), c["dW"]) and int(flag) == 0
