"""The row-list clip + Adam step of the embedding table on the GPU.  Kernel level: gp_optim_rows_sqnorm and
gp_clip_adam_rows(_dev) over hand-made key lists (tests/optim_rows_cases.py), with dW poisoned with NaN outside the touched
rows and guard bands round every buffer, against the existing dense gp_clip_adam_step on the zero-filled dense gradient
that holds the same rows, from one state for one step: exact mode bitwise over the whole table, lazy mode bitwise on the
touched rows and bitwise unchanged everywhere else.  Then ClipAdam.set_row_grad over five chained steps, under the sync
debug mode, and through a checkpoint."""
import copy
import math

import numpy as np
import pytest
import torch

import optim_cases as oc
import optim_rows_cases as rc

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats on either side of a buffer: 256 bytes, so the payload stays 16-byte aligned
MARK = -7.5e30                # what the guard bands hold
T = 3                         # the step number of the one-step tests


def _hyper(hi, mode):
    """HYPERS[hi] of optim_cases; lazy mode takes no weight decay."""
    h = dict(oc.HYPERS[hi])
    if mode == "lazy":
        h["weight_decay"] = 0.0
    return h


class _Buf:
    """A float32 device buffer holding `a` between two guard bands."""

    def __init__(self, a, guard=GUARD):
        self.shape, self.guard = a.shape, guard
        self.full = torch.full((a.size + 2 * guard,), MARK, dtype=torch.float32, device="cuda")
        self.view = self.full[guard:guard + a.size]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        full = self.full.cpu().numpy()
        g = self.guard
        assert (full[:g] == np.float32(MARK)).all() and (full[len(full) - g:] == np.float32(MARK)).all(), "a guard band was written"
        return full[g:len(full) - g].reshape(self.shape).copy()


def _workspace():
    from grand_plus_amd import _native
    n = _native.optim_workspace_bytes() // 8
    full = torch.full((n + 16,), float("nan"), dtype=torch.float64, device="cuda")       # stale partials: NaN
    return full, full[8:8 + n]


def _ws_guards_intact(full):
    edge = torch.cat([full[:8], full[-8:]]).cpu()
    assert bool(torch.isnan(edge).all()), "the workspace's guard was written"


def _dense_step(p, m, v, g, h, t):
    """The reference: gp_clip_adam_step on a dense gradient, one step from (p, m, v).  Returns p, m, v, norm as numpy."""
    from grand_plus_amd import optim
    P, M, Vv, G = (torch.from_numpy(x.copy()).cuda() for x in (p, m, v, g))
    ws, norm = optim._buffers(P.device)
    step_size, rsqrt_bc2 = rc.corrections(h["lr"], oc.BETAS, t)
    optim._call(P.device, P, [(P, G, M, Vv)], 0, ws, norm, max_norm=h["clip"], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS,
                weight_decay=h["weight_decay"], step_size=step_size, rsqrt_bc2=rsqrt_bc2)
    return P.cpu().numpy(), M.cpu().numpy(), Vv.cpu().numpy(), norm.cpu().numpy()


def _rows_step(mode, p, m, v, dW, keys, h, t, dev=False, guard=GUARD, finite=True):
    """One step of the row-list entry points from (p, m, v): sqnorm into a workspace full of stale NaN, then the update.
    dev: the corrections by device pointer.  finite: the touched rows hold finite values, so no slot may end as NaN.  Every
    guard band is checked.  Returns p, m, v, norm as numpy and the sum of the workspace's slots."""
    from grand_plus_amd import _native
    from grand_plus_amd import optim_rows as orows
    V, H = p.shape
    L = _native.lib()
    bp, bm, bv, bg = _Buf(p, guard), _Buf(m, guard), _Buf(v, guard), _Buf(dW, guard)
    bn = _Buf(np.zeros(1, np.float32))
    k = torch.from_numpy(np.concatenate([[-99], keys, [-99]]).astype(np.int64)).cuda()      # a list of 0 keys still has an address
    kp = k.data_ptr() + 8
    ws_full, ws = _workspace()
    stream = torch.cuda.current_stream().cuda_stream
    _native.raise_for_status(L.gp_optim_rows_sqnorm(0, kp, len(keys), V, H, bg.ptr(), 0, ws.data_ptr(), stream))
    step_size, rsqrt_bc2 = rc.corrections(h["lr"], oc.BETAS, t)
    head = (0, bp.ptr(), bm.ptr(), bv.ptr(), bg.ptr(), kp, len(keys), V, H, orows.MODES[mode], h["clip"], h["lr"], oc.BETAS[0],
            oc.BETAS[1], oc.EPS, h["weight_decay"])
    if dev:
        corr = torch.tensor([step_size, rsqrt_bc2], dtype=torch.float32, device="cuda")
        rcode = L.gp_clip_adam_rows_dev(*head, corr.data_ptr(), corr.data_ptr() + 4, ws.data_ptr(), bn.ptr(), stream)
    else:
        rcode = L.gp_clip_adam_rows(*head, step_size, rsqrt_bc2, ws.data_ptr(), bn.ptr(), stream)
    _native.raise_for_status(rcode)
    torch.cuda.synchronize()
    _ws_guards_intact(ws_full)
    assert not finite or not bool(torch.isnan(ws).any()), "a workspace slot kept its stale value"
    assert rc.same_bits(bg.get(), dW), "dW was written"
    assert k[0] == -99 and k[-1] == -99
    return bp.get(), bm.get(), bv.get(), bn.get()[0], float(ws.sum().cpu())


def _check_against_dense(mode, V, H, keys, h, t, dev, exact_sums, seed, guard=GUARD, label=""):
    p, m, v = rc.state(V, H, seed)
    dW = rc.gradient(keys, V, H, seed + 1, exact_sums=exact_sums)
    tch = rc.touched(keys, V)
    assert np.isnan(dW[~tch]).all()
    pr, mr, vr, nr = _dense_step(p, m, v, rc.dense_gradient(dW, keys), h, t)
    po, mo, vo, no, sq = _rows_step(mode, p, m, v, dW, keys, h, t, dev=dev, guard=guard)
    ref64 = math.sqrt(rc.sq_norm64(dW, keys, V))
    assert abs(float(no) - ref64) <= 2.0 ** -23 * ref64, (label, float(no), ref64)
    if exact_sums or not h["clip"] > 0:                                 # the coefficient is bit-equal: everything is
        if exact_sums:
            assert sq == rc.sq_norm64(dW, keys, V) and rc.same_bits(no, nr), (label, float(no), float(nr))
        for name, o, r, old in (("p", po, pr, p), ("exp_avg", mo, mr, m), ("exp_avg_sq", vo, vr, v)):
            if mode == "exact":
                assert rc.same_bits(o, r), f"{label} {name}: exact mode is not the dense kernel"
            else:
                assert rc.same_bits(o[tch], r[tch]), f"{label} {name}: a touched row is not the dense kernel's"
                assert rc.same_bits(o[~tch], old[~tch]), f"{label} {name}: lazy mode changed an untouched row"
    if tch.any() and len(keys) > 0:
        assert not rc.same_bits(po[tch], p[tch])
    return po, mo, vo, no


@pytest.mark.parametrize("V,H", rc.SHAPES, ids=[f"V{v}-H{h}" for v, h in rc.SHAPES])
def test_both_modes_are_the_dense_kernel_on_every_key_list(V, H):
    """Every key list of the CPU grid, both modes; clipping on (HYPERS[0], gradients that sum exactly, so the coefficient is
    bit-equal) and off (HYPERS[1], random gradients), the corrections by value and by device pointer in turn."""
    n = 0
    for name, keys in rc.key_lists(V).items():
        for mode in rc.MODES:
            for hi, exact_sums in ((0, True), (1, False)):
                n += 1
                _check_against_dense(mode, V, H, keys, _hyper(hi, mode), T, dev=bool(n & 1) ^ bool(n & 4), exact_sums=exact_sums, seed=n,
                                     label=f"V{V} H{H} {name} {mode} h{hi}")


def test_the_windows_go_round_the_capped_grid_twice():
    """More windows than twice the grid cap times the waves of a workgroup: a small table, H = 1."""
    V, H = rc.STRIDE_SHAPE
    keys = rc.stride_keys()
    assert rc.touched(keys, V).all() and int(keys[0]) < 0 and int(keys[-1]) >= V
    for mode in rc.MODES:
        _check_against_dense(mode, V, H, keys, _hyper(0, mode), T, dev=False, exact_sums=True, seed=41, label=f"stride {mode}")
    # a table whose first and last rows alone are untouched, over the same list
    inner = np.clip(keys, 1, V - 2)
    for mode in rc.MODES:
        _check_against_dense(mode, V, H, inner, _hyper(1, mode), T, dev=True, exact_sums=False, seed=43, label=f"stride inner {mode}")


@pytest.mark.parametrize("V,H", [(64, 64), (5, 7), (4097, 1)])
def test_a_table_that_is_not_16_byte_aligned_gives_the_same_bits(V, H):
    keys = rc.key_lists(V)["n65"]
    for mode in rc.MODES:
        for hi, exact_sums in ((0, True), (1, False)):
            h = _hyper(hi, mode)
            a = _check_against_dense(mode, V, H, keys, h, T, dev=False, exact_sums=exact_sums, seed=9, guard=GUARD, label="aligned")
            b = _check_against_dense(mode, V, H, keys, h, T, dev=False, exact_sums=exact_sums, seed=9, guard=GUARD + 1, label="odd")
            assert all(rc.same_bits(x, y) for x, y in zip(a, b))


def test_five_repeats_give_equal_bits():
    """Random gradients and clipping on: the norm's partials are summed in a fixed order, so the coefficient repeats."""
    V, H = 585, 7
    keys = rc.key_lists(V)["n1025"]
    p, m, v = rc.state(V, H, 2)
    dW = rc.gradient(keys, V, H, 3)
    for mode in rc.MODES:
        runs = [_rows_step(mode, p, m, v, dW, keys, _hyper(0, mode), T, dev=bool(i & 1))[:4] for i in range(5)]
        for r in runs[1:]:
            assert all(rc.same_bits(x, y) for x, y in zip(r, runs[0])), mode


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_inf_and_nan_gradients_follow_the_dense_kernels_pattern(bad):
    """A non-finite gradient in one touched row.  Clipping off: it stays in its element.  Clipping on: the norm and the
    coefficient are non-finite, and in exact mode they reach the untouched rows exactly as 0.0f * coef does in the dense
    kernel; in lazy mode the untouched rows keep their bits."""
    V, H = 64, 65
    keys = rc.key_lists(V)["runs"]
    tch = rc.touched(keys, V)
    p, m, v = rc.state(V, H, 4)
    dW = rc.gradient(keys, V, H, 5)
    row = int(np.flatnonzero(tch)[1])
    dW[row, 3] = bad
    for hi in (0, 1):
        for mode in rc.MODES:
            h = _hyper(hi, mode)
            pr, mr, vr, nr = _dense_step(p, m, v, rc.dense_gradient(dW, keys), h, T)
            po, mo, vo, no, _ = _rows_step(mode, p, m, v, dW, keys, h, T, finite=False)
            assert rc.same_bits(no, nr) or (np.isnan(no) and np.isnan(nr))
            assert not np.isfinite(no)
            for o, r, old in ((po, pr, p), (mo, mr, m), (vo, vr, v)):
                sel = np.ones(V, bool) if mode == "exact" else tch
                assert (np.isnan(o[sel]) == np.isnan(r[sel])).all() and (np.isinf(o[sel]) == np.isinf(r[sel])).all()
                fin = np.isfinite(r[sel])
                assert rc.same_bits(o[sel][fin], r[sel][fin])
                if mode == "lazy":
                    assert rc.same_bits(o[~tch], old[~tch])
            if hi == 0 and mode == "exact" and math.isnan(bad):
                assert np.isnan(po[~tch]).all()                          # NaN coef: 0.0f * NaN reached every untouched row
            if hi == 1:
                assert np.isfinite(po[~tch]).all() and np.isfinite(np.delete(po[row], 3)).all() and not np.isfinite(mo[row, 3])


# ---- ClipAdam.set_row_grad
def _fill(rg, dW, keys):
    rg.values.copy_(torch.from_numpy(dW))
    rg.fill(torch.from_numpy(np.array(keys)).cuda())


def _sequence(V, H, steps, lists=("n65", "runs", "n1025", "out_of_range", "n64")):
    """`steps` (keys, dW) pairs: another key list every step, NaN outside the touched rows."""
    kl = rc.key_lists(V)
    return [(kl[lists[i % len(lists)]], rc.gradient(kl[lists[i % len(lists)]], V, H, 50 + i) * np.float32(oc.HYPERS[0]["gscale"]))
            for i in range(steps)]


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_five_chained_exact_steps_match_torch_adam_in_float64(capturable):
    """The table by its rows and a dense bias in one optimiser, against torch's clip_grad_norm_ + Adam(foreach=False) on the CPU
    fed the zero-filled dense gradients: test_gpu_optim.py's own bound, and the norm of every step."""
    from grand_plus_amd import ClipAdam, RowGrad
    from grand_plus_amd.step import StepState
    V, H = 585, 7
    h = oc.HYPERS[0]
    seq = _sequence(V, H, oc.STEPS)
    g = torch.Generator().manual_seed(5)
    init = [torch.from_numpy(rc.state(V, H, 1)[0]), torch.randn(H, generator=g) * 0.1]
    bias_grads = [torch.randn(H, generator=g) for _ in seq]
    dense_seq = [[torch.from_numpy(rc.dense_gradient(dW, keys)), bg] for (keys, dW), bg in zip(seq, bias_grads)]
    r64, t32 = oc.torch_run(init, dense_seq, h, torch.float64), oc.torch_run(init, dense_seq, h, torch.float32)
    table, bias = (torch.nn.Parameter(x.cuda()) for x in init)
    kw = dict(capturable=True, state=StepState("cuda")) if capturable else {}
    opt = ClipAdam([table, bias], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], clip_norm=h["clip"], **kw)
    rg = RowGrad(table)
    opt.set_row_grad(table, rg, "exact")
    for (keys, dW), bg, ref in zip(seq, bias_grads, r64["norm"]):
        _fill(rg, dW, keys)
        bias.grad = bg.cuda()
        if capturable:
            opt.step_state.advance(opt)
        norm = opt.step()
        assert abs(float(norm) - float(ref)) <= 2.0 ** -23 * float(ref)
        assert table.grad is None
    ours = {"param": [table, bias], "exp_avg": [opt.state[table]["exp_avg"], opt.state[bias]["exp_avg"]],
            "exp_avg_sq": [opt.state[table]["exp_avg_sq"], opt.state[bias]["exp_avg_sq"]]}
    oc.error_ratios(ours, t32, r64, "rows-exact")
    assert set(opt.state[table]) == {"step", "exp_avg", "exp_avg_sq"} and opt.state[table]["exp_avg"].shape == (V, H)


@pytest.mark.parametrize("capturable", [False, True], ids=["eager", "capturable"])
def test_five_chained_lazy_steps_match_the_float64_mirror(capturable):
    """The table as the optimiser's only parameter.  The bound is test_gpu_optim.py's, with the float32 mirror in torch32's
    place: 4 max|mirror32 - mirror64| + 2^-23 max|mirror64|.  Rows that no step touched keep their first bits."""
    from grand_plus_amd import ClipAdam, RowGrad
    from grand_plus_amd.step import StepState
    V, H = 585, 7
    h = _hyper(0, "lazy")
    seq = _sequence(V, H, oc.STEPS)
    p0, m0, v0 = rc.state(V, H, 1)
    zeros = np.zeros_like(p0)
    table = torch.nn.Parameter(torch.from_numpy(p0).cuda())
    kw = dict(capturable=True, state=StepState("cuda")) if capturable else {}
    opt = ClipAdam([table], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, clip_norm=h["clip"], **kw)
    rg = RowGrad(table)
    opt.set_row_grad(table, rg, "lazy")
    s64, s32 = (p0, zeros, zeros), (p0, zeros, zeros)
    ever = np.zeros(V, bool)
    for t, (keys, dW) in enumerate(seq, 1):
        _fill(rg, dW, keys)
        if capturable:
            opt.step_state.advance(opt)
        norm = opt.step()
        step_size, rsqrt_bc2 = rc.corrections(h["lr"], oc.BETAS, t)
        args = dict(lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=0.0, clip=h["clip"], step_size=step_size, rsqrt_bc2=rsqrt_bc2)
        *s64, n64 = rc.mirror_step("lazy", *s64, dW, keys, dtype=np.float64, **args)
        *s32, _ = rc.mirror_step("lazy", *s32, dW, keys, dtype=np.float32, **args)
        assert abs(float(norm) - float(n64)) <= 2.0 ** -23 * float(n64)
        ever |= rc.touched(keys, V)
    assert ever.any() and not ever.all()
    ours = (table.detach().cpu().numpy(), opt.state[table]["exp_avg"].cpu().numpy(), opt.state[table]["exp_avg_sq"].cpu().numpy())
    for name, o, a32, a64, first in zip(("param", "exp_avg", "exp_avg_sq"), ours, s32, s64, (p0, zeros, zeros)):
        e_ours, e_32, top = np.abs(o.astype(np.float64) - a64).max(), np.abs(a32.astype(np.float64) - a64).max(), np.abs(a64).max()
        bound = 4 * e_32 + 2.0 ** -23 * top
        print(f"rows-lazy {name}: ours {e_ours:.3e} mirror32 {e_32:.3e} bound {bound:.3e}")
        assert e_ours <= bound, (name, e_ours, bound)
        assert rc.same_bits(o[~ever], first[~ever]), name


def test_a_step_before_any_backward_is_refused_and_the_table_alone_steps():
    from grand_plus_amd import ClipAdam, RowGrad
    table = torch.nn.Parameter(torch.from_numpy(rc.state(5, 7, 1)[0]).cuda())
    opt = ClipAdam([table], lr=1e-2)
    rg = RowGrad(table)
    opt.set_row_grad(table, rg, "exact")
    before = table.detach().clone()
    with pytest.raises(RuntimeError, match="no backward has filled"):
        opt.step()
    assert not opt.state and torch.equal(table.detach(), before)
    keys = rc.key_lists(5)["edges"]
    _fill(rg, rc.gradient(keys, 5, 7, 3), keys)
    norm = opt.step()
    assert float(norm) > 0 and opt.state[table]["step"] == 1 and not torch.equal(table.detach(), before)
    assert bool(torch.isfinite(table).all())


@pytest.mark.parametrize("mode", rc.MODES)
def test_the_step_does_not_synchronise(mode):
    from grand_plus_amd import ClipAdam, RowGrad
    V, H = 64, 64
    table, bias = torch.nn.Parameter(torch.from_numpy(rc.state(V, H, 1)[0]).cuda()), torch.nn.Parameter(torch.zeros(H, device="cuda"))
    opt = ClipAdam([table, bias], lr=1e-2, clip_norm=0.1)
    rg = RowGrad(table)
    opt.set_row_grad(table, rg, mode)
    keys = rc.key_lists(V)["runs"]
    _fill(rg, rc.gradient(keys, V, H, 3), keys)
    bias.grad = torch.ones(H, device="cuda")
    opt.step()                                                          # the first step creates the state
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        norm = opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(norm) > 0 and bool(torch.isfinite(table).all())


@pytest.mark.parametrize("mode", rc.MODES)
def test_a_checkpoint_goes_both_ways_with_torch_adam(mode):
    from grand_plus_amd import ClipAdam, RowGrad
    V, H = 64, 7
    h = _hyper(1, mode)
    seq = _sequence(V, H, 3)

    def make(init):
        table = torch.nn.Parameter(init.clone())
        opt = ClipAdam([table], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], clip_norm=h["clip"])
        rg = RowGrad(table)
        opt.set_row_grad(table, rg, mode)
        return table, opt, rg

    table, opt, rg = make(torch.from_numpy(rc.state(V, H, 1)[0]).cuda())
    for keys, dW in seq[:2]:
        _fill(rg, dW, keys)
        opt.step()
    # ours -> torch.optim.Adam: the keys, shapes and the step count are torch's
    theirs_p = torch.nn.Parameter(table.detach().clone())
    theirs = torch.optim.Adam([theirs_p], lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], foreach=False)
    theirs.load_state_dict(copy.deepcopy(opt.state_dict()))        # load_state_dict keeps the tensors it is given
    st = theirs.state[theirs_p]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 2 and st["exp_avg"].shape == (V, H)
    assert torch.equal(st["exp_avg"], opt.state[table]["exp_avg"]) and torch.equal(st["exp_avg_sq"], opt.state[table]["exp_avg_sq"])
    # torch.optim.Adam -> ours: the third step continues bit for bit
    table2, opt2, rg2 = make(table.detach())
    opt2.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert opt2.state[table2]["step"] == 2
    keys, dW = seq[2]
    for o, r in ((opt, rg), (opt2, rg2)):
        _fill(r, dW, keys)
        o.step()
    assert torch.equal(table.detach().view(torch.int32), table2.detach().view(torch.int32))
    for key in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(opt.state[table][key].view(torch.int32), opt2.state[table2][key].view(torch.int32))
    assert opt.state[table]["step"] == opt2.state[table2]["step"] == 3
