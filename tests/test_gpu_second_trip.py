"""Every capped grid of the newer kernels taken round its grid-stride loop twice (cases in
tests/second_trip_cases.py, which tests/test_host_second_trip.py holds to the caps in the sources).

The gradients are compared BIT FOR BIT with a vectorised float64 bincount: the inputs are built so that every partial sum
is exact in float32, whatever the order (second_trip_cases.py states the rules).  Every test also looks at the index
range of the second trip on its own, first, so that a failure names the trip.  No test here changes a tolerance: the
optimiser, the masks, the selection, the snapshot and the head keep the rules of their own test modules."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import evaluate_cases as ec
import optim_cases as oc
import second_trip_cases as st
import step_cases as sc
from mag_cases import node_keep
from mlp_block_cases import hashed_keep
from test_gpu_optim import _assert_norm, _bits_equal, _optimizer, _state_of

pytestmark = pytest.mark.gpu

GUARD = 96
G64, G32 = -0x5A5A5A5A5A5A5A5B, 0x5A5A5A5A


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _assert_gradient(got, want, sorted_keys, what):
    """got (CUDA) is bitwise want (CPU, [n_dest, 1]); first on the destinations that only the gather's second trip reaches."""
    got = got.cpu()
    only = torch.from_numpy(st.second_trip_only(sorted_keys, want.shape[0]))
    assert int(only.sum()) >= 2
    assert bool((got[only] != 0).all()), f"{what}: a destination of the second trip's windows was left at zero"
    assert _bits_equal(got[only], want[only]), f"{what}: the second trip's destinations differ: {got[only].reshape(-1)} vs {want[only].reshape(-1)}"
    bad = got.view(torch.int32) != want.view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} destinations differ, the first at {int(torch.nonzero(bad)[0, 0])}"


# ---- case 1: mag_det, mag_prop's atomic backward and the MagOp gather
def _mag_grad(c, **over):
    from grand_plus_amd import mag_prop_rows
    w, ip, ix, dt, col, val, filled, K = c["P"].cuda()
    W = w.requires_grad_(True)
    out = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, None, **c["kw"], **over)
    out.backward(c["G"].cuda())
    return W.grad


def test_mag_deterministic_table_gradient_past_five_caps():
    """mag_slot_len_kernel (2 099 200 slots against 2 097 152), mag_keys_kernel's slot loop (against 32 768),
    mag_slot_grad_kernel (1 049 600 batch rows against 8 192) and gather_sum_kernel<MagOp> (the entry total + 1 000
    sentinels against 4 194 240 sorted positions)."""
    c = st.mag_case()
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    dW = _mag_grad(c, deterministic=True, max_entries=c["total"] + st.MAG_SLACK, overflow=flag)
    assert int(flag) == 0
    _assert_gradient(dW, c["dW"], c["sorted_keys"], "mag_prop_rows, deterministic")


def test_mag_atomic_backward_past_its_grid_gives_the_same_bits():
    """mag_prop_rows_backward_kernel over 1 049 600 batch rows against 8 192 workgroups: its sums are exact too."""
    c = st.mag_case()
    _assert_gradient(_mag_grad(c, deterministic=False), c["dW"], c["sorted_keys"], "mag_prop_rows, atomic")


def test_mag_keys_slot_base_and_tail_past_the_grid():
    """gp_mag_det_keys as tests/test_gpu_mag_det.py calls it: slot_base, the keys and the tail of 1 000 sentinels equal the
    vectorised entry order, between guard bands."""
    from grand_plus_amd import _native
    c = st.mag_case()
    P, n_slots, cap = c["P"], st.MAG_B * st.MAG_K, c["total"] + st.MAG_SLACK
    _, ip, ix, _dt, col, _val, _filled, K = P.cuda()
    base = torch.full((GUARD + n_slots + 1 + GUARD,), G64, dtype=torch.int64, device="cuda")
    keys = torch.full((GUARD + cap + GUARD,), G64, dtype=torch.int64, device="cuda")
    flag = torch.full((GUARD + 1 + GUARD,), G32, dtype=torch.int32, device="cuda")
    flag[GUARD] = 4
    rc = _native.lib().gp_mag_det_keys(0, P.V, ip.data_ptr(), ix.data_ptr(), P.N, col.data_ptr(), None, P.S_rows, K, None, P.S_rows, cap,
                                  base.data_ptr() + 8 * GUARD, keys.data_ptr() + 8 * GUARD, flag.data_ptr() + 4 * GUARD, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    base, keys, flag = base.cpu().numpy(), keys.cpu().numpy(), flag.cpu().numpy()
    for buf, n, g in ((base, n_slots + 1, G64), (keys, cap, G64), (flag, 1, G32)):
        assert (buf[:GUARD] == g).all() and (buf[GUARD + n:] == g).all(), "a guard band was written"
    base, keys = base[GUARD:GUARD + n_slots + 1], keys[GUARD:GUARD + cap]
    one = st.MAG_LEN_ONE_TRIP
    assert (base[one:] == c["slot_base"][one:]).all(), "slot_base differs on the length kernel's second trip"
    assert (base == c["slot_base"]).all()
    first = int(c["slot_base"][st.MAG_KEYS_ONE_TRIP])                            # the first entry of the key kernel's second trip
    assert (keys[first:c["total"]] == c["keys"][first:]).all(), "the keys differ on the key kernel's later trips"
    assert (keys[:c["total"]] == c["keys"]).all()
    assert (keys[c["total"]:] == P.V).all() and cap - c["total"] == st.MAG_SLACK  # the tail is all sentinel
    assert flag[GUARD] == 4


# ---- case 3: scatter_det, rows form
def test_rows_deterministic_backward_past_both_caps():
    """rows_inv_den_kernel (65 576 batch rows against 65 535 workgroups) and gather_sum_kernel<RowsOp>: in this mode the
    wrapper sorts every one of the B * K = 4 196 864 slots, which is past the 4 194 240 positions of one trip, so B stays
    at 65 535 + 41."""
    from grand_plus_amd.augment import _rows_det_order, random_prop_rows
    c = st.rows_case()
    col, val, filled = c["col"].cuda(), c["val"].cuda(), c["filled"].cuda()
    _order, keys = _rows_det_order(col, filled, st.ROWS_K, None, st.ROWS_N)
    assert keys.numel() == st.ROWS_B * st.ROWS_K > st.GATHER_ONE_TRIP and np.array_equal(keys.cpu().numpy(), c["sorted_keys"])
    x = torch.zeros((st.ROWS_N, 1), device="cuda", requires_grad=True)
    out = random_prop_rows(x, col, val, filled, st.ROWS_K, training=False, deterministic=True)
    out.backward(c["G"].cuda())
    _assert_gradient(x.grad, c["grad"], c["sorted_keys"], "random_prop_rows, deterministic")


# ---- case 4: scatter_det, bag form
def test_bag_deterministic_backward_past_both_caps():
    """bag_inv_den_kernel (262 181 bags against 262 140 waves) and gather_sum_kernel<BagOp> (4 194 896 sorted positions),
    through the C entry point on a gradient inside guard rows, so that the bad-id count can be read."""
    from grand_plus_amd import _native
    from grand_plus_amd.embedding import _det_order, _Layout
    c = st.bag_case()
    M, V, nnz = st.BAG_M, st.BAG_V, st.BAG_M * st.BAG_LEN
    L = _Layout(c["indptr"].cuda(), M, None, None, M, c["indices"].cuda(), c["data"].cuda())
    order, keys, rows = _det_order(L, nnz, V)
    assert order.numel() == nnz > st.GATHER_ONE_TRIP and np.array_equal(keys.cpu().numpy(), c["sorted_keys"])
    gbuf = torch.zeros((V + 4, 1), device="cuda")
    G = c["G"].cuda()
    n_bad = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    inv = torch.empty(_native.scatter_bag_workspace_bytes(M) // 4, device="cuda")
    _native.raise_for_status(_native.lib().gp_embedding_bag_backward_det(
        0, G.data_ptr(), V, 1, *L.args(), 0.0, 0, ctypes.c_uint64(0), None, gbuf[2:V + 2].data_ptr(), n_bad.data_ptr(),
        order.data_ptr(), keys.data_ptr(), rows.data_ptr(), nnz, inv.data_ptr(), _stream()))
    assert int(n_bad.item()) == 0
    assert bool((inv[st.BAG_DEN_ONE_TRIP:] == 1.0).all()), "a bag of the denominator kernel's second trip"
    assert bool((inv == 1.0).all())
    assert torch.count_nonzero(gbuf[:2]) == 0 and torch.count_nonzero(gbuf[V + 2:]) == 0
    _assert_gradient(gbuf[2:V + 2], c["dW"], c["sorted_keys"], "embedding bag, deterministic")


# ---- case 5: the optimiser
def _second_trip_slices(state):
    """The elements of the four chunks that workgroups 0 .. 3 take on their second trip, as error_ratios takes them."""
    second = st.stride_chunks()[2]
    return {key: [state[key][t].detach().reshape(-1)[a:a + n] for t, a, n in second] for key in ("param", "exp_avg", "exp_avg_sq")}


def test_clipadam_steps_1028_chunks_and_then_one_element_on_a_stale_workspace():
    """optim_sqnorm_kernel and the Adam branch of optim_clip_adam_kernel over 1 028 chunks against 1 024 workgroups, clipping
    active, 2 steps, under §7g's rule (error_ratios, _assert_norm) -- on the second trip's four chunks alone, then on
    everything.  Directly afterwards one element is stepped on the same device: its norm is |g| exactly, so no partial
    of the large call survived in the workspace, neither in torch's cached block nor in one handed over explicitly."""
    from grand_plus_amd import _native
    from grand_plus_amd.optim import _buffers, _call
    hi, steps = 0, oc.STRIDE_STEPS
    init, seq = oc.inputs("stride", hi, steps)
    r64, t32 = oc.reference("stride", hi, steps)
    params = oc.device_params("stride", init)
    opt = _optimizer(params, hi)
    norms = []
    for grads in seq:
        oc.set_grads(params, grads)
        norms.append(opt.step())
    solo_init, solo_seq = oc.inputs("solo", hi, 1)
    (solo,) = oc.device_params("solo", solo_init)
    oc.set_grads([solo], solo_seq[0])
    g_abs = solo.grad.abs().reshape(())
    assert float(g_abs) > 0.0
    assert _bits_equal(_optimizer([solo], hi).step(), g_abs)
    ws, norm = _buffers(solo.device)
    _call(solo.device, params[1], [(None, p.grad, None, None) for p in params], _native.GP_OPTIM_CLIP_ONLY, ws, norm)
    _assert_norm(norm.clone(), r64["norm"][-1])                                  # all 1 024 slots hold a partial now
    _call(solo.device, solo, [(None, solo.grad, None, None)], _native.GP_OPTIM_CLIP_ONLY, ws, norm)
    assert _bits_equal(norm, g_abs)
    ours = _state_of(opt, params)
    oc.error_ratios(_second_trip_slices(ours), _second_trip_slices(t32), _second_trip_slices(r64), "stride-h0, second trip")
    oc.error_ratios(ours, t32, r64, "stride-h0")
    for got, ref in zip(norms, r64["norm"]):
        _assert_norm(got, ref)
    assert all(opt.state[p]["step"] == steps for p in params)


def test_clip_grad_norm_scales_1028_chunks_by_the_fp32_coefficient():
    """The clip-only branch of optim_clip_adam_kernel past the grid: bitwise g * coef, as test_gpu_optim.py holds it."""
    from grand_plus_amd import clip_grad_norm
    init, seq = oc.inputs("stride", 0, oc.STRIDE_STEPS)
    params = oc.device_params("stride", init)
    oc.set_grads(params, seq[0])
    before = [p.grad.clone() for p in params]
    max_norm = 0.1
    norm = clip_grad_norm(params, max_norm)
    _assert_norm(norm, oc.reference("stride", 0, oc.STRIDE_STEPS)[0]["norm"][0])
    coef = torch.tensor(max_norm, dtype=torch.float32) / (norm.cpu() + torch.tensor(1e-6, dtype=torch.float32))
    assert coef.dtype == torch.float32 and float(coef) < 1.0
    for t, a, n in st.stride_chunks()[2]:
        assert _bits_equal(params[t].grad[a:a + n], before[t][a:a + n] * coef.cuda()), f"second trip: tensor {t} from {a}"
    for p, g in zip(params, before):
        assert _bits_equal(p.grad, g * coef.cuda())


def test_capturable_clipadam_past_the_grid_equals_the_host_number_step():
    """The _dev template of optim_clip_adam_kernel past the grid.  At step 1 both bias corrections are the float32 of
    lr / (1 - beta1) and 1 / sqrt(1 - beta2) on the device as on the host, so the step is bitwise the host-number one."""
    from grand_plus_amd import ClipAdam, StepState
    hi = 0
    h = oc.HYPERS[hi]
    init, seq = oc.inputs("stride", hi, oc.STRIDE_STEPS)
    kw = dict(lr=h["lr"], betas=oc.BETAS, eps=oc.EPS, weight_decay=h["weight_decay"], clip_norm=h["clip"])
    grads = [g.cuda() for g in seq[0]]
    state = StepState("cuda", 1, 1.0, 10)
    params = oc.device_params("stride", init)
    opt = ClipAdam(params, capturable=True, state=state, **kw)
    host_params = oc.device_params("stride", init)
    host_opt = ClipAdam(host_params, **kw)
    state.advance(opt)
    for p, q, g in zip(params, host_params, grads):
        p.grad = q.grad = g
    norm, host_norm = opt.step(), host_opt.step()
    assert state.read().tick == 1 and _bits_equal(norm, host_norm)
    a, b = _state_of(opt, params), _state_of(host_opt, host_params)
    for key in a:
        for (t, lo, n), x, y in zip(st.stride_chunks()[2], _second_trip_slices(a)[key], _second_trip_slices(b)[key]):
            assert _bits_equal(x, y), f"second trip: {key} of tensor {t} from {lo}"
        for x, y in zip(a[key], b[key]):
            assert _bits_equal(x, y), key


# ---- case 6: the masks
def test_masks_past_the_grid_with_the_segment_boundary_on_the_second_trip():
    """step_masks_kernel over 1 590 800 items against 4 096 x 256: a rows segment of S = 16, K = 64, B = 1 025 (1 049 600
    items) and a layer segment of width 33 behind it, against the host mirrors as test_gpu_captured_step.py compares them.
    Unfilled slots, rows outside the batch and a 4 KiB tail behind each buffer keep their 0xAA."""
    from grand_plus_amd import StepState
    from grand_plus_amd._common import step_seed
    from grand_plus_amd.step import layer_segment, rows_segment, step_masks
    S, K, B, R, F, p, tail, layer = st.MASK_S, st.MASK_K, st.MASK_B, st.MASK_ROWS, st.MASK_WIDTH, 0.5, 4096, 1
    filled, rows = st.mask_case()
    L = R * K
    state = StepState("cuda", sc.BASE_SEED, sc.LAM, sc.WARMUP)
    state.advance()
    state.advance()
    seed = step_seed(sc.BASE_SEED, 2)
    node = torch.full((S * L + tail,), 0xAA, dtype=torch.uint8, device="cuda")
    lay = torch.full((S * B * F + tail,), 0xAA, dtype=torch.uint8, device="cuda")
    step_masks(state, [rows_segment(node[:S * L].view(S, L), rows.cuda(), filled.cuda(), K, S, p),
                       layer_segment(lay[:S * B * F].view(S, B, F), layer, p)])
    torch.cuda.synchronize()
    in_batch = torch.zeros(R, dtype=torch.bool)
    in_batch[rows.long()] = True
    live = (in_batch[:, None] & (torch.arange(K)[None, :] < filled[:, None])).reshape(-1)
    want = torch.where(live[None, :], node_keep(seed, S, L, p), torch.full((S, L), 0xAA, dtype=torch.uint8))
    got = node.cpu()
    # the second trip: items from 1 048 576 on are sample 15's batch positions from 1 009 on, then the whole layer segment
    b0 = (st.STEP_ONE_TRIP - (S - 1) * B * K) // K
    assert (S - 1) * B * K < st.STEP_ONE_TRIP and b0 == 1009
    late = (rows[b0:].long()[:, None] * K + torch.arange(K)[None, :]).reshape(-1)
    assert torch.equal(got[:S * L].view(S, L)[S - 1, late], want[S - 1, late]), "the rows segment differs on the second trip"
    got_lay = lay.cpu()
    assert torch.equal(got_lay[:S * B * F].view(S, B, F), hashed_keep(seed, layer, S, B, F, p)), "the layer segment (second trip)"
    assert torch.equal(got[:S * L].view(S, L), want)
    assert bool((got[S * L:] == 0xAA).all()) and bool((got_lay[S * B * F:] == 0xAA).all())
    assert bool((want == 0xAA).any()) and state.read().tick == 2


# ---- case 7: the selection
def test_fit_select_draws_a_whole_pool_past_the_grid():
    """fit_select_kernel over 3 + 1 048 876 selections against 4 096 x 256: the unlabelled half is a permutation of the
    pool, and agrees with perm_index on the first 64, the 128 round selection index 1 048 576 and the last 64."""
    from grand_plus_amd import StepState
    from grand_plus_amd._common import _FIT_UNLABEL_MUL, _M64, _mix, perm_index, step_seed
    from grand_plus_amd.fit import Sampler, fit_select
    base, guard, mark = 0x5EED0FACADE, 512, -7777
    n_train, n_unlabel, total = st.SELECT_TRAIN, st.SELECT_UNLABEL, st.SELECT_TOTAL
    s = Sampler(n_train, n_unlabel, n_train, n_unlabel, 0xC0FFEE)
    state = StepState("cuda", base, 0.0, 1.0)
    state.advance()
    assert s.shape(1) == (n_train, n_unlabel)
    sel = torch.full((guard + total + guard,), mark, dtype=torch.int64, device="cuda")
    flag = torch.full((2 * guard + 1,), mark, dtype=torch.int32, device="cuda")
    flag[guard] = 0
    fit_select(state, s, n_train, sel[guard:guard + total], flag[guard:guard + 1])
    sel, flag = sel.cpu().numpy(), flag.cpu().numpy()
    assert (sel[:guard] == mark).all() and (sel[guard + total:] == mark).all(), "the selection's guard bands were written"
    assert (flag[:guard] == mark).all() and (flag[guard + 1:] == mark).all() and flag[guard] == 0
    got = sel[guard:guard + total]
    key = _mix((step_seed(base, 1) & _M64) ^ _FIT_UNLABEL_MUL)
    for i in st.SELECT_PROBES.tolist():
        assert got[i] - n_train == perm_index(key, n_unlabel, i - n_train), f"selection index {i} (the second trip starts at {st.FIT_ONE_TRIP})"
    assert np.array_equal(got[:n_train], s.labelled(1))
    assert np.array_equal(np.sort(got[n_train:]), np.arange(n_train, n_train + n_unlabel))


# ---- case 8: the snapshot
def test_fit_snapshot_copies_three_tensors_past_the_grid():
    """fit_snapshot_kernel over 5 + 1 052 673 + 7 words against 4 096 x 256: the entry boundary into the third tensor lies
    on the second trip.  Every destination is bitwise its source between unwritten guard words; copy_now = 0 writes nothing."""
    from grand_plus_amd import _native
    from grand_plus_amd._native import GpFitCopy, GpFitTrack
    words, guard, mark = st.SNAPSHOT_WORDS, 256, 0x5A5A5A5A
    src_at = np.concatenate([[0], np.cumsum(words)])
    dst_at = [guard * (i + 1) + int(src_at[i]) for i in range(3)]
    gen = torch.Generator(device="cuda").manual_seed(8)
    src = torch.randint(-2 ** 31, 2 ** 31 - 1, (int(src_at[-1]),), generator=gen, device="cuda", dtype=torch.int64).to(torch.int32)
    dst = torch.full((dst_at[-1] + words[-1] + guard,), mark, dtype=torch.int32, device="cuda")
    table = (GpFitCopy * 3)(*[GpFitCopy(src=src.data_ptr() + 4 * int(src_at[i]), dst=dst.data_ptr() + 4 * dst_at[i], n_words=words[i])
                              for i in range(3)])

    def snapshot(copy_now):
        track = torch.frombuffer(bytearray(bytes(GpFitTrack(best_loss=float("inf"), copy_now=copy_now))), dtype=torch.int64).cuda()
        _native.raise_for_status(_native.lib().gp_fit_snapshot(0, track.data_ptr(), table, 3, _stream()))
        torch.cuda.synchronize()
        return dst.cpu().numpy()

    assert (snapshot(0) == np.int32(mark)).all()
    got, host = snapshot(1), src.cpu().numpy()
    expect = np.full_like(got, np.int32(mark))
    for i in range(3):
        expect[dst_at[i]:dst_at[i] + words[i]] = host[src_at[i]:src_at[i + 1]]
    late = st.FIT_ONE_TRIP - int(src_at[1])                                      # the second tensor's first word of the second trip
    assert np.array_equal(got[dst_at[1] + late:], expect[dst_at[1] + late:]), "the second trip: the end of tensor 2, tensor 3, the guards"
    assert np.array_equal(got, expect)


# ---- case 9: the head
@pytest.mark.parametrize("C", st.HEAD_C)
def test_head_past_the_grid_with_ignored_and_bad_labels(C):
    """eval_head_kernel over 262 177 rows against 65 535 x 4 waves, some labels ignored and some out of range: the checks
    of test_gpu_evaluate.test_head_matches_torch, first on the last 37 rows (the second trip) alone."""
    from grand_plus_amd import eval_head, eval_reduce
    z, y, y_valid = st.head_case(C)
    n, one = st.HEAD_N, st.HEAD_ONE_TRIP
    zd = z.cuda()
    buf = eval_head(zd, y.cuda())
    loss, acc, counts = eval_reduce(buf)
    pred = torch.argmax(z, dim=1)
    valid = y_valid != st.HEAD_IGNORE
    flag = torch.where(valid, (pred == y).to(torch.uint8), torch.where(y == st.HEAD_IGNORE, torch.tensor(ec.IGNORED, dtype=torch.uint8),
                                                                        torch.tensor(ec.BAD, dtype=torch.uint8)))
    logp = Fn.log_softmax(z.double(), dim=1)
    per_row = torch.where(valid, -logp.gather(1, y_valid.clamp(min=0)[:, None])[:, 0], torch.zeros(n, dtype=torch.float64))
    got_pred, got_flag, got_nll = buf.pred.cpu().long(), buf.flag.cpu(), buf.nll.cpu().double()
    for what, rows in (("the second trip's 37 rows", slice(one, n)), ("all rows", slice(0, n))):
        assert torch.equal(got_pred[rows], pred[rows]), what
        assert torch.equal(got_flag[rows], flag[rows]), what
        assert float((got_nll[rows] - per_row[rows]).abs().max()) <= 1e-5 * float(per_row[rows].abs().max()) + 1e-6, what
        assert not bool(got_nll[rows][~valid[rows]].any()), what
    n_correct = int(((pred == y) & valid).sum())
    assert counts.tolist() == [int(valid.sum()), n_correct, int((y == st.HEAD_IGNORE).sum()), int((~valid).sum() - (y == st.HEAD_IGNORE).sum())]
    assert float(acc) == float(np.float32(n_correct / n))
    ref64 = float(Fn.nll_loss(logp, y_valid, ignore_index=st.HEAD_IGNORE))
    ec.assert_loss(float(loss), ec.nll32_on(zd, y_valid.cuda(), st.HEAD_IGNORE), ref64, f"head C={C} n={n}")
