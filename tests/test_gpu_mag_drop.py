"""MAG's device seed and its deterministic table gradient with input dropout on the GPU (csrc/mag_drop.hip and
csrc/mag_prop.hip; cases in tests/mag_drop_cases.py, audited on the CPU by tests/test_host_mag_drop.py).

The contract is bitwise: a call whose seed stands in device memory gives the forward of the int-seed call with that value,
also from a replayed graph, and W.grad of the deterministic backward equals the numpy float32 walk of the order contract of
csrc/mag_drop_abi.hpp, unchunked and in chunks.  Against float64 autograd the gradient is held to test_gpu_mag_det.py's
derived bound with n = S * contributions + the longest bag + S: every entry now adds up to S products."""
import ctypes

import numpy as np
import pytest
import torch

import mag_cases as mc
import mag_det_cases as dc
import mag_drop_cases as xc

pytestmark = pytest.mark.gpu

GUARD = 96                  # elements of guard band on each side of a buffer
BIG_SEED = 0xF00DFACE5EED0001       # above 2^63: the int64 tensor is read as a uint64


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _cuda(t):
    return None if t is None else t.cuda()


def _seed_tensor(value):
    return torch.tensor([value - 2 ** 64 if value >= 2 ** 63 else value], dtype=torch.int64).cuda()


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


def _det(c, **over):
    args = dict(deterministic=True, det_input_dropout=True, max_entries=c["E"]["total"] + 130)
    args.update(over)
    return _grad(c["P"], c["batch"], c["kw"], c["G"], **args)


def _hashed_case():
    """A case without input dropout whose DropNode mask is hashed from the seed: (P, batch, kw, keep on the host, G)."""
    c = dc.walk_case("h64_k32_s2")
    assert c["kw"]["keep"] is None and c["kw"]["input_droprate"] == 0.0 and c["kw"]["training"]
    keep = mc.node_keep(dc.SEED, c["S"], c["P"].S_rows * c["P"].K, c["kw"]["dropnode_rate"])
    return c["P"], c["batch"], c["kw"], keep, c["G"]


# ---- 1. the seed in device memory
@pytest.mark.parametrize("name", ["pin05_h65_s3", "pin05_s16", "hashed_dropnode"])
def test_a_tensor_seed_is_the_int_seed_of_the_same_value(name):
    """The forward bit for bit, the atomic backward within today's rule; with an explicit DropNode mask the seed keys the
    input dropout alone, in the third case the hashed DropNode mask alone."""
    if name == "hashed_dropnode":
        P, batch, kw, keep, G = _hashed_case()
        S = kw["samples"]
        _o, _t, dW64, dW_terms = mc.ref64(P, batch, S, kw["dropnode_rate"], 0.0, True, keep, dc.SEED, G)
        roundings = P.K + P.longest + S + 8
    else:
        c = xc.case(name)
        P, batch, kw, G = c["P"], c["batch"], c["kw"], c["G"]
        dW64, dW_terms, _n = xc.reference(name)
        roundings = mc.case(name)["roundings"]
    for value in (kw["seed"], BIG_SEED):
        seed = _seed_tensor(value)
        out_i, dW_i = _grad(P, batch, kw, G, seed=value, deterministic=False)
        out_t, dW_t = _grad(P, batch, kw, G, seed=seed, deterministic=False)
        assert _same(out_t, out_i) and bool(out_i.any()) and int(seed.cpu()) == (value if value < 2 ** 63 else value - 2 ** 64)
        assert _same(_call(P, batch, kw, seed=seed), out_i)                      # without a gradient too
        if value == kw["seed"]:
            for what, dW in (("tensor seed", dW_t), ("int seed", dW_i)):         # today's path is inside today's rule, and so is the new one
                mc.close(dW, dW64, dW_terms, roundings, f"{name}, atomic, {what}")
        else:
            assert not _same(out_i, _call(P, batch, kw))                         # another seed, another mask
            assert bool(torch.isfinite(dW_t).all()) and bool(dW_t.any())


def test_a_replayed_graph_draws_the_mask_of_the_seed_that_stands_there():
    c = xc.case("pin05_h65_s3")
    P, batch, kw = c["P"], c["batch"], dict(c["kw"])
    from grand_plus_amd import mag_prop_rows
    w, ip, ix, dt, col, val, filled, K = P.cuda()
    kw["keep"] = _cuda(kw["keep"])
    rows = _cuda(batch)
    seed = _seed_tensor(1)
    kw["seed"] = seed
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mag_prop_rows(w, ip, ix, dt, col, val, filled, K, rows, **kw)           # loads code, fills the allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mag_prop_rows(w, ip, ix, dt, col, val, filled, K, rows, **kw)
    got = []
    for value in (c["kw"]["seed"], BIG_SEED):
        seed.copy_(_seed_tensor(value))
        graph.replay()
        got.append(out.clone())
        assert _same(got[-1], _call(P, batch, c["kw"], seed=value)), hex(value)   # the eager int-seed call, bit for bit
    assert not _same(got[0], got[1])


# ---- 2. the deterministic gradient, bit for bit
@pytest.mark.parametrize("chunk", [None, xc.CHUNK])
@pytest.mark.parametrize("name", xc.CASES)
def test_weight_gradient_is_the_float32_walk_of_the_order_contract(name, chunk):
    c = xc.case(name)
    want = c["dW"] if chunk is None else c["dW_chunked"]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, dW = _det(c, overflow=flag, segment_chunk=chunk)
    assert dW.dtype == torch.float32 and bool(torch.isfinite(dW).all())
    diff = (dW.cpu() - want).abs().max()
    assert _same(dW.cpu(), want), f"{name}: max |d| {float(diff):.3e}"
    assert int(flag) == 0
    assert bool(dW.any()) == (name not in xc.DEGENERATE)                         # input_droprate = 1: all zeros
    # the forward is what it is without the keywords, the exact capacity gives the same gradient, and so does a device seed
    assert _same(out, _call(c["P"], c["batch"], c["kw"]))
    _, exact = _det(c, overflow=flag, segment_chunk=chunk, max_entries=max(c["E"]["total"], 1))
    assert _same(exact, dW) and int(flag) == 0
    _, dseed = _det(c, overflow=flag, segment_chunk=chunk, seed=_seed_tensor(c["kw"]["seed"]))
    assert _same(dseed, dW)


def test_a_device_seed_keys_the_hashed_dropnode_mask_of_the_deterministic_backward():
    """No input dropout, a hashed DropNode mask and a tensor seed: only gp_mag_prop_rows_backward_det_drop reads a device seed,
    so the call runs the per-sample contract with the mask factor 1."""
    P, batch, kw, keep, G = _hashed_case()
    want = xc.walk_dW32_drop(P, batch, kw["samples"], kw["dropnode_rate"], 0.0, True, keep, G, dc.SEED)
    total = dc.entry_order(P, batch)["total"]
    for det_drop in (False, True):
        _, dW = _grad(P, batch, kw, G, seed=_seed_tensor(dc.SEED), deterministic=True, max_entries=total, det_input_dropout=det_drop)
        assert _same(dW.cpu(), want)


def test_a_short_buffer_sets_the_flag_and_gives_the_walk_truncated_at_max_entries():
    c = xc.case("pin05_h65_s3")
    total = c["E"]["total"]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.use_deterministic_algorithms(True)                                     # torch's mode selects the path as the keyword does
    try:
        _, dW = _grad(c["P"], c["batch"], c["kw"], c["G"], max_entries=total, overflow=flag, det_input_dropout=True)
    finally:
        torch.use_deterministic_algorithms(False)
    assert _same(dW.cpu(), c["dW"]) and int(flag) == 0
    for cap in (total - 1, total // 2, 1):
        for chunk in (None, xc.CHUNK):
            flag.zero_()
            _, short = _det(c, max_entries=cap, overflow=flag, segment_chunk=chunk)
            want = xc.walk_dW32_drop(*c["args"], max_entries=cap, chunk=chunk)
            assert int(flag) == 1 and _same(short.cpu(), want), (cap, chunk)     # the entries below the capacity, and only they
    _det(c, max_entries=1)                                                       # no overflow tensor: a private one, never read


def test_five_backwards_are_bitwise_equal_and_a_row_grad_gets_the_same_rows_and_keys():
    from grand_plus_amd.optim_rows import RowGrad
    c = xc.case("pin05_h64_k32")
    P = c["P"]
    runs = [_det(c) for _ in range(5)]
    for out, dW in runs[1:]:
        assert _same(out, runs[0][0]) and _same(dW, runs[0][1])
    assert _same(runs[0][1].cpu(), c["dW"])
    E = c["E"]
    cap = E["total"] + 130
    want_keys = np.concatenate([np.sort(E["keys"], kind="stable"), np.full(130, P.V)])
    for chunk, want in ((None, c["dW"]), (xc.CHUNK, c["dW_chunked"])):
        W = P.W.cuda().requires_grad_(True)
        rg = RowGrad(W)
        rg.values.fill_(float("nan"))
        out = _call(P, c["batch"], c["kw"], W=W, deterministic=True, det_input_dropout=True, max_entries=cap, row_grad=rg, segment_chunk=chunk)
        (out * c["G"].cuda()).sum().backward()
        assert W.grad is None and rg.filled() and rg.n_sorted == cap
        assert (rg.keys.cpu().numpy() == want_keys).all()
        touched = torch.from_numpy(np.bincount(E["keys"], minlength=P.V + 1)[:P.V] > 0)
        assert _same(rg.values.cpu()[touched], want[touched]) and bool(torch.isnan(rg.values.cpu()[~touched]).all())


def test_guard_bands_around_the_scratch_and_the_gradient_stay_intact():
    """gp_mag_prop_rows_backward_det_drop itself, on U [S, B * K, H], inv [S, B] and dW [V, H] between bands of a NaN pattern,
    H = 65 and a batch that repeats a row: every write lands inside its buffer."""
    from grand_plus_amd import _native
    c = xc.case("pin05_h65_s3")
    P, S = c["P"], c["S"]
    _, ip, ix, dt, col, val, filled, K = P.cuda()
    batch, keep, G = c["batch"].cuda(), c["kw"]["keep"].cuda(), c["G"].cuda().contiguous()
    B, cap = batch.numel(), c["E"]["total"] + 7
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = _native.lib()
    base = torch.empty(B * K + 1, dtype=torch.int64, device="cuda")
    keys = torch.empty(cap, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert L.gp_mag_det_keys(0, P.V, ip.data_ptr(), ix.data_ptr(), P.N, col.data_ptr(), filled.data_ptr(), P.S_rows, K, batch.data_ptr(), B,
                             cap, base.data_ptr(), keys.data_ptr(), flag.data_ptr(), stream) == 0
    skeys, order = torch.sort(keys, stable=True)
    sizes = {"U": S * B * K * P.H, "inv": S * B, "dW": P.V * P.H}
    poison = float("nan")
    for chunk in (0, xc.CHUNK):
        bufs = {k: torch.full((GUARD + n + GUARD,), poison, device="cuda") for k, n in sizes.items()}
        bufs["dW"][GUARD:GUARD + sizes["dW"]] = 0.0
        scratch = torch.empty(max(1, 2 * ((cap + 63) // 64) * P.H), device="cuda")
        ptr = {k: b.data_ptr() + 4 * GUARD for k, b in bufs.items()}
        rc = L.gp_mag_prop_rows_backward_det_drop(
            0, G.data_ptr(), P.V, P.H, ip.data_ptr(), ix.data_ptr(), dt.data_ptr(), P.N, col.data_ptr(), val.data_ptr(), filled.data_ptr(),
            P.S_rows, K, batch.data_ptr(), B, S, c["kw"]["dropnode_rate"], c["kw"]["input_droprate"], 1, ctypes.c_uint64(c["kw"]["seed"]),
            None, keep.data_ptr(), col.numel(), base.data_ptr(), order.data_ptr(), skeys.data_ptr(), cap, ptr["U"], ptr["inv"], ptr["dW"],
            chunk, scratch.data_ptr() if chunk else None, 4 * scratch.numel() if chunk else 0, stream)
        assert rc == 0
        torch.cuda.synchronize()
        for k, b in bufs.items():
            b = b.cpu()
            assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + sizes[k]:]).all()), f"{k}: a guard band was written"
        dW = bufs["dW"].cpu()[GUARD:GUARD + sizes["dW"]].reshape(P.V, P.H)
        assert _same(dW, c["dW"] if chunk == 0 else c["dW_chunked"]) and int(flag) == 0
        assert bool(torch.isfinite(bufs["inv"].cpu()[GUARD:GUARD + sizes["inv"]]).all())


# ---- 3. against float64
@pytest.mark.parametrize("name", xc.CASES)
def test_weight_gradient_matches_float64_autograd_under_the_derived_bound(name):
    c = xc.case(name)
    dW64, _terms, _n = xc.reference(name)
    bound = xc.bound(name)
    for what, chunk in (("unchunked", None), ("chunked", xc.CHUNK)):
        _, dW = _det(c, segment_chunk=chunk)
        err = (dW.double().cpu() - dW64).abs()
        ratio = float((err / bound).max())
        print(f"[mag drop] {name} {what}: worst error / bound {ratio:.3g}, max |d| {float(err.max()):.3e}")
        assert ratio <= 1.0


# ---- 4. today's paths
def test_the_keyword_changes_nothing_where_no_mask_is_drawn_and_the_atomic_path_keeps_its_rule():
    """det_input_dropout=True at input_droprate = 0, and in eval mode, is the plain deterministic call bit for bit; the
    int-seed atomic call with input dropout is inside mag_cases.close as before."""
    for name in ("h7_k5_s3", "h64_k32_s2", "eval"):
        c = dc.walk_case(name)
        cap = c["E"]["total"] + 130
        for chunk in (None, xc.CHUNK):
            plain = _grad(c["P"], c["batch"], c["kw"], c["G"], deterministic=True, max_entries=cap, segment_chunk=chunk)
            keyed = _grad(c["P"], c["batch"], c["kw"], c["G"], deterministic=True, max_entries=cap, segment_chunk=chunk, det_input_dropout=True)
            assert _same(plain[0], keyed[0]) and _same(plain[1], keyed[1]), (name, chunk)
            if chunk is None:
                assert _same(plain[1].cpu(), c["dW"])                            # and both are today's walk
    c = dc.walk_case("eval")                                                     # eval mode with a rate: no mask either
    kw = dict(c["kw"], input_droprate=0.5)
    keyed = _grad(c["P"], c["batch"], kw, c["G"], deterministic=True, max_entries=c["E"]["total"], det_input_dropout=True)
    assert _same(keyed[1].cpu(), c["dW"])
    with pytest.raises(ValueError, match="does not support input dropout"):     # without the keyword the refusal stays
        x = xc.case("pin05_h65_s3")
        _grad(x["P"], x["batch"], x["kw"], x["G"], deterministic=True, max_entries=x["E"]["total"])
    for name in ("pin05_h65_s3", "pin05_h64_k32", "eps_scale"):
        m = mc.case(name)
        _o64, _t, dW64, dW_terms = m["ref"]
        _, dW = _grad(m["P"], m["batch"], dict(m["kw"], keep=m["keep"]), m["G"], deterministic=False)
        mc.close(dW, dW64, dW_terms, m["roundings"], f"{name}, atomic")


def test_forward_and_backward_do_not_synchronise():
    c = xc.case("pin05_h64_k32")
    P = c["P"]
    from grand_plus_amd import mag_prop_rows
    w, ip, ix, dt, col, val, filled, K = P.cuda()
    W = P.W.cuda().requires_grad_(True)
    G, batch = c["G"].cuda(), _cuda(c["batch"])
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    cap = c["E"]["total"] + 130
    kw = dict(c["kw"], keep=_cuda(c["kw"]["keep"]), seed=_seed_tensor(c["kw"]["seed"]))
    for chunk, want in ((None, c["dW"]), (xc.CHUNK, c["dW_chunked"])):
        args = dict(deterministic=True, det_input_dropout=True, max_entries=cap, overflow=flag, segment_chunk=chunk, **kw)
        warm = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, batch, **args)
        (warm * G).sum().backward()                                              # loads code, fills the allocator
        W.grad = None
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = mag_prop_rows(W, ip, ix, dt, col, val, filled, K, batch, **args)
            (out * G).sum().backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert _same(W.grad.cpu(), want) and int(flag) == 0
        W.grad = None
