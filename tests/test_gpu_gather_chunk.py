"""The chunked deterministic segment sums on the GPU (csrc/gather_chunk.hpp; the contract, the cases and their
audit are tests/gather_chunk_cases.py and tests/test_host_gather_chunk.py): the order contract of gather_chunk_abi.hpp
pinned bit for bit in the bag, rows and MAG forms, segments of at most C entries equal to the unchunked gradient bit for
bit, run-to-run equality, guard bands round the gradient and the scratch, no host synchronisation, float64 under the
derived bound (n + 8) * 2^-24 * sum|terms| + 1e-7 (recursive summation of n terms in any grouping, at most eight further
roundings per term), the captured MAG step, and the second trip of the grid-stride loop."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import gather_chunk_cases as gcc
import mag_cases as mc
import mag_det_cases as dc
import second_trip_cases as st
from augment_cases import ref_grad, rows_to_coo

pytestmark = pytest.mark.gpu
f32 = np.float32


def _bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _close_hub(got, ref, terms, n):
    got, ref, terms = got.double().cpu(), ref.double().cpu(), terms.double().cpu()
    bad = (got - ref).abs() > (n + 8) * 2.0 ** -24 * terms + 1e-7
    assert not bool(bad.any()), f"{int(bad.sum())} elements off; max |d| {float((got - ref).abs().max()):.3e}"


# ---------------------------------------------------------------------------------------------- the bag form
def _bag_grad(name, H, chunk):
    """dW of embedding_bag over the case's entries: every entry a bag of its own with weight 1, eval mode."""
    from grand_plus_amd.embedding import embedding_bag
    e = gcc.entries(name, H)
    V, n = e["n_dest"], len(e["dest"])
    attr = torch.from_numpy(np.where(e["dest"] >= 0, e["dest"], V + 3)).cuda()    # the dead entries: an id outside the table
    W = torch.zeros((V, H), device="cuda", requires_grad=True)
    embedding_bag(W, attr, torch.arange(n).cuda(), torch.ones(n).cuda(), training=False, validate=False, deterministic=True,
                  n_out=n, segment_chunk=chunk).backward(torch.from_numpy(e["G"]).cuda())
    return W.grad


@pytest.mark.parametrize("H", [1, 64, 65, 257])
def test_bag_cases_hold_the_contract_bit_for_bit(H):
    """Every case of gather_chunk_cases.CASES that lists this width: one destination of 63 .. 4 097 entries at sorted position
    0, 1, 63 and 64 under C = 64, C = 256, the adjacent long segments, a long segment that ends the list and one that runs
    into the sentinel tail, and the all-sentinel list.  257 columns take a second pass of kCols slabs."""
    ran = 0
    for name, c in gcc.CASES.items():
        if H not in c["H"]:
            continue
        got = _bag_grad(name, H, c["C"])
        assert _bits(got.cpu(), torch.from_numpy(gcc.expected(name, H))), name
        ran += 1
    assert ran >= 24


def test_segments_of_at_most_c_entries_are_the_unchunked_bag_gradient_and_longer_ones_are_not():
    for name in ("c64_n63_at1", "c64_n64_at63", "c256_n256_at1"):
        c = gcc.CASES[name]
        assert max(c["segs"]) <= c["C"]
        assert _bits(_bag_grad(name, 65, c["C"]), _bag_grad(name, 65, None)), name
    assert not _bits(_bag_grad("c64_n129_at1", 65, 64), _bag_grad("c64_n129_at1", 65, None))
    # C = 4096 holds the 4 097 entries in two chunks; the second is one entry, which is the plain walk (gather_chunk_cases)
    assert _bits(_bag_grad("c64_n4097_at1", 65, 4096), _bag_grad("c64_n4097_at1", 65, None))


def test_empty_batches_give_zero_gradients():
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag_csr
    W = torch.zeros((9, 70), device="cuda", requires_grad=True)
    ip = torch.tensor([0, 0, 0, 3]).cuda()
    ix, dt = torch.tensor([1, 2, 3], dtype=torch.int32).cuda(), torch.ones(3).cuda()
    for nodes in (torch.zeros(0, dtype=torch.int64), torch.tensor([0, 1, 1])):     # no bags at all, and bags that are all empty
        W.grad = None
        out = embedding_bag_csr(W, ip, ix, dt, nodes=nodes.cuda(), training=False, deterministic=True, segment_chunk=64)
        out.backward(torch.ones_like(out))
        assert out.shape == (nodes.numel(), 70) and W.grad.shape == W.shape and torch.count_nonzero(W.grad) == 0
    x = torch.zeros((9, 70), device="cuda", requires_grad=True)
    col = torch.zeros(8, dtype=torch.int32).cuda()
    out = random_prop_rows(x, col, torch.ones(8, dtype=torch.float64).cuda(), None, 4, batch_rows=torch.zeros(0, dtype=torch.int32).cuda(),
                           training=False, deterministic=True, segment_chunk=64)
    out.backward(torch.ones_like(out))
    assert out.shape == (0, 70) and torch.count_nonzero(x.grad) == 0
    # every slot unfilled: an all-sentinel order
    out = random_prop_rows(x, col, torch.ones(8, dtype=torch.float64).cuda(), torch.zeros(2, dtype=torch.int32).cuda(), 4, training=False,
                           deterministic=True, segment_chunk=64)
    out.backward(torch.ones_like(out))
    assert torch.count_nonzero(x.grad) == 0


def _guarded(call, n_dest, width, n_sorted, C, want, sorted_keys, what):
    """One chunked C entry point on a gradient and an exact-size scratch that lie inside guard rows: call(dst, scratch,
    scratch_bytes) runs it.  The guards keep their fill, the gradient has the contract's bits, and the scratch rows that
    were written are those of the long segments' chunks (gather_chunk_cases.mapping_model) and no others."""
    from grand_plus_amd import _native, gather_chunk as gc
    nbytes = gc.scratch_bytes(n_sorted, C, width)
    guard = 2 * width
    gbuf = torch.full((n_dest + 4, width), 7.0, device="cuda")
    gbuf[2:n_dest + 2] = 0
    sbuf = torch.full((nbytes // 4 + 2 * guard,), 123.0, device="cuda")
    _native.raise_for_status(call(gbuf[2:n_dest + 2].data_ptr(), sbuf[guard:].data_ptr(), nbytes))
    assert bool((gbuf[:2] == 7.0).all()) and bool((gbuf[n_dest + 2:] == 7.0).all()), what
    assert bool((sbuf[:guard] == 123.0).all()) and bool((sbuf[guard + nbytes // 4:] == 123.0).all()), what
    assert _bits(gbuf[2:n_dest + 2].cpu(), torch.from_numpy(want)), what
    touched = (sbuf[guard:guard + nbytes // 4].reshape(-1, width) != 123.0).any(1).nonzero().flatten().tolist()
    _, written = gcc.mapping_model(sorted_keys, np.zeros((len(sorted_keys), 1), f32), n_dest, C)
    assert written and touched == written, what


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_guard_bands_round_the_bag_gradient_and_its_scratch_keep_their_fill():
    """gp_embedding_bag_backward_det_chunked on the adjacent long segments (both scratch rows of one span in use) and on a
    long segment that ends the list."""
    from grand_plus_amd import _native
    from grand_plus_amd.embedding import _det_order, _Layout
    H, C = 65, 64
    for name in ("adjacent_at10", "long_ends_the_list"):
        e = gcc.entries(name, H)
        V, n = e["n_dest"], len(e["dest"])
        attr = torch.from_numpy(np.where(e["dest"] >= 0, e["dest"], V + 3)).cuda()
        L = _Layout(torch.arange(n + 1).cuda(), n, None, None, n, attr, torch.ones(n).cuda())
        order, keys, rows = _det_order(L, n, V)
        assert np.array_equal(keys.cpu().numpy(), e["sorted_keys"])
        inv = torch.empty(n, device="cuda")
        G = torch.from_numpy(e["G"]).cuda()
        _guarded(lambda dst, scratch, nbytes: _native.lib().gp_embedding_bag_backward_det_chunked(
            0, G.data_ptr(), V, H, *L.args(), 0.0, 0, ctypes.c_uint64(0), None, dst, None, order.data_ptr(), keys.data_ptr(),
            rows.data_ptr(), n, inv.data_ptr(), C, scratch, nbytes, _stream()), V, H, n, C, gcc.expected(name, H), e["sorted_keys"], name)


def test_guard_bands_round_the_rows_gradient_and_its_scratch_keep_their_fill():
    """gp_random_prop_rows_backward_det_chunked on the rows hub at F = 257 (two passes of kCols slabs): width = F,
    n_sorted = B * K."""
    from grand_plus_amd import _native
    from grand_plus_amd.augment import _rows_det_order
    F, C = 257, 64
    col, val, X, G, keep = _rows_hub(F)
    cc, vc, Gc, kc = col.reshape(-1).cuda(), val.reshape(-1).cuda(), G.cuda(), keep.reshape(-1).cuda()
    order, keys = _rows_det_order(cc, None, ROWS_K, None, ROWS_N)
    n = keys.numel()
    assert n == ROWS_B * ROWS_K
    inv = torch.empty(_native.scatter_rows_workspace_bytes(ROWS_S, ROWS_B) // 4, device="cuda")
    _guarded(lambda dst, scratch, nbytes: _native.lib().gp_random_prop_rows_backward_det_chunked(
        0, Gc.data_ptr(), ROWS_B, F, cc.data_ptr(), vc.data_ptr(), None, ROWS_K, None, ROWS_S, 0.5, 1, ctypes.c_uint64(0),
        kc.data_ptr(), cc.numel(), dst, ROWS_N, order.data_ptr(), keys.data_ptr(), n, inv.data_ptr(), C, scratch, nbytes, _stream()),
        ROWS_N, F, n, C, _rows_walk(col, val, G, keep, 0.5, C, ROWS_N), keys.cpu().numpy(), "rows")


def test_guard_bands_round_the_mag_gradient_and_its_scratch_keep_their_fill():
    """gp_mag_prop_rows_backward_det_chunked on the MAG hub with max_entries above the total: n_sorted = max_entries, the
    scratch sized from it, a sentinel tail of 37 positions behind the entries."""
    from grand_plus_amd import _native
    from grand_plus_amd.mag import _Call
    C = 64
    P, G, keep, E, _ = _mag_hub()
    cap = E["total"] + 37
    W, indptr, indices, data, col, val, filled, K = P.cuda()
    call = _Call((indptr, indices, data, col, val, filled, None, keep.reshape(-1).cuda()), MAG_B, K, MAG_B, MAG_S, 0.5, 0.0, True, 0)
    slot_base = torch.empty(MAG_B * K + 1, dtype=torch.int64, device="cuda")
    keys = torch.empty(cap, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    _native.raise_for_status(_native.lib().gp_mag_det_keys(0, MAG_V, indptr.data_ptr(), indices.data_ptr(), MAG_N, col.data_ptr(), None, MAG_B,
                                                      K, None, MAG_B, cap, slot_base.data_ptr(), keys.data_ptr(), flag.data_ptr(), _stream()))
    sorted_keys, order = torch.sort(keys, stable=True)
    want, walk_keys = _mag_want()
    assert np.array_equal(sorted_keys.cpu().numpy()[:E["total"]], walk_keys) and bool((sorted_keys[E["total"]:] == MAG_V).all())
    U = torch.empty((MAG_B * K, MAG_H), device="cuda")
    inv = torch.empty((MAG_S, MAG_B), device="cuda")
    Gc = G.cuda()
    _guarded(lambda dst, scratch, nbytes: _native.lib().gp_mag_prop_rows_backward_det_chunked(
        0, Gc.data_ptr(), MAG_V, MAG_H, *call.args(), slot_base.data_ptr(), order.data_ptr(), sorted_keys.data_ptr(), cap, U.data_ptr(),
        inv.data_ptr(), dst, C, scratch, nbytes, _stream()), MAG_V, MAG_H, cap, C, want, sorted_keys.cpu().numpy(), "mag")
    assert int(flag.item()) == 0


# ---------------------------------------------------------------------------------------------- the rows form
ROWS_B, ROWS_K, ROWS_S, ROWS_N = 130, 4, 2, 40


@functools.lru_cache(maxsize=None)
def _rows_hub(F):
    """Node 7 in slot 0 of every row (a segment of 130 positions: three chunks at C = 64), the other slots on other nodes."""
    g = torch.Generator().manual_seed(900 + F)
    col = torch.randint(8, ROWS_N, (ROWS_B, ROWS_K), generator=g, dtype=torch.int32)
    col[:, 0] = 7
    val = torch.rand((ROWS_B, ROWS_K), generator=g, dtype=torch.float64) + 0.1
    X = torch.randn((ROWS_N, F), generator=g)
    G = torch.randn((ROWS_S, ROWS_B, F), generator=g) * 10.0 ** torch.randint(-3, 4, (1, ROWS_B, 1), generator=g)
    keep = (torch.rand((ROWS_S, ROWS_B * ROWS_K), generator=g) >= 0.5).to(torch.uint8)
    return col, val, X, G, keep


def _rows_walk(col, val, G, keep, p, C, n_nodes):
    """features.grad by the contract: c_e = sum_s (g[s, b] * inv_{s,b}) * w'_{s,e}, s ascending from 0.0f (scatter_det.hip's
    expression, denominators summed over k in order), the slots sorted by column, gather_chunk_cases.chunked_sum."""
    S, B, F = G.shape
    K = col.shape[1]
    scale = f32(1.0) / (f32(1.0) - f32(p))
    w = val.numpy().astype(f32)[None] * np.where(keep.numpy().reshape(S, B, K) != 0, scale, f32(0.0)).astype(f32)
    den = np.zeros((S, B), f32)
    for k in range(K):
        den = (den + w[:, :, k]).astype(f32)
    inv = (f32(1.0) / (den + f32(1e-12))).astype(f32)
    g = G.numpy().astype(f32)
    terms = np.zeros((B * K, F), f32)
    for s in range(S):
        gi = (g[s] * inv[s][:, None]).astype(f32)                                # [B, F]
        terms = (terms + (gi[:, None, :] * w[s][:, :, None]).astype(f32).reshape(B * K, F)).astype(f32)
    keys = col.numpy().reshape(-1).astype(np.int64)
    order = np.argsort(keys, kind="stable")
    return gcc.chunked_sum(keys[order], terms[order], n_nodes, C)


@pytest.mark.parametrize("F", [7, 257])
def test_rows_hub_holds_the_contract_with_explicit_and_seeded_masks(F):
    from grand_plus_amd.augment import random_prop_rows
    col, val, X, G, keep = _rows_hub(F)
    seed = 0xC0FFEE + F
    hashed = mc.node_keep(seed, ROWS_S, ROWS_B * ROWS_K, 0.5)
    cc, vc = col.reshape(-1).cuda(), val.reshape(-1).cuda()
    for mask, kw in ((keep, dict(keep=keep.reshape(-1).cuda())), (hashed, dict(seed=seed))):
        grads = []
        for chunk in (64, None):
            x = X.cuda().requires_grad_(True)
            random_prop_rows(x, cc, vc, None, ROWS_K, dropnode_rate=0.5, training=True, samples=ROWS_S, deterministic=True,
                             segment_chunk=chunk, **kw).backward(G.cuda())
            grads.append(x.grad)
        want = _rows_walk(col, val, G, mask, 0.5, 64, ROWS_N)
        assert _bits(grads[0].cpu(), torch.from_numpy(want))
        # every node but 7 has fewer than 64 slots: its row is the unchunked one, bit for bit; node 7's is not
        assert int(torch.bincount(col.reshape(-1).long()).sort().values[-2]) < 64
        others = torch.arange(ROWS_N) != 7
        assert _bits(grads[0][others.cuda()], grads[1][others.cuda()]) and not _bits(grads[0][7], grads[1][7])
        idx, cols, scores, kp = rows_to_coo(col, val, torch.full((ROWS_B,), ROWS_K), ROWS_K, torch.arange(ROWS_B), mask)
        ref, terms = ref_grad(X, scores, idx, 0.5, True, kp, G, cols=cols)
        _close_hub(grads[0], ref, terms, ROWS_B)


# ---------------------------------------------------------------------------------------------- the MAG form
MAG_V, MAG_H, MAG_K, MAG_B, MAG_N, MAG_S, MAG_HUB = 50, 8, 4, 40, 30, 2, 5


@functools.lru_cache(maxsize=None)
def _mag_hub():
    """Every node's bag holds attribute 5 first and two others: with B = 40 full rows of K = 4 the hub's segment has 160
    positions, three chunks at C = 64.  (P, G, keep, the entry order, terms per entry)."""
    g = torch.Generator().manual_seed(77)
    indices = torch.randint(6, MAG_V, (MAG_N, 3), generator=g, dtype=torch.int32)
    indices[:, 0] = MAG_HUB
    P = mc.Problem(W=torch.randn((MAG_V, MAG_H), generator=g), indptr=torch.arange(MAG_N + 1, dtype=torch.int64) * 3,
                   indices=indices.reshape(-1), data=torch.rand(MAG_N * 3, generator=g) + 0.05,
                   col=torch.randint(0, MAG_N, (MAG_B, MAG_K), generator=g, dtype=torch.int32),
                   val=torch.rand((MAG_B, MAG_K), generator=g, dtype=torch.float64) + 0.1, filled=None, K=MAG_K, N=MAG_N, V=MAG_V,
                   H=MAG_H, S_rows=MAG_B, longest=3)
    G = torch.randn((MAG_S, MAG_B, MAG_H), generator=g) * 10.0 ** torch.randint(-3, 4, (1, MAG_B, 1), generator=g)
    keep = (torch.rand((MAG_S, MAG_B * MAG_K), generator=g) >= 0.5).to(torch.uint8)
    E = dc.entry_order(P, None)
    U = dc.slot_grads32(P, None, MAG_S, 0.5, True, keep, G)
    terms = (U[E["slot"]] * E["d"][:, None]).astype(f32)
    assert E["total"] == MAG_B * MAG_K * 3 and int((E["keys"] == MAG_HUB).sum()) == 160
    return P, G, keep, E, terms


def _mag_want(max_entries=None, C=64):
    P, G, keep, E, terms = _mag_hub()
    n = E["total"] if max_entries is None else min(E["total"], max_entries)
    keys = E["keys"][:n]
    order = np.argsort(keys, kind="stable")
    return gcc.chunked_sum(keys[order], terms[:n][order], MAG_V, C), np.sort(keys, kind="stable")


def _mag_call(chunk, max_entries, row_grad=False, overflow=None):
    from grand_plus_amd.mag import mag_prop_rows
    from grand_plus_amd.optim_rows import RowGrad
    P, G, keep, E, _ = _mag_hub()
    W, *rest = P.cuda()
    W.requires_grad_(True)
    rg = RowGrad(W) if row_grad else None
    out = mag_prop_rows(W, *rest, samples=MAG_S, dropnode_rate=0.5, training=True, keep=keep.reshape(-1).cuda(), deterministic=True,
                        max_entries=max_entries, overflow=overflow, row_grad=rg, segment_chunk=chunk)
    out.backward(G.cuda())
    return W, rg


def test_mag_hub_holds_the_contract_dense_as_a_row_list_and_past_the_capacity():
    P, G, keep, E, _ = _mag_hub()
    total = E["total"]
    want, sorted_keys = _mag_want()
    W, _ = _mag_call(64, total + 37)
    assert _bits(W.grad.cpu(), torch.from_numpy(want))
    plain, _ = _mag_call(None, total + 37)
    counts = dc.contributions(P, None)
    short = counts <= 64
    assert int(counts[MAG_HUB]) == 160 and int(short.sum()) == MAG_V - 1
    assert _bits(W.grad[short.cuda()], plain.grad[short.cuda()]) and not _bits(W.grad[MAG_HUB], plain.grad[MAG_HUB])
    assert _bits(_mag_call(256, total + 37)[0].grad, plain.grad)                 # every segment within C = 256: the unchunked bits
    # float64 under the derived bound
    _, _, dW, dW_terms = mc.ref64(P, None, MAG_S, 0.5, 0.0, True, keep, 0, G)
    _close_hub(W.grad, dW, dW_terms, 160)
    # the row list: the touched rows of `values` have those bits, and the key list is the unchunked call's
    Wr, rg = _mag_call(64, total + 37, row_grad=True)
    Wp, rg_plain = _mag_call(None, total + 37, row_grad=True)
    assert Wr.grad is None and torch.equal(rg.keys, rg_plain.keys) and rg.n_sorted == total + 37
    assert np.array_equal(rg.keys.cpu().numpy()[:total], sorted_keys) and bool((rg.keys[total:] == MAG_V).all())
    touched = torch.from_numpy(np.unique(sorted_keys)).cuda()
    assert _bits(rg.values[touched].cpu(), torch.from_numpy(want)[touched.cpu()])
    # one entry short: the flag is set, and the entries below the capacity still sum by the contract
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    Wo, _ = _mag_call(64, total - 1, overflow=flag)
    assert int(flag.item()) == 1
    assert _bits(Wo.grad.cpu(), torch.from_numpy(_mag_want(total - 1)[0]))


# ---------------------------------------------------------------------------------------------- all three forms
def test_short_segments_are_the_unchunked_gradient_in_every_form():
    """The inputs of test_gpu_deterministic_backward.py (every destination has at most 61 contributions) and a MAG walk case
    under the smallest C that holds its longest segment."""
    from grand_plus_amd.mag import mag_prop_rows
    from test_gpu_deterministic_backward import _bag_check, _rows_grad, _rows_inputs
    from test_gpu_embedding import _bags
    col, val, filled, X, g, rows, G = _rows_inputs(65, 2, seed=12)
    kw = dict(dropnode_rate=0.5, training=True, seed=5, samples=2, deterministic=True)
    assert int(torch.bincount(col[rows.long()].reshape(-1).long()).max()) <= 64
    a, _ = _rows_grad(X, col, val, filled, col.shape[1], rows, G, segment_chunk=64, **kw)
    b, _ = _rows_grad(X, col, val, filled, col.shape[1], rows, G, **kw)
    assert _bits(a, b) and float(a.abs().sum()) > 0
    attr_idx, node_idx, attr_data, gb = _bags(500, 80, seed=3)
    assert int(torch.bincount(attr_idx).max()) <= 64
    W = torch.randn((500, 65), generator=gb).cuda()
    keep = (torch.rand((attr_idx.numel(), 65), generator=gb) >= 0.5).to(torch.uint8)
    Gb = torch.randn((int(node_idx[-1]) + 1, 65), generator=gb)
    a, _ = _bag_check(W, attr_idx, node_idx, attr_data, 0.5, True, keep, Gb, deterministic=True, segment_chunk=64)
    b, _ = _bag_check(W, attr_idx, node_idx, attr_data, 0.5, True, keep, Gb, deterministic=True)
    assert _bits(a, b)
    c = dc.walk_case("h7_k5_s3")
    longest = int(dc.contributions(c["P"], c["batch"]).max())
    C = max(64, 1 << (longest - 1).bit_length())
    kw = dict(c["kw"])
    kw["keep"] = None if kw["keep"] is None else kw["keep"].reshape(-1).cuda()
    grads = []
    for chunk in (C, None):
        Wm, *rest = c["P"].cuda()
        Wm.requires_grad_(True)
        mag_prop_rows(Wm, *rest, batch_rows=None if c["batch"] is None else c["batch"].cuda(), deterministic=True,
                      max_entries=c["E"]["total"] + 5, segment_chunk=chunk, **kw).backward(c["G"].cuda())
        grads.append(Wm.grad)
    assert _bits(*grads) and _bits(grads[0].cpu(), c["dW"])


def test_five_backwards_are_bitwise_equal_and_hold_float64_at_4097_entries():
    """test_gpu_deterministic_backward.py's hubs (one destination of 4 097 contributions) at C = 64 and C = 1024."""
    from grand_plus_amd.embedding import embedding_bag
    from test_gpu_deterministic_backward import _hub_bags, _hub_rows, _rows_grad
    from test_gpu_embedding import emb_ref
    col, val, filled, X, G = _hub_rows()
    B = col.shape[0]
    idx, cols, scores, kp = rows_to_coo(col, val, filled, 1, torch.arange(B), torch.ones((1, B, 1), dtype=torch.uint8))
    ref, terms = ref_grad(X, scores, idx, 0.0, False, kp[0], G, cols=cols)
    W, attr_idx, node_idx, attr_data, Gb = _hub_bags()
    n = Gb.shape[0]
    ws = W.double().clone().requires_grad_(True)
    (emb_ref(ws, attr_idx, node_idx, attr_data, 0.0, False, None) * Gb.double()).sum().backward()
    wa = W.double().abs().requires_grad_(True)
    (emb_ref(wa, attr_idx, node_idx, attr_data, 0.0, False, None) * Gb.double().abs()).sum().backward()
    for C in (64, 1024):
        grads = [_rows_grad(X, col, val, filled, 1, None, G, training=False, deterministic=True, segment_chunk=C)[0] for _ in range(5)]
        _close_hub(grads[0], ref, terms, B)
        assert all(_bits(grads[0], x) for x in grads[1:])
        grads = []
        for _ in range(5):
            Wc = W.cuda().requires_grad_(True)
            embedding_bag(Wc, attr_idx.cuda(), node_idx.cuda(), attr_data.cuda(), training=False, deterministic=True,
                          segment_chunk=C).backward(Gb.cuda())
            grads.append(Wc.grad)
        _close_hub(grads[0], ws.grad, wa.grad, n)
        assert all(_bits(grads[0], x) for x in grads[1:])
    W5 = [_mag_call(64, _mag_hub()[3]["total"])[0].grad for _ in range(5)]
    assert all(_bits(W5[0], x) for x in W5[1:])


def test_no_host_synchronisation():
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag
    from grand_plus_amd.mag import mag_prop_rows
    col, val, X, G, keep = _rows_hub(7)
    x = X.cuda().requires_grad_(True)
    cc, vc, Gc = col.reshape(-1).cuda(), val.reshape(-1).cuda(), G.cuda()
    e = gcc.entries("adjacent_at10", 65)
    V, n = e["n_dest"], len(e["dest"])
    attr = torch.from_numpy(np.where(e["dest"] >= 0, e["dest"], V + 3)).cuda()
    node, ones, Gb = torch.arange(n).cuda(), torch.ones(n).cuda(), torch.from_numpy(e["G"]).cuda()
    Wb = torch.zeros((V, 65), device="cuda", requires_grad=True)
    P, Gm, keep_m, E, _ = _mag_hub()
    Wm, *rest = P.cuda()
    Wm.requires_grad_(True)
    km, Gmc = keep_m.reshape(-1).cuda(), Gm.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        random_prop_rows(x, cc, vc, None, ROWS_K, dropnode_rate=0.5, training=True, seed=1, samples=ROWS_S, deterministic=True,
                         segment_chunk=64).backward(Gc)
        embedding_bag(Wb, attr, node, ones, training=False, validate=False, deterministic=True, n_out=n, segment_chunk=64).backward(Gb)
        mag_prop_rows(Wm, *rest, samples=MAG_S, dropnode_rate=0.5, training=True, keep=km, deterministic=True,
                      max_entries=E["total"], segment_chunk=64).backward(Gmc)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()
    assert float(x.grad.abs().sum()) > 0 and float(Wm.grad.abs().sum()) > 0
    assert _bits(Wb.grad.cpu(), torch.from_numpy(gcc.expected("adjacent_at10", 65)))


# ---------------------------------------------------------------------------------------------- the captured step
HUB_COPIES = 12


@functools.lru_cache(maxsize=None)
def _hub_world():
    """test_gpu_mag_step.py's world with attribute 5 put HUB_COPIES times at the head of every node's bag."""
    import test_gpu_mag_step as ms
    seeds, col, val, filled, (indptr, indices, data), labels, longest = ms.world()
    rng = np.random.default_rng(29)
    lens = (indptr[1:] - indptr[:-1]).numpy()
    new_idx, new_data = [], []
    for v in range(ms.N):
        lo, hi = int(indptr[v]), int(indptr[v + 1])
        new_idx += [MAG_HUB] * HUB_COPIES + indices[lo:hi].tolist()
        new_data += (rng.random(HUB_COPIES) + 0.05).astype(f32).tolist() + data[lo:hi].tolist()
    ip = torch.from_numpy(np.concatenate([[0], np.cumsum(lens + HUB_COPIES)]).astype(np.int64))
    return seeds, col, val, filled, (ip, torch.tensor(new_idx, dtype=torch.int32), torch.tensor(new_data, dtype=torch.float32)), labels


def _hub_segment(sel):
    """How many sorted positions the hub attribute has in the batch of a selection."""
    import test_gpu_mag_step as ms
    seeds, col, val, filled, attrs, labels = _hub_world()
    rows = np.concatenate([sel[0], ms.N_TRAIN + sel[1]])
    return int(filled.numpy()[rows].clip(0, ms.K).sum()) * HUB_COPIES


def _hub_step(capture, chunk, table_step):
    import optim_cases as oc
    import test_gpu_mag_step as ms
    from grand_plus_amd import ClipAdam, MagTrainStep, StepState, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    seeds, col, val, filled, attrs, labels = _hub_world()
    row = torch.from_numpy(np.repeat(seeds, ms.K).astype(np.int32))
    rm = RowMatrix(seeds, ms.K, row.cuda(), col.cuda(), val.cuda(), filled.cuda(), ms.N)
    torch.manual_seed(7)
    m = MagMLP(ms.V, ms.C, ms.H, 2, True, 0.0, 0.5, True).cuda().train()
    decay = 0.0 if table_step == "lazy" else 5e-4                              # the lazy mode takes no weight decay
    opt = ClipAdam(mag_trained_parameters(m), lr=ms.LR, betas=oc.BETAS, eps=oc.EPS, weight_decay=decay, clip_norm=0.1, capturable=True,
                   state=StepState("cuda"))
    ts = MagTrainStep(m, opt, rm, *(a.cuda() for a in attrs), labels.cuda(), seeds[:ms.N_TRAIN], seeds[ms.N_TRAIN:], samples=ms.S,
                      dropnode_rate=ms.P_NODE, lam=ms.LAM, warmup=ms.WARMUP, tem=ms.TEM, conf=ms.CONF, kind="l2", seed=ms.BASE_SEED,
                      capture=capture, deterministic=True, table_step=table_step, segment_chunk=chunk)
    return ts, m, opt


@pytest.mark.parametrize("table_step", [None, "exact", "lazy"])
def test_three_replayed_chunked_steps_equal_three_eager_steps_bit_for_bit(table_step):
    import test_gpu_mag_step as ms
    cap, eag, plain = _hub_step(True, 64, table_step), _hub_step(False, 64, table_step), _hub_step(False, None, table_step)
    assert cap[0].segment_chunk == 64 and plain[0].segment_chunk is None
    differs = False
    for t in range(1, 4):
        sel = ms.selection(t)
        assert _hub_segment(sel) > 64, "the hub's segment has to span more than one chunk"
        rc, re, rp = cap[0].step(*sel), eag[0].step(*sel), plain[0].step(*sel)
        ms._assert_twins((rc, cap[1], cap[2]), (re, eag[1], eag[2]), f"step {t}")
        differs |= not ms._same(cap[1].embeds.weight, plain[1].embeds.weight)
        assert np.isfinite(float(rc.loss))
    cap[0].check_entries_flag()
    assert differs                                  # the chunked order is another order: the hub row's bits moved the table


# ---------------------------------------------------------------------------------------------- the second trip
def test_rows_backward_takes_the_grid_stride_loop_round_twice():
    """second_trip_cases.rows_case(): 4 196 864 sorted positions against 4 194 240 per trip, some 256 slots a node (four
    chunks at C = 64), and a reference that is exact in any order: the chunked gradient is `grad` bit for bit."""
    from grand_plus_amd.augment import random_prop_rows
    c = st.rows_case()
    assert st.ROWS_B * st.ROWS_K > st.GATHER_ONE_TRIP
    col, val, filled = c["col"].cuda(), c["val"].cuda(), c["filled"].cuda()
    x = torch.zeros((st.ROWS_N, 1), device="cuda", requires_grad=True)
    random_prop_rows(x, col, val, filled, st.ROWS_K, training=False, deterministic=True, segment_chunk=64).backward(c["G"].cuda())
    assert _bits(x.grad.cpu(), c["grad"])
    late = st.second_trip_only(c["sorted_keys"], st.ROWS_N)
    assert late.sum() >= 3 and float(c["grad"][torch.from_numpy(late)].abs().sum()) > 0
