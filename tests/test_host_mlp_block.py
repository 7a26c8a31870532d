"""CPU companion of tests/test_gpu_mlp_block.py: the cases of mlp_block_cases.py themselves, with no GPU.

Headroom: the block restated with the same torch ops in float32 stays within ROOM = 0.1 of every bound of every case
(LOOSE_ROOM = 0.5 for the B = 2 cases under BN|TRAINING, which are on the loose rule), so a correct kernel can pass.
Sensitivity: each deliberate mistake of mlp_block_cases.MUTANTS, built into the float64 formulas, moves an asserted
quantity by more than SEEN = 100 bounds in some case, so the lists can fail.  Workspace arithmetic: mlp.hip's k_chunk
restated; no shape overruns the split-K workspaces and the three tight shapes fill them to the last float.  And
`mlp.block` refuses what it cannot run.
The measured shares are in DESIGN §7f."""
import functools

import numpy as np
import pytest
import torch

import mlp_block_cases as mc

ROOM, LOOSE_ROOM, SEEN = 0.1, 0.5, 100.0


@functools.lru_cache(maxsize=None)
def _case(c):
    """(the case built, its float64 reference), once for the whole file: neither is modified by what reads it."""
    b = mc.build(c)
    return b, mc.block_ref64(b)


ALL_CASES = [c for lst in mc.LISTS.values() for c in lst]


def test_the_lists_are_what_the_gpu_file_names():
    assert [c.flags for c in mc.FLAGS] == list(range(16)) and len({c.name for c in ALL_CASES + mc.GUARD}) == len(ALL_CASES + mc.GUARD)
    assert all(c.p == (0.5 if c.flags & mc.TRAIN else 0.0) for c in mc.FLAGS)
    assert sorted({c.S for c in mc.SAMPLES}) == [1, 5, 15, 16]
    assert len(mc.GEMM_EDGES) <= 60 and len(ALL_CASES) <= 250
    assert [mc.splits(9, 5, c.F) for c in mc.GEMM_EDGES if c.name.endswith("-split")] == [2, 2, 3, 4, 26]
    assert 193 - 3 * mc.k_chunk(1, 193) == 1 and 65 - mc.k_chunk(1, 65) == 17          # last chunks of 1 and of 17 elements
    assert [mc.splits(9, 5, c.N) for c in mc.GEMM_EDGES if c.name.endswith("-split_dA")] == [2, 4]
    assert [mc.splits(5, 9, c.S * c.B) for c in mc.GEMM_EDGES if c.name.endswith("-split_dW")] == [2, 4, 2]
    assert {c.loose for c in mc.BN_EDGES if c.B == 2} == {True} and not any(c.loose for c in ALL_CASES if c.B != 2)
    for B in (2, 3, 15, 16, 17, 33):                         # the constant columns' float32 mean is exact: sum * (1 / B)
        assert np.float32(B) * (np.float32(1) / np.float32(B)) == np.float32(1), B


def test_special_inputs_are_what_the_lists_promise():
    b = mc.build(next(c for c in mc.BN_EDGES if c.flags == (mc.BN | mc.TRAIN) and c.F == 17 and c.B == 16))
    assert bool((b.x[:, :, 16] == 0).all()) and all(float(b.x[s, :, 0].var()) == 0.0 for s in range(2))
    assert float(b.x[0, 0, 0]) != float(b.x[1, 0, 0])
    b = mc.build(next(c for c in mc.ROW_EDGES if c.flags & mc.RELU and c.F == 65))
    r = b.x.view(9, 65)
    assert bool((r[0] < 0).all()) and int((r[1] > 0).sum()) == 1
    assert float(r[2, 0]) == 0.0 and bool(torch.signbit(r[2, 0])) and float(r[2, 1]) == 0.0 and not bool(torch.signbit(r[2, 1]))
    ref = mc.block_ref64(b)
    assert torch.equal(ref.out[0, 0], b.fc.bias.detach().double()) and not bool(ref.gx[0, 0].any())      # output = bias, dX row = 0
    for c in mc.ROW_EDGES:                                   # NORM without RELU: no all-zero row in the lists
        if not c.flags & mc.RELU:
            assert bool(mc.build(c).x.view(9, c.F).abs().sum(1).min() > 0)
    b = mc.build(mc.ZERO_ROW)
    assert not bool(b.x.view(9, 65)[4].any())
    ref = mc.block_ref64(b)                                  # dX = 1e12 * g * keep / (1 - p) there, in torch's float64 as well
    g = (b.gy.double().view(9, 4) @ b.fc.weight.detach().double())[4] * b.keep.view(9, 65)[4] * 2.0
    torch.testing.assert_close(ref.gx.view(9, 65)[4], 1e12 * g, rtol=1e-9, atol=0)


def test_manual_formulas_are_the_autograd_reference():
    for c in mc.FLAGS + mc.OPTIONAL[:2] + mc.ROW_EDGES + mc.BN_EDGES[:8] + mc.GEMM_EDGES[-8:]:
        (b, ref), man = _case(c), mc.block_manual64(_case(c)[0])
        for name in ref._fields:
            r, m = getattr(ref, name), getattr(man, name)
            if name == "nbt" or r is None:
                assert r == m, (c.name, name)
            else:
                torch.testing.assert_close(m, r, rtol=1e-9, atol=1e-12 * max(1.0, float(r.abs().max())), msg=f"{c.name} {name}")


@pytest.mark.parametrize("lst", list(mc.LISTS))
def test_float32_torch_stays_well_inside_every_bound(lst):
    worst, worst_loose = {}, {}
    for c in mc.LISTS[lst]:
        b, ref = _case(c)
        sh = mc.shares(b, mc.block_ref(b, torch.float32), ref)
        into = worst_loose if c.loose else worst
        for k, v in sh.items():
            if v >= into.get(k, (-1.0, ""))[0]:
                into[k] = (v, c.name)
        room = LOOSE_ROOM if c.loose else ROOM
        assert all(v < room for v in sh.values()), f"{c.name}: float32 torch uses {sh} of the bounds"
    print(f"[mlp_block host] {lst}: float32 shares " + ", ".join(f"{k} {v:.3g}" for k, (v, _) in worst.items()))
    if worst_loose:
        print(f"[mlp_block host] {lst} (loose rule): " + ", ".join(f"{k} {v:.3g}" for k, (v, _) in worst_loose.items()))


def test_guard_shapes_float32_headroom():
    for c in mc.GUARD:
        b, ref = _case(c)
        sh = mc.shares(b, mc.block_ref(b, torch.float32), ref)
        print(f"[mlp_block host] {c.name}: float32 shares " + ", ".join(f"{k} {v:.3g}" for k, v in sh.items()))
        assert all(v < ROOM for v in sh.values()), f"{c.name}: float32 torch uses {sh} of the bounds"


@pytest.mark.parametrize("mut", mc.MUTANTS)
def test_each_deliberate_mistake_moves_a_case_by_100_bounds(mut):
    best = (0.0, None, None)
    for c in ALL_CASES:
        b, ref = _case(c)
        sh = mc.shares(b, mc.block_manual64(b, mut), ref, only=mc.wanted(c) | {"out", "rm", "rv"})
        k = max(sh, key=sh.get)
        if sh[k] > best[0]:
            best = (sh[k], c.name, k)
        if best[0] > SEEN:
            break
    print(f"[mlp_block host] {mut}: {best[2]} of {best[1]} moves by {best[0]:.3g} bounds")
    assert best[0] > SEEN, f"{mut} moves nothing by more than {best[0]:.3g} bounds ({best[2]} of {best[1]})"


def test_split_partials_fit_their_workspaces_and_the_tight_shapes_fill_them():
    LIMIT = 524288                                           # floats: 2 MiB per sample forward, the backward's tail
    r = np.arange(1, 401, dtype=np.int64)
    tiles = (-(-r // 64))[:, None] * (-(-r // 64))[None, :]
    for K in sorted({1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 97, 129, 193, 2048, 2049, 4000}):
        want = np.where(tiles >= 128, 1, 128 // np.minimum(tiles, 128))
        want = np.maximum(1, np.minimum(np.minimum(want, -(-K // 64)), 32))
        kc = -(-(-(-K // 16)) // want) * 16
        n = -(-K // kc)
        assert int((n * r[:, None] * r[None, :]).max()) <= LIMIT, K
        for rows, cols in ((1, 1), (64, 64), (65, 400), (400, 1), (128, 128), (129, 127)):       # the vector form is k_chunk
            assert int(n[rows - 1, cols - 1]) == mc.splits(rows, cols, K), (rows, cols, K)
    for rows, cols, K in ((2048, 128, 128), (16 * 400, 400, 2049), (4096, 127, 65), (8191, 64, 4000)):   # dA with S B rows
        n = mc.splits(rows, cols, K)
        assert n == 1 or n * rows * cols <= LIMIT, (rows, cols, K)
    fwd, dA, dW = mc.TIGHT
    assert mc.splits(fwd.B, fwd.N, fwd.F) * fwd.B * fwd.N == LIMIT                               # per sample: S * 2 MiB in all
    assert mc.splits(dA.S * dA.B, dA.F, dA.N) * dA.S * dA.B * dA.F == LIMIT
    assert mc.splits(dW.N, dW.F, dW.S * dW.B) * dW.N * dW.F == LIMIT
    assert mc.splits(dW.S * dW.B, dW.F, dW.N) * dW.S * dW.B * dW.F == LIMIT                      # and that case's dA as well


def test_hashed_keep_is_the_layer_seed_hash():
    k = mc.hashed_keep(mc.DROP_SEED, 0, 3, 37, 70, 0.5)
    assert k.dtype == torch.uint8 and tuple(k.shape) == (3, 37, 70) and abs(float(k.float().mean()) - 0.5) < 0.03
    assert not torch.equal(k[0], k[1]) and not torch.equal(k, mc.hashed_keep(mc.DROP_SEED, 1, 3, 37, 70, 0.5))
    assert bool(mc.hashed_keep(1, 0, 1, 4, 4, 0.0).all()) and not bool(mc.hashed_keep(1, 0, 1, 4, 4, 1.0).any())


def test_block_refuses_what_it_cannot_run_before_any_native_call(monkeypatch):
    from grand_plus_amd import _native, mlp
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("block() reached the native library"))
    fc, bn = torch.nn.Linear(6, 3), torch.nn.BatchNorm1d(6)
    kw = dict(relu=True, node_norm=True, training=True, dropout=0.5, seed=1, layer=0)
    bad = [([[1.0] * 6] * 2, "tensor"),                                       # a non-tensor
           (torch.zeros((2, 4, 6), dtype=torch.float64), "float32"),
           (torch.zeros((2, 4, 6), dtype=torch.float16), "float32"),
           (torch.zeros((4, 6)), r"\[S, B, F\]"),                              # rank 2
           (torch.zeros((1, 2, 4, 6)), r"\[S, B, F\]"),
           (torch.zeros((2, 6, 4)).transpose(1, 2), "contiguous"),
           (torch.zeros((4, 4, 6))[::2], "contiguous"),
           (torch.zeros((0, 4, 6)), "number of samples"),
           (torch.zeros((17, 4, 6)), "number of samples"),
           (torch.zeros((2, 0, 6)), "no rows"),
           (torch.zeros((2, 4, 6)), "GPU only")]                              # a CPU tensor: the last check
    for x, msg in bad:
        for b in (bn, None):
            with pytest.raises(ValueError, match=msg):
                mlp.block(x, fc, b, **kw)
    with pytest.raises(ValueError, match="more than 1 value per channel"):   # every other check still comes before "GPU only"
        mlp.block(torch.zeros((2, 1, 6)), fc, bn, **kw)
    with pytest.raises(ValueError, match="takes 6 features"):
        mlp.block(torch.zeros((2, 4, 5)), fc, None, **kw)
    with pytest.raises(ValueError, match="keep must"):
        mlp.block(torch.zeros((2, 4, 6)), fc, None, keep=torch.zeros((2, 4, 6)), **kw)
