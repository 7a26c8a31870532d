"""CPU tests of MAG's device seed and of its deterministic table gradient with input dropout: the entry
points of csrc/mag_drop_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py holds the types), their error codes before
any GPU work, every refusal of the Python layer before a device call, the audit of tests/mag_drop_cases.py -- each
deliberate mistake moves a case, two samples' masks differ on a common element -- and the contract's own float32 rounding
against the float64 bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import abi_header as ah
import mag_cases as mc
import mag_drop_cases as xc
from grand_plus_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_mag_prop_rows_backward_det_drop", "gp_mag_prop_rows_backward_dseed", "gp_mag_prop_rows_dseed"]


# ---- 1. the binding
def test_the_table_is_the_headers_prototypes_position_by_position():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos, table = ah.prototypes("mag_drop_abi.hpp"), _native.PRIVATE_ABI["mag_drop_abi.hpp"]
    assert sorted(protos) == sorted(table) == NAMES
    assert [len(table[n][1]) for n in NAMES] == [34, 24, 25]
    # the device-seed forms are grandplus_mag.h's pair but for one position: d_seed, a device pointer, where seed stands
    public = ah.prototypes("grandplus_mag.h")
    for name in ("gp_mag_prop_rows", "gp_mag_prop_rows_backward"):
        val, dev = public[name][1], protos[name + "_dseed"][1]
        assert len(val) == len(dev) and [i for i in range(len(val)) if val[i] != dev[i]] == [19]
        assert val[19] == ("uint64_t", 0, "seed") and dev[19] == ("uint64_t", 1, "d_seed")
        assert _native.ABI["grandplus_mag.h"][name][1][19] is ctypes.c_uint64 and table[name + "_dseed"][1][19] is ctypes.c_void_p
    # the deterministic backward: gp_mag_prop_rows_backward_det's arguments, d_seed after seed, the chunk's three before the stream
    det, drop = ah.prototypes("mag_det_abi.hpp")["gp_mag_prop_rows_backward_det"][1], protos["gp_mag_prop_rows_backward_det_drop"][1]
    assert det[19][2] == "seed" and drop[:20] == det[:20] and drop[20] == ("uint64_t", 1, "d_seed")
    assert drop[21:30] == det[20:29] and drop[-1] == det[-1] == ("void", 1, "stream")
    assert drop[30:33] == [("int32_t", 0, "chunk"), ("float", 1, "d_scratch"), ("int64_t", 0, "scratch_bytes")]
    assert drop[30:] == ah.prototypes("gather_chunk_abi.hpp")["gp_mag_prop_rows_backward_det_chunked"][1][-4:]


def test_the_entry_points_stay_outside_c_abi_4_and_add_no_constant():
    import glob
    import __graft_entry__ as entry
    assert "mag_drop.hip" in entry.LIB_UNITS
    for hdr in ("mag_drop_abi.hpp", "mag_drop_gather.hpp", "mag_stage.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "dseed" not in public and "det_drop" not in public
    assert not [n for n in vars(_native) if re.fullmatch(r"GP_[A-Z0-9_]+", n) and ("DROP" in n or "DSEED" in n)]
    assert _native.lib().gp_abi_version() == 4
    # the public pair keeps its parameter counts
    assert [len(_native.ABI["grandplus_mag.h"][n][1]) for n in ("gp_mag_prop_rows", "gp_mag_prop_rows_backward")] == [25, 24]


def test_the_unit_shares_its_lines_and_holds_no_atomics():
    hip = open(os.path.join(CSRC, "mag_drop.hip")).read()
    for hdr in ("mag_stage.hpp", "mag_drop_abi.hpp", "mag_drop_gather.hpp", "gather_chunk_layout.hpp"):
        assert f'#include "{hdr}"' in hip
    for call in ("stage_row(", "call_seed(", "inv_den_rows(", "inv_den_bag(", "inv_keep(", "waves_for(", "mag_check(",
                 "gp_gather_chunk::chunk_ok(", "gp_gather_chunk::scratch_bytes(", "gp_mag_drop::gather("):
        assert call in hip, call
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"atomic|\basm\b|printf|assert\s*\(|__builtin_amdgcn_s_|hipMalloc|hipMemcpy|Synchronize", code)
    assert not re.search(r"1e-1[02]f", code), "a denominator written out by hand"
    for restated in ("struct MagArgs", "void stage_row(", "struct SlotArgs", "slot_node(const", "sample_weight(float", "keep_scale(u64",
                     "gather_sum_kernel(Op op", "gather_chunk_kernel(Op op"):
        assert restated not in hip, restated
    # GP_MAG_SLOT_SEED keeps one definition, in mag_prop.hip, where the gather's Op stands next to it; the seed is read by one line
    prop = open(os.path.join(CSRC, "mag_prop.hip")).read()
    holders = [n for n in os.listdir(CSRC) if "u64 slot_seed(" in open(os.path.join(CSRC, n), errors="replace").read()]
    assert holders == ["mag_prop.hip"] and "slot_seed(" not in hip
    for call in ("struct MagDropOp", "gather_sum_kernel<MagDropOp>", '"gather_chunk_kernel<MagDropOp>"', "slot_seed(E.seed, s, rslot)",
                 "gp_mag_det::slot_of(", "gp_mag_det::live_entries(", "slot_node(A, e, node)", "keep_scale(sseed,"):
        assert call in prop, call
    stage = open(os.path.join(CSRC, "mag_stage.hpp")).read()
    assert "return A.d_seed ? *A.d_seed : A.seed;" in stage and re.search(r"const u64\* d_seed;[^\n]*\n\};", stage), "d_seed is MagArgs' last member"
    for unit in ("mag_prop.hip", "mag_det.hip", "mag_drop.hip"):
        kernels = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, unit)).read()).split('extern "C"')[0]
        assert "A.seed" not in kernels, f"{unit}: a kernel reads A.seed past call_seed"
    mag_det = open(os.path.join(CSRC, "mag_det.hip")).read()
    assert mag_det.count("const MagArgs A") == 1 and mag_det.count("const MagOp op") == 1 and "MagDropOp" not in mag_det


# ---- 2. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def back(g=P, V=50, H=7, indptr=P, indices=P, data=P, n_nodes=12, col=P, val=P, filled=P, n_rows=6, K=5, batch=P, B=4, S=2,
             p_node=0.5, p_in=0.5, training=1, d_seed=None, keep=None, stride=0, base=P, order=P, skeys=P, cap=100, U=P, inv=P, dW=P,
             chunk=0, scratch=None, nbytes=0):
        return L.gp_mag_prop_rows_backward_det_drop(0, g, V, H, indptr, indices, data, n_nodes, col, val, filled, n_rows, K, batch, B, S,
                                                    p_node, p_in, training, ctypes.c_uint64(1), d_seed, keep, stride, base, order, skeys,
                                                    cap, U, inv, dW, chunk, scratch, nbytes, None)

    for kw in (dict(V=0), dict(H=0), dict(n_nodes=-1), dict(n_rows=-1), dict(K=0), dict(K=1025), dict(B=-1), dict(S=0), dict(S=17),
               dict(p_node=1.5), dict(p_in=-0.1), dict(p_in=1.5), dict(p_in=float("nan")), dict(keep=P, stride=0), dict(cap=0),
               dict(cap=-5), dict(B=2 ** 21, K=1024), dict(B=2 ** 31 - 1, K=2), dict(B=0, K=0), dict(B=0, cap=0)):
        assert back(**kw) == E, kw
    assert "gp_mag_prop_rows_backward_det_drop" in L.gp_last_error().decode()
    # the chunk: 0 is the unchunked gather and looks at no scratch; otherwise §7w's rules
    need = 2 * ((100 + 63) // 64) * 7 * 4
    for kw in (dict(chunk=1), dict(chunk=32), dict(chunk=96), dict(chunk=8192), dict(chunk=-64), dict(chunk=64, scratch=P, nbytes=need - 1),
               dict(chunk=64, scratch=P, nbytes=0), dict(chunk=63, B=0)):
        assert back(**kw) == E, kw
    assert back(chunk=64, scratch=None, nbytes=need) == N
    assert back(chunk=0, scratch=None, nbytes=-1, B=0) == OK
    assert back(chunk=64, scratch=None, nbytes=0, B=0) == OK                     # nothing to do: no scratch is needed
    for name in ("g", "indptr", "indices", "data", "col", "val", "base", "order", "skeys", "U", "inv", "dW"):
        assert back(**{name: None}) == N, name
        assert back(**{name: None}, chunk=64, scratch=P, nbytes=need) == N, name
    assert back(g=None, cap=0) == E                                              # sizes are judged first
    # input dropout is accepted at every rate, and so is d_seed = NULL (the value is used) or a pointer
    for kw in (dict(p_in=0.0), dict(p_in=0.5), dict(p_in=1.0), dict(training=0), dict(d_seed=P), dict(g=None, dW=None)):
        assert back(B=0, **kw) == OK, kw
    assert back(B=2 ** 21 - 1, K=1024, indptr=None) == N                         # 2^31 - 1024 slots pass the size check

    def front(name, d_seed=P, w=P, V=5, H=4, ip=P, ix=P, dt=P, n_nodes=3, col=P, val=P, filled=P, S_rows=2, K=3, rows=P, B=2, S=1,
              p_node=0.5, p_in=0.5, training=1, keep=None, stride=6, out=P, n_bad=P):
        tail = (out, n_bad, None) if name == "gp_mag_prop_rows_dseed" else (out, None)
        return getattr(L, name)(0, w, V, H, ip, ix, dt, n_nodes, col, val, filled, S_rows, K, rows, B, S, p_node, p_in, training, d_seed,
                                keep, stride, *tail)

    for name in ("gp_mag_prop_rows_dseed", "gp_mag_prop_rows_backward_dseed"):
        for kw in (dict(S=17), dict(S=0), dict(K=0), dict(K=1025), dict(H=0), dict(V=0), dict(p_node=-0.1), dict(p_in=1.5), dict(B=-1),
                   dict(keep=P, stride=0), dict(B=0, K=0)):
            assert front(name, **kw) == E, (name, kw)
        assert name in L.gp_last_error().decode()
        for missing in ("d_seed", "w", "ip", "ix", "dt", "col", "val", "out"):
            assert front(name, **{missing: None}) == N, (name, missing)
        assert front(name, B=0) == OK and front(name, B=0, d_seed=None, w=None, out=None) == OK


# ---- 3. the Python layer
class _Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it passes the type checks of the Python layer, which must refuse before it
    reaches the library."""
    @property
    def is_cuda(self):
        return True


def _fake_cuda(t):
    return None if t is None else t.as_subclass(_Cuda)


def _host_args(**kw):
    Pm = mc.case("h7_k5_s3")["P"]
    a = dict(weight=Pm.W, attr_indptr=Pm.indptr, attr_indices=Pm.indices, attr_data=Pm.data, col=Pm.col.reshape(-1),
             val=Pm.val.reshape(-1), filled=Pm.filled, K=Pm.K)
    a.update(kw)
    return {k: _fake_cuda(v) if isinstance(v, torch.Tensor) else v for k, v in a.items()}


def test_mag_prop_rows_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd.mag import mag_prop_rows
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    a = _host_args()
    a["weight"] = _fake_cuda(mc.case("h7_k5_s3")["P"].W.clone().requires_grad_(True))
    # det_input_dropout is the deterministic backward's: the mode and the capacity are needed, whatever the rate
    for kw in (dict(), dict(deterministic=False), dict(deterministic=False, max_entries=100), dict(deterministic=True),
               dict(max_entries=100), dict(deterministic=True, input_droprate=0.5), dict(deterministic=False, max_entries=100, input_droprate=0.5)):
        with pytest.raises(ValueError, match=r"det_input_dropout=True .* needs deterministic=True .* and max_entries="):
            mag_prop_rows(**a, det_input_dropout=True, **kw)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="det_input_dropout must be True or False"):
            mag_prop_rows(**a, deterministic=True, max_entries=100, det_input_dropout=bad)
    # without the keyword the pinned refusal stays, with the words it has today
    with pytest.raises(ValueError, match=r"does not support input dropout \(DESIGN §9\): input_droprate must be 0 in training"):
        mag_prop_rows(**a, deterministic=True, max_entries=100, input_droprate=0.5)
    # a seed tensor of another dtype, size or device
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.uint8), torch.zeros(1), torch.zeros(2, dtype=torch.int64),
                torch.zeros(0, dtype=torch.int64), torch.zeros((1, 1), dtype=torch.int64).expand(1, 2), torch.zeros(1, dtype=torch.int64, device="meta")):
        for kw in (dict(), dict(input_droprate=0.5), dict(deterministic=True, max_entries=100, det_input_dropout=True, input_droprate=0.5),
                   dict(training=False)):
            with pytest.raises(TypeError, match="seed must be an int, or a contiguous int64 tensor of one element"):
                mag_prop_rows(**a, seed=bad, **kw)


def test_backward_det_still_refuses_input_dropout(monkeypatch):
    from grand_plus_amd import mag_det, mag_drop
    from grand_plus_amd.mag import _Call
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="does not support input dropout"):
        mag_det.backward_det((5, 3), z, _Call((z,) * 8, 2, 2, 2, 1, 0.5, 0.5, True, 0), 10, z)
    with pytest.raises(ValueError, match="fewer than 2\\*\\*31 slots"):
        mag_drop.backward_det_drop((5, 3), z, _Call((z,) * 8, 2, 1024, 2 ** 21, 1, 0.5, 0.5, True, 0), 10, z)
    reached = object()
    monkeypatch.setattr(_native, "lib", lambda: reached)
    assert mag_drop.lib() is reached                                             # one patch of the binder reaches this module too
    assert not hasattr(mag_drop, "ABI")
    assert _Call((z,) * 8, 2, 2, 2, 1, 0.5, 0.5, True, torch.zeros(1, dtype=torch.int64)).dseed and not _Call((z,) * 8, 2, 2, 2, 1, 0.5, 0.5, True, 7).dseed


class _FakeState:
    device = torch.device("cuda", 0)

    def configure(self, *a):
        pass


def _mag_step(p_in, **kw):
    from grand_plus_amd import ClipAdam, MagTrainStep, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    from grand_plus_amd.rows import RowMatrix
    model = MagMLP(9, 3, 4, 2, True, p_in, 0.5, True).train()
    opt = ClipAdam(mag_trained_parameters(model), capturable=True, state=_FakeState())
    z = torch.zeros(24, dtype=torch.int32)
    rows = RowMatrix(np.arange(6), 4, z, z, torch.zeros(24, dtype=torch.float64), torch.full((6,), 4, dtype=torch.int32), 12)
    return MagTrainStep(model, opt, rows, torch.zeros(13, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0),
                        torch.zeros(12, dtype=torch.int64), [0, 1, 2], [3, 4, 5], samples=2, dropnode_rate=0.5, lam=1.0, warmup=10,
                        tem=0.5, seed=1, **kw)


def test_mag_train_step_refuses_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    for bad in (1, 0, None, "yes"):
        with pytest.raises(TypeError, match="input_dropout must be True or False"):
            _mag_step(0.5, input_dropout=bad)
    with pytest.raises(ValueError, match=r"input_droprate = 0.*DESIGN §9.*input_dropout=True"):
        _mag_step(0.5)
    with pytest.raises(ValueError, match=r"input_droprate = 0.*DESIGN §9"):
        _mag_step(0.5, input_dropout=False)
    # with the keyword the model passes: every other refusal follows as before, down to the missing device
    for p_in in (0.5, 0.0):
        with pytest.raises(ValueError, match="no CPU fallback"):
            _mag_step(p_in, input_dropout=True)
    with pytest.raises(ValueError, match="needs the deterministic table gradient"):
        _mag_step(0.5, input_dropout=True, deterministic=False, table_step="lazy")
    import inspect
    from grand_plus_amd.mlp import MagMLP
    sig = inspect.signature(MagMLP.emb_rows).parameters
    assert sig["det_input_dropout"].default is False and sig["seed"].default is None


# ---- 4. the cases
def test_the_cases_are_the_ones_the_design_names():
    assert set(xc.CASES) >= {"pin05_h65_s3", "pin05_h64_k32", "pin05_s16", "pin1", "eps_scale", "h257_k5_s2", "k1024_s16", "segments",
                             "bad_indices", "hub"}
    for name in xc.CASES:
        kw = xc.case(name)["kw"]
        assert kw["training"] and kw["input_droprate"] == (1.0 if name == "pin1" else 0.5), name
    assert xc.case("h257_k5_s2")["P"].H == 257 and xc.case("k1024_s16")["P"].K == 1024 and xc.case("k1024_s16")["P"].H == 1
    assert xc.case("k1024_s16")["S"] == 16 and (16384 - 1024 - 16) // 1024 < 16   # the 16 weight rows take two LDS stages
    hub = xc.case("hub")
    assert hub["P"].longest == 4097 and int(np.bincount(hub["E"]["keys"]).min()) > 2 * xc.CHUNK   # every row: three chunks or more
    assert not torch.equal(hub["dW"], hub["dW_chunked"])                          # the chunked order is another order there
    E = xc.case("segments")["E"]
    sk = np.sort(E["keys"], kind="stable")
    assert [int((sk == a).sum()) for a in range(4)] == [63, 64, 65, 64] and int(np.flatnonzero(sk == 1)[0]) == 63
    bad = xc.case("bad_indices")
    assert int((bad["E"]["keys"] == bad["P"].V).sum()) >= 4
    # a destination of at most CHUNK entries has the unchunked bits
    for name in xc.CASES:
        c = xc.case(name)
        short = torch.from_numpy(np.bincount(c["E"]["keys"], minlength=c["P"].V + 1)[:c["P"].V] <= xc.CHUNK)
        assert torch.equal(c["dW"][short], c["dW_chunked"][short]), name


def test_two_samples_masks_differ_on_a_common_element_in_every_case_that_draws_one():
    for name in xc.CASES:
        c = xc.case(name)
        assert c["overlap"] == (name not in xc.DEGENERATE), name
        if name in xc.DEGENERATE:
            assert not bool(c["dW"].any())                                       # input_droprate = 1 keeps nothing
        else:
            assert bool(c["dW"].any()) and bool(torch.isfinite(c["dW"]).all())


@pytest.mark.parametrize("mistake", xc.MISTAKES)
def test_each_deliberate_mistake_moves_a_case(mistake):
    """The bitwise walk sees the mistake in `moved`; in `caught` the float64 bound sees it too."""
    moved, caught = [], []
    for name in xc.CASES:
        c = xc.case(name)
        got = xc.walk_dW32_drop(*c["args"], mut=mistake)
        if not torch.equal(got.view(torch.int32), c["dW"].view(torch.int32)):
            moved.append(name)
            if float(((got.double() - xc.reference(name)[0]).abs() / xc.bound(name)).max()) > 1.0:
                caught.append(name)
    print(f"[mag drop] {mistake}: moves {moved}, past the float64 bound in {caught}")
    assert moved and caught and "pin1" not in moved
    with pytest.raises(AssertionError):
        xc.walk_dW32_drop(*xc.case("segments")["args"], mut="no such mistake")


# ---- 5. the contract's own rounding
def test_the_float32_walk_stays_within_the_float64_bound_on_every_case():
    worst = 0.0
    for name in xc.CASES:
        c = xc.case(name)
        dW64, _terms, _n = xc.reference(name)
        b = xc.bound(name)
        for what, dW in (("unchunked", c["dW"]), ("chunked", c["dW_chunked"])):
            ratio = float(((dW.double() - dW64).abs() / b).max())
            print(f"[mag drop] {name} {what}: walked error / bound {ratio:.3g}")
            worst = max(worst, ratio)
            assert ratio <= 1.0, (name, what, ratio)
    print(f"[mag drop] worst walked error / bound {worst:.3g}")
