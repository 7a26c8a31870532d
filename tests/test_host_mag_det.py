"""CPU tests of MAG's deterministic table gradient and its captured step: what is particular to
the entry points of csrc/mag_det_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py holds the types), their error codes
before any GPU work, every refusal of the Python layer before a device call, and csrc/mag_det_layout.hpp itself
(tests/native/mag_det_check.cpp, built with the address and undefined-behaviour sanitizers and run as a program) against the
brute-force entry order."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header as ah
import mag_cases as mc
import mag_det_cases as dc
import native_check
from grand_plus_amd import _native
from grand_plus_amd import mag_det as md

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_mag_det_keys", "gp_mag_prop_rows_backward_det"]


# ---- 1. the binding
def test_the_table_is_the_headers_prototypes_position_by_position():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos, table = ah.prototypes("mag_det_abi.hpp"), _native.PRIVATE_ABI["mag_det_abi.hpp"]
    assert sorted(protos) == sorted(table) == NAMES
    assert len(table["gp_mag_det_keys"][1]) == 16 and len(table["gp_mag_prop_rows_backward_det"][1]) == 30
    # the deterministic backward takes the atomic backward's arguments up to keep_stride, name by name
    atomic = ah.prototypes("grandplus_mag.h")["gp_mag_prop_rows_backward"][1]
    assert protos["gp_mag_prop_rows_backward_det"][1][:22] == atomic[:22] and atomic[21][2] == "keep_stride"


def test_the_entry_points_stay_outside_c_abi_4():
    import __graft_entry__ as entry
    assert "mag_det.hip" in entry.LIB_UNITS
    for hdr in ("mag_det_abi.hpp", "mag_det_layout.hpp", "gather_sum.hpp", "mag_stage.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "gp_mag_det" not in public and "backward_det(" not in public.replace("gp_random_prop_rows_backward_det(", "").replace(
        "gp_embedding_bag_backward_det(", "")
    assert not [n for n in vars(_native) if "MAG_DET" in n.upper()]
    assert _native.lib().gp_abi_version() == 4


def test_the_units_share_their_lines_and_the_kernels_hold_no_atomics():
    hip = open(os.path.join(CSRC, "mag_det.hip")).read()
    for hdr in ("mag_stage.hpp", "gather_sum.hpp", "mag_det_layout.hpp", "mag_det_abi.hpp"):
        assert f'#include "{hdr}"' in hip
    for call in ("stage_row(", "sample_weight", "row_len(", "inv_den_rows(", "inv_den_bag(", "gp_mag_det::slot_of(",
                 "gp_mag_det::live_entries(", "gp_mag_det::tail_begin(", "gp_mag_det::overflowed(", "gather_sum_kernel<MagOp>"):
        assert call in hip or call in open(os.path.join(CSRC, "mag_stage.hpp")).read(), call
    code = re.sub(r"//[^\n]*", "", hip)
    assert not re.search(r"atomic|\basm\b|printf|assert\s*\(|__builtin_amdgcn_s_", code)
    assert not re.search(r"1e-1[02]f", code), "a denominator written out by hand"
    # the gather kernel and the staging are stated once
    for name, home in (("gather_sum_kernel(Op op", "gather_sum.hpp"), ("void stage_row(", "mag_stage.hpp"), ("struct MagArgs", "mag_stage.hpp")):
        holders = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if name in open(p, errors="replace").read()]
        assert holders == [home], (name, holders)
    scatter = open(os.path.join(CSRC, "scatter_det.hip")).read()
    assert '#include "gather_sum.hpp"' in scatter and "gather_sum_kernel<RowsOp>" in scatter
    layout = open(os.path.join(CSRC, "mag_det_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["cstdint"]


# ---- 2. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def keys(V=50, indptr=P, indices=P, n_nodes=12, col=P, filled=P, n_rows=6, K=5, batch=P, B=4, cap=100, base=P, out=P, flag=P):
        return L.gp_mag_det_keys(0, V, indptr, indices, n_nodes, col, filled, n_rows, K, batch, B, cap, base, out, flag, None)

    for kw in (dict(V=0), dict(n_nodes=-1), dict(n_rows=-1), dict(K=0), dict(K=1025), dict(B=-1), dict(cap=0), dict(cap=-5),
               dict(B=2 ** 31 - 1, K=2), dict(B=2 ** 21, K=1024)):
        assert keys(**kw) == E, kw
    assert "gp_mag_det_keys" in L.gp_last_error().decode()
    for name in ("indptr", "indices", "col", "base", "out", "flag"):
        assert keys(**{name: None}) == N, name
    assert keys(indptr=None, cap=0) == E                                         # sizes are judged first
    assert keys(B=0) == OK and keys(B=0, indptr=None, out=None) == OK            # nothing to do: nothing launched
    assert keys(B=2 ** 21 - 1, K=1024, indptr=None) == N                         # 2^31 - 1024 slots pass the size check

    def back(g=P, V=50, H=7, indptr=P, indices=P, data=P, n_nodes=12, col=P, val=P, filled=P, n_rows=6, K=5, batch=P, B=4, S=2,
             p_node=0.5, p_in=0.0, training=1, keep=None, stride=0, base=P, order=P, skeys=P, cap=100, U=P, inv=P, dW=P):
        return L.gp_mag_prop_rows_backward_det(0, g, V, H, indptr, indices, data, n_nodes, col, val, filled, n_rows, K, batch, B, S,
                                               p_node, p_in, training, ctypes.c_uint64(1), keep, stride, base, order, skeys, cap,
                                               U, inv, dW, None)

    for kw in (dict(V=0), dict(H=0), dict(n_nodes=-1), dict(n_rows=-1), dict(K=0), dict(K=1025), dict(B=-1), dict(S=0), dict(S=17),
               dict(p_node=1.5), dict(p_in=-0.1), dict(keep=P, stride=0), dict(cap=0), dict(B=2 ** 21, K=1024),
               dict(p_in=0.5), dict(p_in=1.0), dict(p_in=0.5, B=0)):
        assert back(**kw) == E, kw
    assert "input dropout" in L.gp_last_error().decode() and "gp_mag_prop_rows_backward_det" in L.gp_last_error().decode()
    assert back(p_in=0.5, training=0, B=0) == OK                                 # eval mode: input dropout does nothing
    for name in ("g", "indptr", "indices", "data", "col", "val", "base", "order", "skeys", "U", "inv", "dW"):
        assert back(**{name: None}) == N, name
    assert back(g=None, cap=0) == E
    assert back(B=0) == OK and back(B=0, g=None, dW=None) == OK


# ---- 3. the Python layer
def _host_args(**kw):
    c = mc.case("h7_k5_s3")
    Pm = c["P"]
    a = dict(weight=Pm.W, attr_indptr=Pm.indptr, attr_indices=Pm.indices, attr_data=Pm.data, col=Pm.col.reshape(-1),
             val=Pm.val.reshape(-1), filled=Pm.filled, K=Pm.K)
    a.update(kw)
    return a


class _Cuda(torch.Tensor):
    """A CPU tensor that says it is on the GPU: it passes the type checks of the Python layer, which must refuse before it
    reaches the library."""
    @property
    def is_cuda(self):
        return True


def _fake_cuda(t):
    return None if t is None else t.as_subclass(_Cuda)


def test_mag_prop_rows_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd.mag import mag_prop_rows
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    for bad in (0, -3, 2.0, "8", True):
        with pytest.raises(ValueError, match="max_entries must be an int >= 1"):
            mag_prop_rows(**_host_args(), max_entries=bad)
    a = {k: _fake_cuda(v) if isinstance(v, torch.Tensor) else v for k, v in _host_args().items()}
    a["weight"] = _fake_cuda(mc.case("h7_k5_s3")["P"].W.clone().requires_grad_(True))
    # the two pinned refusals of today's call: no max_entries, a gradient wanted, the flag or torch's global mode
    with pytest.raises(RuntimeError, match=r"deterministic=True.*embedding_bag_csr"):
        mag_prop_rows(**a, deterministic=True)
    torch.use_deterministic_algorithms(True)
    try:
        with pytest.raises(RuntimeError, match=r"deterministic=True.*embedding_bag_csr"):
            mag_prop_rows(**a)
        with pytest.raises(ValueError, match="does not support input dropout"):
            mag_prop_rows(**a, max_entries=100, input_droprate=0.5)
    finally:
        torch.use_deterministic_algorithms(False)
    with pytest.raises(ValueError, match="does not support input dropout"):
        mag_prop_rows(**a, deterministic=True, max_entries=100, input_droprate=0.5)
    for bad in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), [0], torch.zeros(1, dtype=torch.int32, device="meta")):
        with pytest.raises(TypeError, match="overflow must be a contiguous int32 tensor of one element"):
            mag_prop_rows(**a, deterministic=True, max_entries=100, overflow=bad)
    with pytest.raises(TypeError, match="deterministic must be None, True or False"):
        mag_prop_rows(**a, deterministic=1, max_entries=100)


def test_backward_det_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd.mag import _Call
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="does not support input dropout"):
        md.backward_det((5, 3), z, _Call((z,) * 8, 2, 2, 2, 1, 0.5, 0.5, True, 0), 10, z)
    with pytest.raises(ValueError, match="fewer than 2\\*\\*31 slots"):
        md.backward_det((5, 3), z, _Call((z,) * 8, 2, 1024, 2 ** 21, 1, 0.5, 0.0, True, 0), 10, z)


class _FakeState:
    device = torch.device("cuda", 0)

    def configure(self, *a):
        pass


def _rows(n_nodes=12, S_rows=6, K=4):
    from grand_plus_amd.rows import RowMatrix
    z = torch.zeros(S_rows * K, dtype=torch.int32)
    return RowMatrix(np.arange(S_rows), K, z, z, torch.zeros(S_rows * K, dtype=torch.float64),
                     torch.full((S_rows,), K, dtype=torch.int32), n_nodes)


def _mag_step(model=None, opt=None, rows=None, attrs=None, **kw):
    from grand_plus_amd import ClipAdam, MagTrainStep, mag_trained_parameters
    from grand_plus_amd.mlp import MagMLP
    model = MagMLP(9, 3, 4, 2, True, 0.0, 0.5, True).train() if model is None else model
    opt = ClipAdam(mag_trained_parameters(model), capturable=True, state=_FakeState()) if opt is None else opt
    args = dict(samples=2, dropnode_rate=0.5, lam=1.0, warmup=10, tem=0.5, seed=1)
    args.update(kw)
    attrs = (torch.zeros(13, dtype=torch.int64), torch.zeros(0, dtype=torch.int32), torch.zeros(0)) if attrs is None else attrs
    return MagTrainStep(model, opt, _rows() if rows is None else rows, *attrs, torch.zeros(12, dtype=torch.int64), [0, 1, 2], [3, 4, 5],
                        **args)


def test_mag_train_step_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd import ClipAdam, MagTrainStep, TrainStep, mag_trained_parameters
    from grand_plus_amd.mlp import GrandPlusMLP, MagMLP
    from grand_plus_amd.step import trained_parameters
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    assert issubclass(MagTrainStep, TrainStep)
    dense = GrandPlusMLP(5, 3, 4, 2, True, 0.5, 0.5, True).train()
    with pytest.raises(ValueError, match="takes a MagMLP"):
        _mag_step(model=dense, opt=ClipAdam(trained_parameters(dense), capturable=True, state=_FakeState()))
    drop = MagMLP(9, 3, 4, 2, True, 0.5, 0.5, True).train()
    with pytest.raises(ValueError, match=r"input_droprate = 0.*DESIGN §9"):
        _mag_step(model=drop)
    model = MagMLP(9, 3, 4, 2, True, 0.0, 0.5, True).train()
    with pytest.raises(ValueError, match=re.escape("ClipAdam(capturable=True)")):
        _mag_step(model=model, opt=ClipAdam(model.parameters()))
    with pytest.raises(ValueError, match="rows must be a RowMatrix"):
        _mag_step(rows=object())
    z64, z32, zf = torch.zeros(13, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), torch.zeros(3)
    for attrs, msg in (((z64.int(), z32, zf), "attr_indptr"), ((z64, z32.long(), zf), "attr_indices"), ((z64, z32, zf.double()), "attr_data"),
                       ((z64[:12], z32, zf), "one entry per node"), ((z64, z32, zf[:2]), "the same length")):
        with pytest.raises(ValueError, match=msg):
            _mag_step(attrs=attrs)
    for kw, msg in ((dict(samples=0), "samples"), (dict(samples=17), "samples"), (dict(dropnode_rate=1.5), "dropnode_rate"),
                    (dict(kind="mse"), "kind"), (dict(tem=0.0), "tem"), (dict(max_entries=0), "max_entries"),
                    (dict(max_entries=1.5), "max_entries")):
        with pytest.raises(ValueError, match=msg):
            _mag_step(**kw)
    with pytest.raises(TypeError, match="deterministic must be"):
        _mag_step(deterministic="yes")
    with pytest.raises(ValueError, match="no CPU fallback"):                     # everything else passes: only the device is missing
        _mag_step()
    # TrainStep still refuses a MagMLP, with the words the step's users know
    with pytest.raises(ValueError, match="takes a GrandPlusMLP"):
        TrainStep(model, ClipAdam(mag_trained_parameters(model), capturable=True, state=_FakeState()), _rows(), torch.zeros((12, 5)),
                  torch.zeros(12, dtype=torch.int64), [0, 1, 2], [3, 4, 5], samples=2, dropnode_rate=0.5, lam=1.0, warmup=10, tem=0.5, seed=1)


def test_mag_trained_parameters_and_the_exports():
    import grand_plus_amd
    from grand_plus_amd import mag_step
    from grand_plus_amd.mlp import MagMLP
    assert grand_plus_amd.MagTrainStep is mag_step.MagTrainStep
    assert grand_plus_amd.mag_trained_parameters is mag_step.mag_trained_parameters
    assert "MagTrainStep" not in grand_plus_amd.__all__
    m = MagMLP(9, 3, 4, 3, True, 0.0, 0.5, True)
    ps = mag_step.mag_trained_parameters(m)
    assert ps[0] is m.embeds.weight and len(ps) == 1 + 2 * (2 + 2)
    nobn = MagMLP(9, 3, 4, 2, False, 0.0, 0.5, True)
    assert len(mag_step.mag_trained_parameters(nobn)) == 1 + 2
    one = MagMLP(9, 3, 4, 1, True, 0.0, 0.5, True)                                 # the embedding is the logits
    assert [p is one.embeds.weight for p in mag_step.mag_trained_parameters(one)] == [True]
    # the new keywords of emb_rows default to today's call
    import inspect
    sig = inspect.signature(MagMLP.emb_rows).parameters
    assert [sig[k].default for k in ("deterministic", "max_entries", "overflow")] == [None, None, None]


# ---- 4. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "mag_det_check")
    return lambda lines: native_check.ints(native_check.run(exe, lines))


def test_the_layout_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_layout.cpp"
    src.write_text('#include "mag_det_layout.hpp"\nint main() { long long b[2] = {0, 3}; return (int)gp_mag_det::slot_of(b, 1, 2); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_layout"), str(src)], check=True,
                   timeout=120)


@pytest.mark.parametrize("n_slots", sorted(dc.GRID))
def test_the_layout_is_the_brute_force_entry_order(checker, n_slots):
    """Slot counts around the scan's 1 024, bags of 0, 1, 63, 64 and 65 entries, max_entries one short of the total, equal to
    it and 130 past it: every entry's slot, the clamp and the tail, from the header under the sanitizers."""
    Pm = dc.grid_problem(n_slots)
    E = dc.entry_order(Pm, None)
    lens = np.diff(E["slot_base"])
    assert len(lens) == n_slots and E["total"] > 1
    if n_slots > 1:
        assert set(dc.GRID_BAGS) <= set(lens.tolist())                             # every bag length occurs, the empty bag too
    caps = [E["total"] + d for d in dc.SLACK]
    got = checker([f"layout {cap} " + " ".join(map(str, lens)) for cap in caps])
    assert len(got) == len(dc.SLACK) == 4
    for cap, line in zip(caps, got):
        total, live, tail, over, miss_lo, miss_at, miss_past = line[:7]
        assert total == E["total"] and live == tail == min(total, cap) and over == int(total > cap)
        assert miss_lo == miss_at == miss_past == n_slots                          # no entry: the slot count comes back
        assert line[7:] == E["slot"].tolist()
        assert cap - tail == max(cap - total, 0)                                   # the tail's length


def test_the_layout_of_lone_and_leading_empty_slots(checker):
    got = checker(["layout 5 0 0 3 0 0 2 0", "layout 1 4", "layout 9 0 1"])
    assert got[0] == [5, 5, 5, 0, 7, 7, 7, 2, 2, 2, 5, 5]
    assert got[1] == [4, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0]
    assert got[2] == [1, 1, 1, 0, 2, 2, 2, 1]
