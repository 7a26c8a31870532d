"""CPU tests of the ctypes binding, _native.ABI and _native.PRIVATE_ABI, header by header: every public header is wired
into the one ABI and the one library, the private headers csrc/*_abi.hpp stay outside it, each table's entries are its
header's prototypes, every type is the one the convention stated above _native.ABI gives, and the Python mirrors of the
macros and structs equal what the C compiler makes of the headers."""
import ctypes
import glob
import os
import re

import pytest

import abi_header as ah
import optim_cases as oc
from grand_plus_amd import _native

HEADERS = list(_native.ABI)
PRIVATE = list(_native.PRIVATE_ABI)                                   # the headers of the entry points outside C ABI 4
# header -> the translation units of libgrandplus.so that define its entry points
UNITS = {"grandplus.h": ("gfpush.hip", "augment.hip", "propagate.hip", "objective.hip", "mlp.hip", "optim.hip"),
         "grandplus_eval.h": ("evaluate.hip",), "grandplus_scatter.h": ("scatter_det.hip",),
         "grandplus_infer.h": ("mlp_infer.hip",), "grandplus_infer_chain.h": ("mlp_chain.hip",),
         "grandplus_mag.h": ("mag_prop.hip",), "grandplus_order.h": ("gfpush.hip",),
         "grandplus_step.h": ("step_state.hip", "optim.hip"), "grandplus_fit.h": ("fit.hip",)}
N_MAIN = 42                                                           # prototypes of grandplus.h itself
NAMES = {"grandplus_eval.h": ["gp_eval_head", "gp_eval_reduce"],
         "grandplus_scatter.h": ["gp_embedding_bag_backward_det", "gp_random_prop_rows_backward_det"],
         "grandplus_infer.h": ["gp_mlp_infer_block"], "grandplus_infer_chain.h": ["gp_mlp_infer_chain2"],
         "grandplus_mag.h": ["gp_mag_prop_rows", "gp_mag_prop_rows_backward"],
         "grandplus_order.h": ["gp_internal_row_order", "gp_internal_wg_log"],
         "grandplus_step.h": ["gp_clip_adam_step_dev", "gp_step_advance", "gp_step_masks"],
         "grandplus_fit.h": ["gp_fit_select", "gp_fit_snapshot", "gp_fit_track_update"]}
N_PARAMS = {"gp_mlp_infer_block": 16, "gp_mlp_infer_chain2": 25, "gp_mag_prop_rows": 25, "gp_mag_prop_rows_backward": 24,
            "gp_clip_adam_step": 15, "gp_clip_adam_step_dev": 15, "gp_fit_select": 11}


def test_the_table_lists_the_headers_as_the_main_header_includes_them():
    import __graft_entry__ as entry
    main, _ = ah.read("grandplus.h")
    assert HEADERS == ["grandplus.h"] + re.findall(r'#include "(grandplus_\w+\.h)"', main) and set(HEADERS) == set(UNITS)
    public = sorted(glob.glob(os.path.join(ah.INC, "*.h")))
    assert public == sorted(os.path.join(ah.INC, h) for h in HEADERS)
    assert [s for s in entry.lib_sources() if s.endswith(".h")] == public
    assert '"row_order"' in main                                       # the option that grandplus_order.h's entry points report on
    # every entry name occurs under exactly one header
    names = [name for entries in _native.ABI.values() for name in entries]
    assert len(names) == len(set(names)) == N_MAIN + sum(len(v) for v in NAMES.values())
    for header in HEADERS:
        for other in HEADERS:
            assert header == other or not set(_native.ABI[header]) & set(ah.prototypes(other)), (header, other)
    # the exceptions to the convention are three parameters that exist
    params = {(name, p[2]) for h in HEADERS for name, (_, ps) in ah.prototypes(h).items() for p in ps}
    assert ah.HOST_AS_VOID <= params and len(ah.HOST_AS_VOID) == 3


@pytest.mark.parametrize("header", HEADERS)
def test_the_header_is_part_of_the_one_abi_and_the_one_library(header):
    import __graft_entry__ as entry
    main, _ = ah.read("grandplus.h")
    assert header == "grandplus.h" or f'#include "{header}"' in main
    assert "#define GP_ABI_VERSION 4\n" in main                      # one ABI, still version 4
    assert os.path.join(ah.INC, header) in entry.lib_sources()
    for unit in UNITS[header]:
        assert unit in entry.LIB_UNITS and os.path.join(entry.CSRC, unit) in entry.lib_sources()
    assert _native.lib().gp_abi_version() == 4
    assert _native.lib().gp_strerror(2) == b"invalid CSR"


def _table(header):
    return _native.PRIVATE_ABI[header] if header in PRIVATE else _native.ABI[header]


def test_the_private_headers_stay_outside_the_public_abi():
    # every entry name occurs exactly once across the two tables
    names = [name for table in (_native.ABI, _native.PRIVATE_ABI) for entries in table.values() for name in entries]
    assert len(names) == len(set(names))
    assert sorted(PRIVATE) == sorted(os.path.basename(p) for p in glob.glob(os.path.join(ah.CSRC, "*_abi.hpp")))
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ah.INC, "*")))
    for header in PRIVATE:
        assert header not in public and not [name for name in _native.PRIVATE_ABI[header] if name in public], header


def test_one_patch_of_the_binder_reaches_every_modules_loader(monkeypatch):
    """mag_det.lib, optim_rows.lib, gather_chunk.lib and fit.rows_lib go through `_native.lib` at each call, so the one patch
    by which the host tests prove "the native library was not reached" covers them; none holds a table of its own."""
    from grand_plus_amd import fit, gather_chunk, mag_det, optim_rows
    reached = object()
    monkeypatch.setattr(_native, "lib", lambda: reached)
    assert [f() for f in (mag_det.lib, optim_rows.lib, gather_chunk.lib, fit.rows_lib)] == [reached] * 4
    assert fit.ROWS_ABI is _native.PRIVATE_ABI["fit_rows_abi.hpp"]
    assert not [m.__name__ for m in (mag_det, optim_rows, gather_chunk) if hasattr(m, "ABI") or hasattr(m, "MARK_ABI")]


@pytest.mark.parametrize("header", HEADERS + PRIVATE)
def test_the_entries_are_the_headers_prototypes(header):
    protos = ah.prototypes(header)
    assert sorted(protos) == sorted(_table(header))
    if header == "grandplus.h":
        assert len(protos) == N_MAIN
    elif header in HEADERS:                                           # a private header's names stand in its module's own test
        assert sorted(protos) == NAMES[header]
    built = ctypes.CDLL(_native.LIB_PATH)
    for name in protos:
        assert hasattr(built, name), f"libgrandplus.so does not export {name}"


@pytest.mark.parametrize("header", HEADERS + PRIVATE)
def test_the_types_are_the_conventions_position_by_position(header):
    """Every entry of the table against the header's prototype: the count, and the one type the convention gives for each
    position; the loaded library carries exactly these."""
    for name, (ret, params) in ah.prototypes(header).items():
        restype, argtypes, required = _table(header)[name]
        assert isinstance(required, bool) if header == "grandplus.h" else required is False, name
        assert restype is ah.expected_ctype(name, *ret), f"{name}: restype {restype} for {ret}"
        assert len(argtypes) == len(params) == N_PARAMS.get(name, len(params)), f"{name}: {len(argtypes)} argtypes for {len(params)} parameters"
        for i, (got, want) in enumerate(zip(argtypes, params)):
            assert got is ah.expected_ctype(name, *want), f"{name}: argument {i} is {got} for {want}"
        f = getattr(_native.lib(), name)
        if isinstance(f, ctypes._CFuncPtr):
            assert f.argtypes == argtypes and f.restype is restype, name
        else:                                                         # the stub of a name an older build lacks
            assert header == "grandplus.h" and not required and f.__name__ == "missing", name


def test_the_device_form_of_the_optimiser_differs_in_two_positions():
    """gp_clip_adam_step_dev takes the value form's arguments, with two device pointers where that takes the two floats."""
    val, dev = _native.ABI["grandplus.h"]["gp_clip_adam_step"][1], _native.ABI["grandplus_step.h"]["gp_clip_adam_step_dev"][1]
    assert len(val) == len(dev) == 15 and [i for i in range(15) if val[i] != dev[i]] == [10, 11]
    assert val[10] == val[11] == ctypes.c_float and dev[10] == dev[11] == ctypes.c_void_p


# ---- the mirrors of the macros.  GP_MAX_SAMPLES and GP_MAX_CLASSES have no C macro (the headers give the two limits as numbers
# in their prose), so nothing holds them here.
NO_MACRO = ("GP_MAX_SAMPLES", "GP_MAX_CLASSES")
INFER = [(0, 1), (1, 1), (2, 1), (3, 7), (10000, 100), (2449029, 1024), (2 ** 40, 2 ** 22)]
CHAIN = [(0, 1, 1), (1, 1, 1), (2, 1, 2), (3, 7, 33), (10000, 100, 1024), (2449029, 100, 1024), (2 ** 40, 2 ** 30, 1024)]
# size function of _native -> (its macro, the argument tuples it is evaluated at): an argument that fits an int is written as
# one, so a product past 2^31 is right only through the macro's own int64_t casts
SIZES = {"optim_workspace_bytes": ("GP_OPTIM_WORKSPACE_BYTES", [()]),
         "eval_workspace_bytes": ("GP_EVAL_WORKSPACE_BYTES", [()]),
         "scatter_rows_workspace_bytes": ("GP_SCATTER_ROWS_WORKSPACE_BYTES", [(3, 7), (16, 2 ** 31 - 1)]),
         "scatter_bag_workspace_bytes": ("GP_SCATTER_BAG_WORKSPACE_BYTES", [(9,), (2 ** 31 - 1,)]),
         "mlp_saved_floats": ("GP_MLP_SAVED_FLOATS", [(2, 250, 602), (16, 2 ** 31 - 1, 2 ** 20)]),
         "mlp_forward_workspace_bytes": ("GP_MLP_FORWARD_WORKSPACE_BYTES", [(3,), (16,)]),
         "mlp_backward_workspace_bytes": ("GP_MLP_BACKWARD_WORKSPACE_BYTES", [(2, 250, 602), (16, 2 ** 20, 2 ** 12)]),
         "grand_loss_workspace_bytes": ("GP_GRAND_LOSS_WORKSPACE_BYTES", [(0,), (1,), (250,), (2 ** 40,)]),
         "mlp_infer_workspace_bytes": ("GP_MLP_INFER_WORKSPACE_BYTES", INFER),
         "mlp_infer_chain_workspace_bytes": ("GP_MLP_INFER_CHAIN_WORKSPACE_BYTES", CHAIN)}


PINNED = {"GP_MAX_K": 1024, "GP_STEP_MAX_GROUPS": 8, "GP_STEP_MAX_LAYERS": 8, "GP_STEP_SEG_ROWS": 0, "GP_STEP_SEG_LAYER": 1,
          "GP_FIT_STOP_ACC": 0, "GP_FIT_STOP_BOTH": 1, "GP_FIT_MAX_COPIES": 32,
          "GP_MLP_CHAIN_MAX_HIDDEN": 1024, "GP_MLP_CHAIN_MAX_OUT": 64, "GP_SCATTER_ROWS_WORKSPACE_BYTES(3, 7)": 4 * 3 * 7,
          "GP_SCATTER_BAG_WORKSPACE_BYTES(9)": 36, "GP_MLP_SAVED_FLOATS(2, 250, 602)": 2 * 250 + 4 * 2 * 602,
          "GP_MLP_FORWARD_WORKSPACE_BYTES(3)": 3 * 2097152,
          "GP_MLP_BACKWARD_WORKSPACE_BYTES(2, 250, 602)": 4 * (2 * 250 * 602 + 524288)}


def _macro(name, args):
    return name + ("(%s)" % ", ".join("%d" % a if a < 2 ** 31 else "%dLL" % a for a in args) if args else "")


def test_the_mirrors_equal_the_macros_as_the_c_compiler_evaluates_them():
    constants = [n for n, v in vars(_native).items() if re.fullmatch(r"GP_[A-Z0-9_]+", n) and isinstance(v, int) and n not in NO_MACRO]
    assert {"GP_OK", "GP_ERR_OVERFLOW", "GP_MAX_K", "GP_LOSS_L2", "GP_MLP_TRAINING", "GP_OPTIM_MAX_TENSORS", "GP_OPTIM_NORM_READY",
            "GP_EVAL_BAD", "GP_STEP_MAX_GROUPS", "GP_STEP_MAX_LAYERS", "GP_STEP_SEG_ROWS", "GP_STEP_SEG_LAYER",
            "GP_MLP_CHAIN_MAX_HIDDEN", "GP_MLP_CHAIN_MAX_OUT", "GP_FIT_STOP_ACC", "GP_FIT_STOP_BOTH", "GP_FIT_MAX_COPIES"} <= set(constants)
    # ... and every macro and status code of the headers has its mirror, but for the version and the step seed's multiplier
    code = "".join(ah.read(h)[1] for h in HEADERS)
    declared = set(re.findall(r"#define (GP_\w+)", code)) | set(re.findall(r"\b(GP_OK|GP_ERR_\w+)\s*=", code))
    assert declared - {"GP_ABI_VERSION", "GP_STEP_MUL"} == set(constants) | {macro for macro, _ in SIZES.values()}
    assert all(hasattr(_native, name) and name not in declared for name in NO_MACRO)
    sizes = [n for n, v in vars(_native).items() if callable(v) and re.search(r"_(bytes|floats)$", n)]
    assert sorted(sizes) == sorted(SIZES)
    want = {name: getattr(_native, name) for name in constants}
    for fn, (macro, tuples) in SIZES.items():
        for args in tuples:
            want[_macro(macro, args)] = getattr(_native, fn)(*args)
    got = dict(zip(want, ah.c_values(want)))
    assert got == want, {e: (got[e], want[e]) for e in want if got[e] != want[e]}
    assert all(0 <= v < 2 ** 63 for v in want.values())               # the macros' int64_t holds every value used here
    # what the numbers have to satisfy beyond being equal
    for expr, value in PINNED.items():
        assert got[expr] == value, expr
    assert got["GP_EVAL_WORKSPACE_BYTES"] == 1024 * (8 + 4 * 8)
    assert got["GP_OPTIM_WORKSPACE_BYTES"] <= 1024 * 8
    assert got["GP_OPTIM_MAX_TENSORS"] == oc.MAX_TENSORS == 32
    assert oc.MAX_TENSORS * 48 + 8 < 4096                             # the by-value table fits the kernel arguments
    assert got["GP_FIT_MAX_COPIES"] * 24 + 8 <= 1024                  # and so does the snapshot's, of 24-byte gp_fit_copy entries
    for n_rows, f_in in INFER:
        size = got[_macro("GP_MLP_INFER_WORKSPACE_BYTES", (n_rows, f_in))]
        assert size % 16 == 0 and 0 <= size - 4 * (n_rows + 2 * f_in) < 16
    for n_rows, f_in, f_hidden in CHAIN:
        size = got[_macro("GP_MLP_INFER_CHAIN_WORKSPACE_BYTES", (n_rows, f_in, f_hidden))]
        assert size % 16 == 0 and 0 <= size - 4 * (n_rows + 2 * f_in + 2 * f_hidden) < 16


# ---- the mirrors of the structs
PINNED_SIZEOF = {"gp_optim_tensor": 40, "gp_fit_track": 40, "gp_fit_copy": 24}


@pytest.mark.parametrize("header,struct,mirror", [
    ("grandplus.h", "gp_stats", _native.GpStats), ("grandplus.h", "gp_optim_tensor", _native.GpOptimTensor),
    ("grandplus_step.h", "gp_step_state", _native.GpStepState), ("grandplus_step.h", "gp_step_segment", _native.GpStepSegment),
    ("grandplus_fit.h", "gp_fit_track", _native.GpFitTrack), ("grandplus_fit.h", "gp_fit_copy", _native.GpFitCopy)])
def test_the_struct_mirrors_have_the_headers_fields_size_and_offsets(header, struct, mirror):
    """Field by field against the header's text, then sizeof and every offsetof as the C compiler lays the struct out."""
    _, code = ah.read(header)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w.*)", decl, flags=re.S)
        assert m, decl
        base, star, items = m.groups()
        for item in items.split(","):
            name, count = re.fullmatch(r"(\w+)(?:\[(\w+)\])?", item.strip()).groups()
            want = ctypes.c_void_p if star else ah.SCALARS[base]       # a device pointer travels as an integer
            if count:
                want = want * (int(count) if count.isdigit() else getattr(_native, count))
            fields.append((name, want))
    assert [(n, t) for n, t in mirror._fields_] == fields
    names = [n for n, _ in fields]
    got = ah.c_values([f"sizeof({struct})"] + [f"offsetof({struct}, {n})" for n in names])
    assert got == [ctypes.sizeof(mirror)] + [getattr(mirror, n).offset for n in names]
    if struct == "gp_step_state":
        assert got == [88, 0, 8, 16, 20, 52]
    if struct in PINNED_SIZEOF:
        assert got[0] == PINNED_SIZEOF[struct]
