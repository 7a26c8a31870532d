"""The headers as the host tests read them -- the public ones under include/, the private csrc/*_abi.hpp --: the header
reader, the prototype parser, the pointer convention of the binding (stated above _native.ABI) as a function, and the C
compiler as the judge of macros, sizeof and offsetof."""
import ctypes
import os
import re
import subprocess
import tempfile

from grand_plus_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")


def read(header):
    """(text, code) of include/<header>, or of csrc/<header> for a private *.hpp: as written, and with /* */ and //
    comments removed."""
    text = open(os.path.join(CSRC if header.endswith(".hpp") else INC, header)).read()
    return text, re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _ctype(decl):
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\**)", decl.strip())
    assert m, decl
    return m.group(1), len(m.group(2))


def prototypes(header):
    """name -> (return type, [parameters]) of every gp_* prototype of the header: the return type as (base type without
    const, number of *), a parameter as (base type, number of *, parameter name)."""
    _, code = read(header)
    protos = {}
    for ret, name, params in re.findall(r"\b((?:const\s+)?\w+\s*\**)\s*\b(gp_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", code):
        assert name not in protos, f"{header} declares {name} twice"
        params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)(\w+)", p.strip(), flags=re.S).groups() for p in params.split(",")]
        protos[name] = (_ctype(ret), [_ctype(decl) + (pname,) for decl, pname in params])
    assert sorted(re.findall(r"\b(gp_[a-z_0-9]+)\s*\(", code)) == sorted(protos), f"{header}: a gp_*( that is no prototype"
    return protos


SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint8_t": ctypes.c_uint8,
           "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
STRUCTS = {"gp_stats": _native.GpStats, "gp_optim_tensor": _native.GpOptimTensor, "gp_step_segment": _native.GpStepSegment,
           "gp_fit_copy": _native.GpFitCopy}
# host arrays that the binding declares c_void_p all the same (the comment on the entry in _native.ABI says why)
HOST_AS_VOID = {("gp_internal_graph_acsr", "h_acsr"), ("gp_internal_graph_acsr", "h_node_pos"), ("gp_internal_graph_acsr", "h_unit_info")}


def expected_ctype(entry, base, stars, param=None):
    """The one ctypes type the binding declares for a return type (param=None) or a parameter of `entry`."""
    if stars == 0:
        return None if base == "void" else SCALARS[base]
    if stars == 2:                                                   # gp_graph**, const int**: an array of pointers held as integers
        return ctypes.POINTER(ctypes.c_void_p)
    assert stars == 1, (entry, base, stars)
    if base == "char":
        return ctypes.c_char_p
    if base in ("void", "gp_graph", "gp_step_state") or (param or "").startswith("d_") or (entry, param) in HOST_AS_VOID:
        return ctypes.c_void_p                                       # device memory, a stream, an opaque handle: an integer
    return ctypes.POINTER(STRUCTS.get(base) or SCALARS[base])       # a host array


def c_values(exprs):
    """The integer value of each C expression (a macro at given arguments, a sizeof, an offsetof), as a host C program that
    includes grandplus.h prints them."""
    exprs = list(exprs)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "values.c"), os.path.join(tmp, "values")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "grandplus.h"\nint main(void) {\n' +
                    "".join(f'  printf("%lld\\n", (long long)({e}));\n' for e in exprs) + "  return 0;\n}\n")
        subprocess.run(["gcc", "-I" + INC, "-o", exe, src], check=True)
        got = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(exprs)
    return got
