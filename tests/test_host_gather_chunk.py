"""CPU tests of the chunked deterministic segment sums: what is particular to the entry points of
csrc/gather_chunk_abi.hpp in _native.PRIVATE_ABI (tests/test_host_abi.py holds the types), their error codes before any GPU
work, every refusal of the Python layer before a device call, the audit of tests/gather_chunk_cases.py with deliberate
mistakes, and csrc/gather_chunk_layout.hpp itself (tests/native/gather_chunk_check.cpp, built with the address and
undefined-behaviour sanitizers and run as a program) against brute force."""
import ctypes
import glob
import inspect
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import abi_header as ah
import gather_chunk_cases as gcc
import native_check
from grand_plus_amd import _native
from grand_plus_amd import gather_chunk as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")
P = ctypes.c_void_p(16)
NAMES = ["gp_embedding_bag_backward_det_chunked", "gp_mag_prop_rows_backward_det_chunked", "gp_random_prop_rows_backward_det_chunked"]
BAD_CHUNKS = (0, 1, 32, 63, 65, 96, 192, 4095, 8192, -64)


# ---- 1. the binding
def _code(name):
    text = open(os.path.join(CSRC, name)).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_table_is_the_headers_prototypes_position_by_position():
    """The generic part -- every type by the convention, the library's exports -- is tests/test_host_abi.py's."""
    protos = ah.prototypes("gather_chunk_abi.hpp")
    assert sorted(protos) == sorted(_native.PRIVATE_ABI["gather_chunk_abi.hpp"]) == NAMES
    # each takes its unchunked twin's arguments up to the stream, name by name, then chunk, d_scratch, scratch_bytes, stream
    scatter = ah.prototypes("grandplus_scatter.h")
    mag = ah.prototypes("mag_det_abi.hpp")
    for name, twin in (("gp_random_prop_rows_backward_det_chunked", scatter["gp_random_prop_rows_backward_det"]),
                       ("gp_embedding_bag_backward_det_chunked", scatter["gp_embedding_bag_backward_det"]),
                       ("gp_mag_prop_rows_backward_det_chunked", mag["gp_mag_prop_rows_backward_det"])):
        got = protos[name][1]
        assert got[:-4] == twin[1][:-1] and got[-1] == twin[1][-1] == ("void", 1, "stream")
        assert got[-4:-1] == [("int32_t", 0, "chunk"), ("float", 1, "d_scratch"), ("int64_t", 0, "scratch_bytes")]


def test_the_entry_points_stay_outside_c_abi_4():
    import __graft_entry__ as entry
    for hdr in ("gather_chunk.hpp", "gather_chunk_abi.hpp", "gather_chunk_layout.hpp"):
        assert os.path.join(CSRC, hdr) in entry.lib_sources()
    public = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert "chunked" not in public and "GATHER_CHUNK" not in public
    assert not [n for n in vars(_native) if "CHUNKED" in n.upper() or "GATHER_CHUNK" in n.upper()]
    assert _native.lib().gp_abi_version() == 4


def test_the_kernels_are_stated_once_with_plain_stores_and_the_layout_is_hip_free():
    unit = _code("gather_chunk.hpp")
    assert not re.search(r"atomic|\basm\b|printf|assert\s*\(|__builtin_amdgcn_s_|hipMalloc|hipMemcpy|Synchronize", unit)
    for call in ("gc::seg_start_of(", "gc::starts_chunk(", "gc::chunk_of(", "gc::slot_of(", "gc::is_long(", "gc::chunk_start(",
                 "gp_gather_chunk::scratch_bytes(", "gp_gather_chunk::chunk_ok(", "gather_grid(n_sorted)", "op.load(", "op.add("):
        assert call in unit, call
    for name in ("gather_chunk_kernel(Op op", "gather_fold_kernel(const long long*"):
        holders = [os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*")) if name in open(p, errors="replace").read()]
        assert holders == ["gather_chunk.hpp"], (name, holders)
    for hip, ops in (("scatter_det.hip", ("RowsOp", "BagOp")), ("mag_det.hip", ("MagOp",))):
        text = open(os.path.join(CSRC, hip)).read()
        assert '#include "gather_chunk.hpp"' in text and '#include "gather_chunk_abi.hpp"' in text
        for op in ops:
            assert f"gather_sum_kernel<{op}>" in text and f'"gather_chunk_kernel<{op}>"' in text
    layout = open(os.path.join(CSRC, "gather_chunk_layout.hpp")).read()
    assert re.findall(r"#include\s*[<\"]([^>\"]+)", layout) == ["cstdint"]


def _body(text, name):
    i = text.index(f"\nint {name}(")
    return [ln.strip() for ln in text[text.index("\n{\n", i) + 3:text.index("\n}\n", i)].splitlines()]


def test_each_deterministic_backward_has_one_body_and_its_entry_points_only_name_themselves():
    """The rows pair and the MAG pair share one body each: the pre-pass is launched on one line of its unit, the Op and the
    arguments are built once, and an entry point holds its own name and no launch.  The pre-pass's grid cap stands on that
    one line, where source_caps() reads it."""
    import second_trip_cases as st
    scatter = open(os.path.join(CSRC, "scatter_det.hip")).read()
    mag = open(os.path.join(CSRC, "mag_det.hip")).read()
    assert len([ln for ln in scatter.splitlines() if "rows_inv_den_kernel," in ln]) == 1 and scatter.count("const RowsOp op") == 1
    assert len([ln for ln in mag.splitlines() if "mag_slot_grad_kernel," in ln]) == 1
    assert mag.count("const MagArgs A") == 1 and mag.count("const MagOp op") == 1
    for path in glob.glob(os.path.join(CSRC, "*")):
        assert "rows_den_grid" not in open(path, errors="replace").read(), path
    for text, twin in ((scatter, "gp_random_prop_rows_backward_det"), (mag, "gp_mag_prop_rows_backward_det")):
        for name in (twin, twin + "_chunked"):
            body = "\n".join(_body(text, name))
            assert f'"{name}"' in body and "hipLaunchKernelGGL" not in body, name
            assert f'"{twin}_chunked"' not in body if name == twin else f'"{twin}"' not in body, name
    assert st.source_caps()["rows_den_grid"] == 65535
    # the bag twin runs its pre-pass through the unchunked entry point itself: nothing is repeated there
    bag = "\n".join(_body(scatter, "gp_embedding_bag_backward_det_chunked"))
    assert "gp_embedding_bag_backward_det(device," in bag and "bag_inv_den_kernel" not in bag


def test_the_scratch_macro_is_the_layout_headers_and_the_bindings_figure(tmp_path):
    shapes = [(1, 64, 1), (64, 64, 7), (65, 64, 7), (4097, 256, 257), (4_196_864, 64, 1), (2 ** 31 + 5, 4096, 512), (0, 64, 3)]
    src = tmp_path / "macro.cpp"
    src.write_text('#include <cstdio>\n#include "gather_chunk_abi.hpp"\n#include "gather_chunk_layout.hpp"\nint main() {\n' +
                   "".join(f'  std::printf("%lld %lld\\n", (long long)GP_GATHER_CHUNK_SCRATCH_BYTES({n}ll, {c}, {w}), '
                           f'gp_gather_chunk::scratch_bytes({n}ll, {c}, {w}));\n' for n, c, w in shapes) + "  return 0;\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o",
                    str(tmp_path / "macro"), str(src)], check=True, timeout=120)
    out = subprocess.run([str(tmp_path / "macro")], check=True, capture_output=True, text=True).stdout.split()
    for (n, c, w), macro, layout in zip(shapes, out[0::2], out[1::2]):
        assert int(macro) == int(layout) == gc.scratch_bytes(n, c, w) == 2 * -(-n // c) * w * 4


# ---- 2. error codes
def test_the_entries_return_their_error_codes_before_any_gpu_work():
    """No device pointer here is real: every call has to stop at its argument checks."""
    E, N, OK = _native.GP_ERR_INVALID_ARG, _native.GP_ERR_NULL, _native.GP_OK
    L = _native.lib()

    def rows(g=P, B=4, F=7, col=P, val=P, K=5, S=2, p=0.5, gx=P, n_nodes=9, order=P, keys=P, n_sorted=20, inv=P, chunk=64,
             scratch=P, nbytes=None):
        nbytes = gc.scratch_bytes(n_sorted, 64, F) if nbytes is None else nbytes
        return L.gp_random_prop_rows_backward_det_chunked(0, g, B, F, col, val, None, K, None, S, p, 1, ctypes.c_uint64(1), None, 0, gx,
                                                          n_nodes, order, keys, n_sorted, inv, chunk, scratch, nbytes, None)

    def bag(g=P, V=50, H=7, offsets=P, n_src=4, n_rows=4, idx=P, idx_bytes=8, data=P, p=0.0, dW=P, order=P, keys=P, srows=P,
            n_sorted=20, inv=P, chunk=64, scratch=P, nbytes=None):
        nbytes = gc.scratch_bytes(n_sorted, 64, H) if nbytes is None else nbytes
        return L.gp_embedding_bag_backward_det_chunked(0, g, V, H, offsets, n_src, None, None, n_rows, idx, idx_bytes, data, p, 0,
                                                       ctypes.c_uint64(1), None, dW, None, order, keys, srows, n_sorted, inv, chunk,
                                                       scratch, nbytes, None)

    def mag(g=P, V=50, H=7, indptr=P, K=5, B=4, S=2, p_in=0.0, training=1, base=P, order=P, skeys=P, cap=100, U=P, inv=P, dW=P,
            chunk=64, scratch=P, nbytes=None):
        nbytes = gc.scratch_bytes(cap, 64, H) if nbytes is None else nbytes
        return L.gp_mag_prop_rows_backward_det_chunked(0, g, V, H, indptr, P, P, 12, P, P, None, 6, K, None, B, S, 0.5, p_in, training,
                                                       ctypes.c_uint64(1), None, 0, base, order, skeys, cap, U, inv, dW, chunk, scratch,
                                                       nbytes, None)

    for call in (rows, bag, mag):
        for c in BAD_CHUNKS:
            assert call(chunk=c) == E, (call.__name__, c)
        assert "chunk is not a power of two in [64, 4096]" in L.gp_last_error().decode()
        assert call(nbytes=gc.scratch_bytes(100 if call is mag else 20, 64, 7) - 1) == E          # one byte short
        assert "scratch" in L.gp_last_error().decode() and call.__name__ in L.gp_last_error().decode()
        assert call(nbytes=0) == E
        assert call(scratch=None) == N
        assert call(chunk=48, scratch=None) == E                                # the chunk is judged before the scratch
    # the twin's own checks come first, and what is left to do without a batch needs no scratch
    for kw in (dict(S=0), dict(S=17), dict(p=1.5), dict(B=-1), dict(F=0), dict(K=0), dict(K=1025), dict(n_nodes=0), dict(n_sorted=-1)):
        assert rows(**kw) == E, kw
    assert rows(S=0, chunk=48) == E and "n_samples" in L.gp_last_error().decode()
    assert rows(B=0, scratch=None, nbytes=0) == OK and rows(n_sorted=0, scratch=None, nbytes=0, g=None) == OK
    assert rows(B=0, chunk=48) == E
    for name in ("g", "col", "val", "gx", "order", "keys", "inv"):
        assert rows(**{name: None}) == N, name
    for kw in (dict(V=-1), dict(H=0), dict(n_src=-1), dict(n_rows=-1), dict(n_sorted=-1), dict(idx_bytes=2), dict(p=1.5)):
        assert bag(**kw) == E, kw
    assert bag(n_rows=0, scratch=None, nbytes=0) == OK and bag(n_rows=0, chunk=48) == E
    for name in ("order", "keys", "srows", "offsets", "idx", "data", "g", "inv", "dW"):
        assert bag(**{name: None}) == N, name
    for kw in (dict(V=0), dict(H=0), dict(K=0), dict(K=1025), dict(B=-1), dict(S=0), dict(S=17), dict(cap=0), dict(B=2 ** 21, K=1024),
               dict(p_in=0.5), dict(p_in=0.5, B=0)):
        assert mag(**kw) == E, kw
    assert mag(p_in=0.5) == E and "input dropout" in L.gp_last_error().decode()   # refused chunked as unchunked
    assert mag(p_in=0.5, training=0, B=0, scratch=None, nbytes=0) == OK
    assert mag(B=0, scratch=None, nbytes=0) == OK and mag(B=0, chunk=48) == E
    for name in ("g", "indptr", "base", "order", "skeys", "U", "inv", "dW"):
        assert mag(**{name: None}) == N, name


# ---- 3. the Python layer
def test_check_chunk_takes_powers_of_two_from_64_to_4096():
    assert gc.check_chunk(None) is None
    assert [gc.check_chunk(c) for c in (64, 128, 256, 512, 1024, 2048, 4096)] == [64, 128, 256, 512, 1024, 2048, 4096]
    for bad in BAD_CHUNKS + (64.0, "64", True, [64]):
        with pytest.raises(ValueError, match="segment_chunk must be None or a power of two in \\[64, 4096\\]"):
            gc.check_chunk(bad)
    assert (gc.MIN_CHUNK, gc.MAX_CHUNK) == (64, 4096)


def test_every_call_refuses_before_any_device_call(monkeypatch):
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    from grand_plus_amd.mag import mag_prop_rows
    from grand_plus_amd.mlp import MagMLP
    from test_host_mag_det import _fake_cuda, _host_args, _mag_step
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("the native library was reached"))
    z = torch.zeros(4)
    model = MagMLP(9, 3, 4, 2, True, 0.0, 0.5, True)
    calls = {
        "random_prop_rows": lambda **kw: random_prop_rows(torch.zeros((3, 2)), z.int(), z.double(), None, 2, **kw),
        "embedding_bag": lambda **kw: embedding_bag(torch.zeros((3, 2)), z.long(), z.long(), z, **kw),
        "embedding_bag_csr": lambda **kw: embedding_bag_csr(torch.zeros((3, 2)), z.long(), z.int(), z, **kw),
        "mag_prop_rows": lambda **kw: mag_prop_rows(**_host_args(), max_entries=100, **kw),
        "emb": lambda **kw: model.emb(z.long(), z.long(), z, **kw),
        "emb_csr": lambda **kw: model.emb_csr(z.long(), z.int(), z, **kw),
        "MagTrainStep": lambda **kw: _mag_step(**kw),
    }
    for name, call in calls.items():
        for bad in (48, 32, 8192, 64.0, True):
            with pytest.raises(ValueError, match="segment_chunk must be None or a power of two"):
                call(segment_chunk=bad, deterministic=True)
        # with the atomic backward the keyword would do nothing: refused, whether the mode is given or follows torch's flag
        for kw in (dict(deterministic=False), dict()):
            with pytest.raises(ValueError, match="segment_chunk= of .* needs deterministic=True"):
                call(segment_chunk=64, **kw)
    with pytest.raises(ValueError, match="segment_chunk= of mag_prop_rows"):
        from grand_plus_amd.rows import RowMatrix                                  # emb_rows passes the keyword on
        zz = torch.zeros(8, dtype=torch.int32)
        model.emb_rows(torch.zeros(13, dtype=torch.int64), z.int(), z, RowMatrix(np.arange(2), 4, zz, zz, torch.zeros(8, dtype=torch.float64),
                                                                                torch.full((2,), 4, dtype=torch.int32), 12), segment_chunk=64)
    torch.use_deterministic_algorithms(True)
    try:                                                                         # None follows torch's flag: past the refusal
        with pytest.raises(ValueError, match="no CPU fallback"):
            _mag_step(segment_chunk=256)
    finally:
        torch.use_deterministic_algorithms(False)
    with pytest.raises(ValueError, match="no CPU fallback"):                     # everything else passes: only the device is missing
        _mag_step(segment_chunk=64, deterministic=True, table_step="lazy", dirty_rows=True)
    # input dropout stays refused in the MAG path, chunked or not
    a = {k: _fake_cuda(v) if isinstance(v, torch.Tensor) else v for k, v in _host_args().items()}
    a["weight"] = _fake_cuda(_host_args()["weight"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="does not support input dropout"):
        mag_prop_rows(**a, deterministic=True, max_entries=100, input_droprate=0.5, segment_chunk=64)


def test_the_keyword_defaults_to_todays_call():
    from grand_plus_amd import MagTrainStep
    from grand_plus_amd.augment import random_prop_rows
    from grand_plus_amd.embedding import embedding_bag, embedding_bag_csr
    from grand_plus_amd.mag import mag_prop_rows
    from grand_plus_amd.mag_det import backward_det
    from grand_plus_amd.mlp import MagMLP
    for f in (random_prop_rows, embedding_bag, embedding_bag_csr, mag_prop_rows, backward_det, MagMLP.emb, MagMLP.emb_csr,
              MagMLP.emb_rows, MagTrainStep.__init__):
        assert inspect.signature(f).parameters["segment_chunk"].default is None, f.__qualname__
    src = inspect.getsource(MagTrainStep._front)
    assert "segment_chunk=self.segment_chunk" in src


# ---- 4. the cases under deliberate mistakes
H_AUDIT = 65


@pytest.mark.parametrize("name", sorted(gcc.CASES))
def test_every_case_tells_the_mistakes_it_claims_from_the_contract(name):
    c = gcc.CASES[name]
    e, want = gcc.entries(name, H_AUDIT), gcc.expected(name, H_AUDIT)
    target = c["target"]
    for mistake in gcc.pins(name):
        got = gcc.MISTAKES[mistake][0](e["sorted_keys"], e["terms"], e["n_dest"], c["C"])
        assert got.tobytes() != want.tobytes(), f"{name} does not tell '{mistake}' from the contract"
    if target is not None and c["segs"][target] > c["C"] + 1:
        assert {"plain left to right", "chunk 2C", "chunk C/2"} <= set(gcc.pins(name))
    # the rows nothing names stay zero, and the sentinel tail adds nothing
    assert not want[len(c["segs"]):].any() and want.shape == (len(c["segs"]) + 2, H_AUDIT)


def test_every_mistake_is_told_by_some_case_and_single_columns_tell_them_too():
    told = {m: [n for n in gcc.CASES if m in gcc.pins(n)] for m in gcc.MISTAKES}
    assert all(len(v) >= 3 for v in told.values()), told
    assert len(gcc.MISTAKES) == 6
    # H = 1: with 65 chunks one float per destination still differs under every mistake (two orders of three partials can
    # agree in a single float by chance, which is why the audit above runs at H = 65)
    for name in ("c64_n4097_at1", "c64_n4097_at63"):
        e, want = gcc.entries(name, 1), gcc.expected(name, 1)
        for mistake in gcc.pins(name):
            got = gcc.MISTAKES[mistake][0](e["sorted_keys"], e["terms"], e["n_dest"], gcc.CASES[name]["C"])
            assert got.tobytes() != want.tobytes(), (name, mistake)


def test_segments_of_at_most_c_are_the_left_to_right_walk_bitwise():
    rng = np.random.default_rng(5)
    for C, lens in ((64, [1, 63, 64, 2, 64, 17]), (256, [256, 255, 1, 200]), (4096, [4096, 3])):
        keys = np.repeat(np.arange(len(lens)), lens)
        terms = (rng.standard_normal((len(keys), 3)) * 10.0 ** rng.integers(-3, 4, (len(keys), 1))).astype(np.float32)
        terms[rng.random(len(keys)) < 0.2] = -0.0                                # positions that contribute a negative zero
        a, b = gcc.chunked_sum(keys, terms, len(lens), C), gcc.left_to_right(keys, terms, len(lens))
        assert a.tobytes() == b.tobytes()
    # 0.0f + partial_0 == partial_0 bit for bit: a sum from +0.0f is never -0.0f
    x = np.array([[-0.0], [-0.0]], np.float32)
    assert gcc.chunked_sum([0, 0], x, 1, 64).tobytes() == np.zeros((1, 1), np.float32).tobytes()


@pytest.mark.parametrize("name", sorted(gcc.CASES))
def test_the_kernels_mapping_gives_the_contract_on_every_case(name):
    """gather_chunk.hpp's windows, heads, walks, scratch rows and fold, restated in numpy over NaN-filled scratch: the
    contract's bits, no scratch row written twice, every row inside the scratch."""
    c = gcc.CASES[name]
    e = gcc.entries(name, 3)
    got, written = gcc.mapping_model(e["sorted_keys"], e["terms"], e["n_dest"], c["C"])
    assert got.tobytes() == gcc.expected(name, 3).tobytes()
    assert all(0 <= s < 2 * -(-len(e["sorted_keys"]) // c["C"]) for s in written)
    n_long_chunks = sum(-(-n // c["C"]) for n in c["segs"] if n > c["C"])
    assert len(written) == n_long_chunks
    if name == "adjacent_at10":                                                  # both rows of one span are in use
        assert any(s % 2 == 0 and s + 1 in written for s in written)


# ---- 5. the layout header
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = native_check.build(tmp_path_factory, "gather_chunk_check")
    return lambda lines: native_check.ints(native_check.run(exe, lines))


def test_the_layout_header_needs_nothing_but_the_standard_library(tmp_path):
    src = tmp_path / "only_layout.cpp"
    src.write_text('#include "gather_chunk_layout.hpp"\nint main() { long long k[3] = {1, 2, 2}; '
                   'return (int)gp_gather_chunk::seg_start_of(k, 3, 2) - 1; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, "-o", str(tmp_path / "only_layout"), str(src)], check=True,
                   timeout=120)
    subprocess.run([str(tmp_path / "only_layout")], check=True, timeout=60)


def test_chunk_ok_is_check_chunk(checker):
    values = list(BAD_CHUNKS) + [64, 128, 256, 512, 1024, 2048, 4096, 2 ** 40]
    got = checker([f"ok {c}" for c in values])
    assert [g[0] for g in got] == [int(c in (64, 128, 256, 512, 1024, 2048, 4096)) for c in values]


def _brute_segment(q0, n, C):
    """Chunk number and chunk-start flag of every position of a segment, by counting."""
    out, p = [], -1
    for i in range(n):
        if i % C == 0:
            p += 1
        out += [p, int(i % C == 0)]
    return out


@pytest.mark.parametrize("C", [64, 256, 4096])
def test_counts_starts_slots_and_sizes_are_brute_force(checker, C):
    ns = [1, C - 1, C, C + 1, 2 * C, 2 * C + 1]
    starts = [0, 1, 63, 64, C - 1]
    lines, want = [], []
    for start in starts:
        for n in ns:
            lens = ([start] if start else []) + [n, 5]
            lines.append(f"slots {C} " + " ".join(map(str, lens)))
            lines.append(f"where {C} {start} {n}")
            want.append((start, n, lens))
    got = checker(lines)
    for (start, n, lens), slots, where in zip(want, got[0::2], got[1::2]):
        total = sum(lens)
        rows = 2 * len(range(0, total, C))
        assert slots[:2] == [rows, rows * 7 * 4]
        it, q0, used = iter(slots[2:]), 0, []
        for ln in lens:
            P = next(it)
            assert P == len(range(0, ln, C))
            for p in range(P):
                q, slot = next(it), next(it)
                assert q == q0 + p * C
                if ln > C:
                    assert 0 <= slot < rows and slot // 2 == q // C
                    used.append(slot)
                else:
                    assert slot == -1
            q0 += ln
        assert not list(it) and len(set(used)) == len(used)
        assert where == _brute_segment(start, n, C)


@pytest.mark.parametrize("C", [64, 256, 4096])
def test_two_rows_per_span_hold_every_arrangement_of_up_to_four_segments(checker, C):
    """Every arrangement of one to four segments with lengths from {1, 2, C-1, C, C+1, 2C+1}: the chunks of the long
    segments take distinct scratch rows inside the scratch, at most two of them start in any aligned span of C positions,
    and of those at most one is a chunk 0."""
    lengths = [1, 2, C - 1, C, C + 1, 2 * C + 1]
    arrangements = [a for k in range(1, 5) for a in itertools.product(lengths, repeat=k)]
    assert len(arrangements) == 6 + 36 + 216 + 1296
    got = checker([f"slots {C} " + " ".join(map(str, a)) for a in arrangements])
    for a, line in zip(arrangements, got):
        rows, it = line[0], iter(line[2:])
        assert rows == 2 * len(range(0, sum(a), C))
        used, per_span = [], {}
        for n in a:
            for p in range(next(it)):
                q, slot = next(it), next(it)
                if n > C:
                    used.append(slot)
                    per_span.setdefault(q // C, []).append(p)
        assert len(set(used)) == len(used) and all(0 <= s < rows for s in used), a
        assert all(len(ps) <= 2 and sum(p == 0 for p in ps) <= 1 and sum(p > 0 for p in ps) <= 1 for ps in per_span.values()), a


@pytest.mark.parametrize("C", [64, 256])
def test_key_arrays_sorted_unsorted_and_all_sentinel_stay_inside_the_scratch(checker, C):
    """seg_start_of over the real blocks: the lower bound on sorted keys, a position inside [0, base) on any array; is_long
    reads keys[q + C] only where it exists; every slot a position can give lies inside the scratch."""
    rng = np.random.default_rng(C)
    sorted_keys = np.repeat(np.arange(7), [1, 63, C, C + 1, 2 * C + 1, 3, 130])
    arrays = {"sorted": sorted_keys, "unsorted": rng.integers(0, 4, 5 * C + 17), "descending": sorted_keys[::-1],
              "sentinel": np.full(3 * C + 1, 9), "one run": np.zeros(4 * C, np.int64), "short": np.array([2, 2, 2])}
    got = checker([f"keys {C} " + " ".join(map(str, k.tolist())) for k in arrays.values()])
    for (name, keys), line in zip(arrays.items(), got):
        n = len(keys)
        rows, top = line[:2]
        bases = list(range(64, n, 64))
        starts, longs = line[2:2 + len(bases)], line[2 + len(bases):]
        assert rows == 2 * -(-n // C) and 0 <= top < rows, name
        assert len(longs) == n
        assert longs == [int(q + C < n and keys[q + C] == keys[q]) for q in range(n)], name
        for b, s in zip(bases, starts):
            if keys[b - 1] != keys[b]:
                assert s == -1
                continue
            assert 0 <= s <= b - 1, (name, b, s)
            assert s == gcc.seg_start_of(keys, b, keys[b]), name
            if name in ("sorted", "sentinel", "one run"):
                assert s == int(np.searchsorted(keys[:b], keys[b], "left")), (name, b)
