"""The stand-alone check programs of tests/native/ as the host tests build and run them: one g++ line with the address and
undefined-behaviour sanitizers linked into the program itself (nothing is preloaded), queries as lines on stdin."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "grand_plus_amd", "csrc")


def build(tmp_path_factory, name):
    """The path of the program built from tests/native/<name>.cpp, which includes the HIP-free headers of csrc/."""
    if shutil.which("g++") is None:
        pytest.fail(f"g++ is needed to build tests/native/{name}.cpp")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC,
                    "-o", exe, os.path.join(ROOT, "tests", "native", name + ".cpp")], check=True, timeout=300)
    return exe


def run(exe, lines):
    """The program's output lines for the query lines.  It has to end clean: a sanitizer report ends the program."""
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def ints(out):
    return [[int(x) for x in ln.split()] for ln in out]
