"""The guarded C boundary (sparsecholesky_amd/csrc/capi_guard.hpp): a failing entry point leaves a
message that begins with its own name, never an earlier call's; a succeeding call leaves the
message alone; no exception crosses extern "C".  Argument and exception paths only: no GPU."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

import sparsecholesky_amd as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SC_ERR_ARG = -1
NOT_A_STATUS = {"sc_flops", "sc_free_symbolic", "sc_numeric_stream", "sc_free_numeric", "sc_normal_free",
                "sc_normal_values_ptr"}


def _handle_first():
    """(return type, name) of every declared function whose first parameter is a handle."""
    out = []
    for fn in ("sparsecholesky.h", "sparsecholesky_debug.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", fn)).read(), flags=re.S)
        for ret, name, first in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(sc_\w+)\s*\(\s*([^,)]*)", txt):
            if re.fullmatch(r"(const\s+)?sc_(symbolic|numeric|normal)\s*\*\s*\w+", first.strip()):
                out.append((" ".join(ret.split()), name))
    return out


HANDLE_FIRST = _handle_first()
STATUS_ENTRIES = sorted(name for ret, name in HANDLE_FIRST if ret == "int64_t")


def _plant(L):
    out = ctypes.c_void_p()
    assert L.sc_analyze_schur(4, None, None, None, -1, None, ctypes.byref(out)) == SC_ERR_ARG
    assert L.sc_last_error() == b"sc_analyze_schur: ns = -1 < 0"


def test_the_sweep_covers_every_handle_entry_point():
    assert len(STATUS_ENTRIES) >= 95
    assert {name for ret, name in HANDLE_FIRST if ret != "int64_t"} == NOT_A_STATUS
    assert set(STATUS_ENTRIES) <= set(sc.exported_symbols())


@pytest.mark.parametrize("name", STATUS_ENTRIES)
def test_null_handle_names_the_entry_point(name):
    L = sc.lib()
    f = getattr(L, name)
    _plant(L)
    zeros = [None if issubclass(t, (ctypes._Pointer, ctypes.c_void_p)) else 0 for t in f.argtypes[1:]]
    assert f(None, *zeros) == SC_ERR_ARG
    assert L.sc_last_error().decode().startswith(name), L.sc_last_error()


def test_an_earlier_message_is_not_reported():
    L = sc.lib()
    _plant(L)
    assert L.sc_symbolic_pattern(None, None, None) == SC_ERR_ARG
    assert L.sc_last_error().startswith(b"sc_symbolic_pattern"), L.sc_last_error()
    with pytest.raises(sc.LibraryError) as e:
        sc._check(L.sc_symbolic_pattern(None, None, None), "pattern")
    assert "sc_analyze_schur" not in str(e.value)


def test_a_successful_call_keeps_the_last_failing_message():
    L = sc.lib()
    s = sc.Symbolic(sc.laplacian3d(3))
    _plant(L)
    assert L.sc_nnz_L(s.h) > 0 and L.sc_symbolic_perm(s.h, None) >= 0
    assert L.sc_last_error() == b"sc_analyze_schur: ns = -1 < 0"


_EREACH = """
import ctypes, numpy as np, sparsecholesky_amd as sc
L = sc.lib()
Ap, Ai, parent = np.zeros(3, np.int64), np.zeros(1, np.int32), np.full(2, -1, np.int32)
s, w = np.zeros(2, np.int32), np.zeros(2, np.int32)
p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
rc = L.sc_ereach(1 << 62, p(Ap), p(Ai), None, 0, p(parent), p(s), p(w), None)
print({-2: "SC_ERR_NOMEM"}.get(rc, rc), "|", L.sc_last_error().decode())
"""


def test_an_exception_does_not_cross_the_boundary():
    r = subprocess.run([sys.executable, "-c", _EREACH], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr)
    status, msg = (t.strip() for t in r.stdout.strip().split("|"))
    assert status == "SC_ERR_NOMEM" and msg.startswith("sc_ereach"), r.stdout


def test_guard_alone_under_sanitizers(tmp_path):
    """tests/cpp/test_capi_guard.cpp: every outcome of a guarded call, and the wrapper of a failed
    handle creation is freed (the leak check)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    out = str(tmp_path / "test_capi_guard")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    "-I", os.path.join(ROOT, "tests", "cpp"),
                    os.path.join(ROOT, "tests", "cpp", "test_capi_guard.cpp"), "-o", out], check=True)
    r = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failed" in r.stdout
