"""The multi-right-hand-side solve at the C-ABI and Python boundary; no device needed."""
import ctypes
import inspect

import numpy as np
import pytest

import sparsecholesky_amd as sc


def test_null_handle_is_an_argument_error():
    L = sc.lib()
    assert L.sc_solve_device_multi(None, 1, None, 0, None, 0) == -1
    assert L.sc_solve_host_multi(None, 1, None, 0, None, 0) == -1
    assert b"sc_solve_host_multi" in L.sc_last_error()


def test_python_table_binds_both_symbols():
    names = sc.exported_symbols()
    assert "sc_solve_device_multi" in names and "sc_solve_host_multi" in names
    L = ctypes.CDLL(sc.LIB_PATH)
    assert hasattr(L, "sc_solve_device_multi") and hasattr(L, "sc_solve_host_multi")


class _FakeLib:
    """Records which solve entry point a Numeric.solve call reaches."""

    def __init__(self):
        self.calls = []

    def sc_solve_host(self, h, b, x):
        self.calls.append(("sc_solve_host",))
        return 0

    def sc_solve_host_multi(self, h, nrhs, B, ldb, X, ldx):
        self.calls.append(("sc_solve_host_multi", nrhs, ldb, ldx))
        return 0


class _Sym:
    n = 6


def test_solve_dispatches_on_argument_shape(monkeypatch):
    assert list(inspect.signature(sc.Numeric.solve).parameters) == ["self", "b"]
    assert list(inspect.signature(sc.Numeric.solve_device_multi).parameters) == [
        "self", "d_B_ptr", "nrhs", "ldb", "d_X_ptr", "ldx"]
    fake = _FakeLib()
    monkeypatch.setattr(sc, "lib", lambda: fake)
    num = object.__new__(sc.Numeric)  # no handle, no device: only the dispatch is under test
    num.symb, num.h = _Sym(), None
    x = num.solve(np.ones(6))
    assert x.shape == (6,) and fake.calls == [("sc_solve_host",)]
    X = num.solve(np.ones((6, 3)))  # C order in, (n, k) out
    assert X.shape == (6, 3) and fake.calls[-1] == ("sc_solve_host_multi", 3, 6, 6)
    X = num.solve(np.ones((6, 1), order="F"))
    assert X.shape == (6, 1) and fake.calls[-1] == ("sc_solve_host_multi", 1, 6, 6)
    with pytest.raises(ValueError):
        num.solve(np.ones((5, 2)))
