"""The factor operators (sc_apply_*, sc_logdet) at the C-ABI and Python boundary; no
device needed."""
import ctypes

import numpy as np
import pytest

import sparsecholesky_amd as sc

ENTRY = ["sc_apply_device", "sc_apply_host", "sc_apply_device_multi", "sc_apply_host_multi", "sc_logdet"]


def test_null_handle_is_an_argument_error():
    L = sc.lib()
    calls = {
        "sc_apply_device": lambda: L.sc_apply_device(None, sc.SC_OP_SOLVE_L, None, None),
        "sc_apply_host": lambda: L.sc_apply_host(None, sc.SC_OP_MUL_L, None, None),
        "sc_apply_device_multi": lambda: L.sc_apply_device_multi(None, sc.SC_OP_MUL_LT, 1, None, 0, None, 0),
        "sc_apply_host_multi": lambda: L.sc_apply_host_multi(None, sc.SC_OP_SOLVE_LT, 1, None, 0, None, 0),
        "sc_logdet": lambda: L.sc_logdet(None, None),
    }
    assert sorted(calls) == sorted(ENTRY)
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.sc_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)


def test_python_table_binds_the_symbols():
    names = sc.exported_symbols()
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in names, name
        assert hasattr(so, name), name


def test_op_constants_are_the_header_enum():
    import os
    import re

    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparsecholesky.h")
    enum = dict((k, int(v)) for k, v in re.findall(r"\b(SC_OP_[A-Z_]+)\s*=\s*(\d+)", open(hdr).read()))
    assert len(enum) == 7
    for k, v in enum.items():
        assert getattr(sc, k) == v, k
        assert k in sc.__all__


class _FakeLib:
    """Records which entry point a Numeric.apply call reaches, and with which op."""

    def __init__(self):
        self.calls = []

    def sc_apply_host(self, h, op, b, x):
        self.calls.append(("sc_apply_host", op))
        return 0

    def sc_apply_host_multi(self, h, op, nrhs, B, ldb, X, ldx):
        self.calls.append(("sc_apply_host_multi", op, nrhs, ldb, ldx))
        return 0

    def sc_logdet(self, h, out):
        self.calls.append(("sc_logdet",))
        return 0


class _Sym:
    n = 6


def _fake_numeric(monkeypatch):
    fake = _FakeLib()
    monkeypatch.setattr(sc, "lib", lambda: fake)
    num = object.__new__(sc.Numeric)  # no handle, no device: only the dispatch is under test
    num.symb, num.h = _Sym(), None
    return num, fake


def test_apply_dispatches_on_argument_shape(monkeypatch):
    num, fake = _fake_numeric(monkeypatch)
    x = num.apply(np.ones(6), sc.SC_OP_SOLVE_L)
    assert x.shape == (6,) and fake.calls == [("sc_apply_host", sc.SC_OP_SOLVE_L)]
    X = num.apply(np.ones((6, 3)), sc.SC_OP_MUL_LT)  # C order in, (n, k) out
    assert X.shape == (6, 3) and fake.calls[-1] == ("sc_apply_host_multi", sc.SC_OP_MUL_LT, 3, 6, 6)
    X = num.apply(np.ones((6, 1), order="F"), sc.SC_OP_PERM)
    assert X.shape == (6, 1) and fake.calls[-1] == ("sc_apply_host_multi", sc.SC_OP_PERM, 1, 6, 6)
    assert num.logdet() == 0.0 and fake.calls[-1] == ("sc_logdet",)


def test_wrappers_pass_their_op(monkeypatch):
    num, fake = _fake_numeric(monkeypatch)
    for meth, op in [("solve_L", sc.SC_OP_SOLVE_L), ("solve_Lt", sc.SC_OP_SOLVE_LT), ("mul_L", sc.SC_OP_MUL_L),
                     ("mul_Lt", sc.SC_OP_MUL_LT), ("apply_P", sc.SC_OP_PERM), ("apply_Pt", sc.SC_OP_PERM_T)]:
        getattr(num, meth)(np.ones(6))
        assert fake.calls[-1] == ("sc_apply_host", op), meth
        getattr(num, meth)(np.ones((6, 2)))
        assert fake.calls[-1] == ("sc_apply_host_multi", op, 2, 6, 6), meth


def test_row_count_mismatch_raises(monkeypatch):
    num, fake = _fake_numeric(monkeypatch)
    with pytest.raises(ValueError):
        num.apply(np.ones((5, 2)), sc.SC_OP_MUL_L)
    with pytest.raises(ValueError):
        num.apply(np.ones(7), sc.SC_OP_MUL_L)
    assert fake.calls == []
