"""Selected inversion (sc_selinv*) at the C-ABI and Python boundary.  Only the last test
needs a device."""
import ctypes

import numpy as np
import pytest

import sparsecholesky_amd as sc
from test_solve_multi import _matrix  # the inputs and their cache, shared

ENTRY = ["sc_selinv", "sc_selinv_diag_host", "sc_selinv_diag_device", "sc_selinv_export", "sc_selinv_flops"]


def test_symbols_are_exported_and_bound():
    names = sc.exported_symbols()
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in names, name
        assert hasattr(so, name), name
    for meth in ("selinv", "inverse_diagonal", "selected_inverse", "inverse_diagonal_device"):
        assert callable(getattr(sc.Numeric, meth))
    assert callable(sc.Symbolic.selinv_flops)


def test_null_arguments_are_argument_errors():
    L = sc.lib()
    buf = np.zeros(4)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    calls = {
        "sc_selinv": lambda: L.sc_selinv(None),
        "sc_selinv_diag_host": lambda: L.sc_selinv_diag_host(None, p),
        "sc_selinv_diag_device": lambda: L.sc_selinv_diag_device(None, p),
        "sc_selinv_export": lambda: L.sc_selinv_export(None, None, None, p),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = L.sc_last_error()
        assert name.encode() in msg and b"null handle" in msg, (name, msg)
    assert np.all(buf == 0.0)
    v = ctypes.c_double(-1.0)
    assert L.sc_selinv_flops(None, ctypes.byref(v)) == -1
    assert b"sc_selinv_flops" in L.sc_last_error() and v.value == -1.0
    s = sc.Symbolic(_matrix("bcsstk01"))
    assert L.sc_selinv_flops(s.h, None) == -1
    assert b"null flops" in L.sc_last_error()


def _flops_by_the_documented_formula(symb):
    """Per supernode (m front rows, w pivots) and block k0 = 0, 128, .. < w, with
    nb = min(128, w - k0), nr = m - k0 - nb:  2 nr nb^2 + 2 nr^2 nb + nb (nb + 1) (nb + nr)."""
    sn = symb.supernodes()
    tot = 0
    for m, w in zip(sn["m"].tolist(), sn["w"].tolist()):
        for k0 in range(0, w, 128):
            nb = min(128, w - k0)
            nr = m - k0 - nb
            tot += 2 * nr * nb * nb + 2 * nr * nr * nb + nb * (nb + 1) * (nb + nr)
    return tot


@pytest.mark.parametrize("name,kw", [("bcsstk01", {}), ("1138_bus", {}), ("1138_bus", dict(ordering=1)), ("lap16", {})],
                         ids=["bcsstk01", "1138_bus", "1138_bus_nd", "lap16"])
def test_flops_equal_the_documented_formula(name, kw):
    s = sc.Symbolic(_matrix(name), **kw)
    want = _flops_by_the_documented_formula(s)
    assert 0 < want < 2 ** 53  # every partial sum is an integer a double holds exactly
    assert s.selinv_flops() == float(want)


@pytest.mark.gpu
def test_device_diagonal_equals_host_diagonal(gpu):
    import torch

    A = _matrix("1138_bus")
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A, ordering=1))
    assert num.factor(A.x) == 0
    L = sc.lib()
    assert L.sc_selinv_diag_host(num.h, None) == -1 and b"null d" in L.sc_last_error()
    assert L.sc_selinv_diag_device(num.h, None) == -1 and b"null d_d" in L.sc_last_error()
    d_dev = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    assert L.sc_selinv_diag_device(num.h, ctypes.c_void_p(d_dev.data_ptr())) == 0  # computes first
    host = np.zeros(n)
    assert L.sc_selinv_diag_host(num.h, host.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(d_dev.cpu().numpy(), host)
    assert num.inverse_diagonal_device(d_dev.data_ptr()) == 0
    assert np.array_equal(d_dev.cpu().numpy(), num.inverse_diagonal())
