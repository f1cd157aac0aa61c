"""The C ABI of the gradient entry points: argument errors with the entry point's name, the
emulated handle, and the header's memory formula."""
import ctypes

import numpy as np
import pytest

import grad_cases as gc
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

SC_ERR_ARG, SC_ERR_NOTIMPL = -1, -7


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _setup():
    A = gc.matrix("bcsstk01")
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    n, nnz = A.size(), len(A.x)
    U = np.ones((n, 2), order="F")
    V = np.ones((n, 2), order="F")
    W = np.ones((n, 2), order="F")
    G = np.full(nnz, -7.0)
    return A, num, n, nnz, U, V, W, G


def _arg(rc, who, G=None):
    assert rc == SC_ERR_ARG
    assert who.encode() in sc.lib().sc_last_error(), sc.lib().sc_last_error()
    if G is not None:
        assert np.all(G == -7.0)


@pytest.mark.parametrize("form", ["host", "device"])
def test_pattern_outer_argument_errors(gpu, form):
    # every check comes before the first look at an array, so host arrays serve both forms
    A, num, n, nnz, U, V, W, G = _setup()
    f = getattr(sc.lib(), "sc_pattern_outer_" + form)
    who = "sc_pattern_outer_" + form
    _arg(f(None, 1.0, 2, _p(U), n, _p(V), n, 0.0, _p(G)), who)
    _arg(f(num.h, 1.0, -1, _p(U), n, _p(V), n, 0.0, _p(G)), who, G)
    _arg(f(num.h, 1.0, 2, None, n, _p(V), n, 0.0, _p(G)), who, G)
    _arg(f(num.h, 1.0, 2, _p(U), n, None, n, 0.0, _p(G)), who, G)
    _arg(f(num.h, 1.0, 2, _p(U), n, _p(V), n, 0.0, None), who)
    _arg(f(num.h, 1.0, 2, _p(U), n - 1, _p(V), n, 0.0, _p(G)), who, G)
    _arg(f(num.h, 1.0, 2, _p(U), n, _p(V), n - 1, 0.0, _p(G)), who, G)
    big = np.ones(max(nnz, 2 * n))
    _arg(f(num.h, 1.0, 2, _p(big), n, _p(V), n, 0.0, _p(big)), who)  # G is U
    _arg(f(num.h, 1.0, 2, _p(U), n, _p(big), n, 0.0, _p(big)), who)  # G is V


@pytest.mark.parametrize("form", ["host", "device"])
def test_pattern_dot_and_logdet_grad_argument_errors(gpu, form):
    A, num, n, nnz, U, V, W, G = _setup()
    L = sc.lib()
    out = ctypes.c_double(-7.0)
    f, who = getattr(L, "sc_pattern_dot_" + form), "sc_pattern_dot_" + form
    _arg(f(None, _p(G), _p(G), ctypes.byref(out)), who)
    _arg(f(num.h, None, _p(G), ctypes.byref(out)), who)
    _arg(f(num.h, _p(G), None, ctypes.byref(out)), who)
    _arg(f(num.h, _p(G), _p(G), None), who)
    assert out.value == -7.0
    f, who = getattr(L, "sc_logdet_grad_" + form), "sc_logdet_grad_" + form
    _arg(f(None, _p(G)), who)
    _arg(f(num.h, None), who)


@pytest.mark.parametrize("form", ["host", "device"])
def test_solve_grad_argument_errors(gpu, form):
    A, num, n, nnz, U, V, W, G = _setup()
    f, who = getattr(sc.lib(), "sc_solve_grad_" + form), "sc_solve_grad_" + form
    W[:] = -7.0
    _arg(f(None, 2, _p(U), n, _p(V), n, _p(W), n, _p(G)), who)
    _arg(f(num.h, -1, _p(U), n, _p(V), n, _p(W), n, _p(G)), who, G)
    _arg(f(num.h, 2, None, n, _p(V), n, _p(W), n, _p(G)), who, G)
    _arg(f(num.h, 2, _p(U), n, None, n, _p(W), n, _p(G)), who, G)
    _arg(f(num.h, 2, _p(U), n, _p(V), n, None, n, _p(G)), who, G)
    _arg(f(num.h, 2, _p(U), n, _p(V), n, _p(W), n, None), who)
    _arg(f(num.h, 2, _p(U), n - 1, _p(V), n, _p(W), n, _p(G)), who, G)
    _arg(f(num.h, 2, _p(U), n, _p(V), n - 1, _p(W), n, _p(G)), who, G)
    _arg(f(num.h, 2, _p(U), n, _p(V), n, _p(W), n - 1, _p(G)), who, G)
    big = np.ones(max(nnz, 2 * n))
    _arg(f(num.h, 2, _p(U), n, _p(big), n, _p(W), n, _p(big)), who)  # G is X (the outer product's V)
    _arg(f(num.h, 2, _p(U), n, _p(V), n, _p(big), n, _p(big)), who)  # G is Bbar (its U)
    assert np.all(W == -7.0)


def test_emulated_two_rank_handle_is_not_implemented(gpu):
    A = sc.laplacian3d(12)
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    n, nnz = A.size(), len(A.x)
    L = sc.lib()
    G = np.full(nnz, -7.0)
    X = np.ones((n, 1), order="F")
    Bbar = np.full((n, 1), -7.0, order="F")
    out = ctypes.c_double(-7.0)
    for rc, who in ((L.sc_logdet_grad_host(num.h, _p(G)), "sc_logdet_grad_host"),
                    (L.sc_pattern_outer_host(num.h, 1.0, 1, _p(X), n, _p(X), n, 0.0, _p(G)), "sc_pattern_outer_host"),
                    (L.sc_pattern_dot_host(num.h, _p(G), _p(G), ctypes.byref(out)), "sc_pattern_dot_host"),
                    (L.sc_solve_grad_host(num.h, 1, _p(X), n, _p(X), n, _p(Bbar), n, _p(G)), "sc_solve_grad_host")):
        assert rc == SC_ERR_NOTIMPL, who
    assert b"single-device" in L.sc_last_error()
    assert np.all(G == -7.0) and np.all(Bbar == -7.0) and out.value == -7.0
    with pytest.raises(sc.LibraryError):
        num.logdet_grad()


def _documented_bytes(symb):
    """The header's formula: 16 ne + 8 ni + 2 x 128 n + 8 (ceil(ne / 1024) + 1), each list at
    least one element."""
    _, _, eff = symb.value_entries()
    ne, ni = max(int(eff.sum()), 1), max(int((~eff).sum()), 1)
    return 16 * ne + 8 * ni + 2 * 128 * max(symb.n, 1) + 8 * ((ne + 1023) // 1024 + 1)


@pytest.mark.parametrize("name", ["six", "bcsstk01", "1138_bus"])
def test_memory_formula(gpu, name):
    A = gc.matrix(name)
    num = sc.Numeric(sc.Symbolic(A))
    n = A.size()
    m0 = num.memory()["total"]
    U = np.ones((n, 17))
    g = num.pattern_outer(U, U)  # the first of these calls allocates; the host form's staging is not kept
    grow = num.memory()["total"] - m0
    print(f"{name}: first call +{grow} bytes (formula {_documented_bytes(num.symb)})")
    assert grow == _documented_bytes(num.symb)
    num.pattern_dot(g, g)
    num.pattern_outer(U, U, alpha=-1.0, beta=1.0, G=g)
    assert num.memory()["total"] == m0 + grow
    # the factor-dependent entries add only what the selected inversion and the solves list
    assert num.factor(A.x) == 0
    num.solve(np.ones((n, 1)))
    assert num.selinv() == 0
    m1 = num.memory()["total"]
    num.logdet_grad()
    num.solve_grad(U, U)
    assert num.memory()["total"] == m1
