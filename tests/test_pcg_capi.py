"""Conjugate gradients at the C-ABI boundary: symbols and defaults, argument and state rules with
their sc_last_error texts, the NULL-values rule, a failed factorization, an emulated handle,
and the documented device memory."""
import ctypes

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

SC_ERR_ARG, SC_ERR_STATE, SC_ERR_NOTIMPL = -1, -5, -7
VP = ctypes.c_void_p
ENTRY = ["sc_default_pcg_options", "sc_solve_pcg_host_multi", "sc_solve_pcg_device_multi", "sc_debug_pcg_vec"]


def _p(a):
    return a.ctypes.data_as(VP)


def _handle(factor=True, **kw):
    A = sc.laplacian3d(4, nd=False)
    num = sc.Numeric(sc.Symbolic(A), **kw)
    if factor:
        assert num.factor(A.x) == 0
    return A, num


def _opts(**kw):
    o = sc.PcgOptions()
    sc.lib().sc_default_pcg_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_symbols_defaults_and_bindings(gpu):
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in sc.exported_symbols() and hasattr(so, name), name
    for meth in ("solve_pcg", "solve_pcg_device_multi"):
        assert callable(getattr(sc.Numeric, meth))
    o = _opts()
    assert (o.struct_size, o.max_iter, o.use_x0, o.tol) == (ctypes.sizeof(sc.PcgOptions), 100, 0, 1e-10)
    assert ctypes.sizeof(sc.PcgOptions) == 24 and ctypes.sizeof(sc.PcgInfo) == 40
    assert (sc.SC_PCG_CONVERGED, sc.SC_PCG_MAXITER, sc.SC_PCG_BREAKDOWN) == (0, 1, 2)
    assert sc.lib().sc_version() == 121


def test_argument_rules(gpu):
    A, num = _handle()
    L = sc.lib()
    n = A.size()
    B, X = np.ones((n, 2), order="F"), np.zeros((n, 2), order="F")
    keep = X.copy()
    ax = _p(A.x)

    def pcg(h=num.h, opt=None, nrhs=2, b=B, ldb=n, x=X, ldx=n):
        return L.sc_solve_pcg_host_multi(h, opt, nrhs, ax, None if b is None else _p(b), ldb,
                                         None if x is None else _p(x), ldx, None)

    who = b"sc_solve_pcg_host_multi: "
    bad = [
        (lambda: pcg(h=None), b"null handle"),
        (lambda: pcg(nrhs=-1), b"nrhs < 0"),
        (lambda: pcg(b=None), b"null B"),
        (lambda: pcg(x=None), b"null X"),
        (lambda: pcg(ldb=n - 1), b"leading dimension of B below n"),
        (lambda: pcg(ldx=n - 1), b"leading dimension of X below n"),
        (lambda: pcg(opt=ctypes.byref(_opts(struct_size=16))), b"sc_pcg_options.struct_size"),
        (lambda: pcg(opt=ctypes.byref(_opts(max_iter=-1))), b"max_iter < 0"),
        (lambda: pcg(opt=ctypes.byref(_opts(tol=-1e-3))), b"tol outside [0, 1)"),
        (lambda: pcg(opt=ctypes.byref(_opts(tol=1.0))), b"tol outside [0, 1)"),
        (lambda: pcg(opt=ctypes.byref(_opts(tol=float("nan")))), b"tol outside [0, 1)"),
        (lambda: pcg(opt=ctypes.byref(_opts(use_x0=2))), b"use_x0 is neither 0 nor 1"),
        (lambda: pcg(opt=ctypes.byref(_opts(use_x0=-1))), b"use_x0 is neither 0 nor 1"),
        (lambda: pcg(x=B), b"X aliases B"),
    ]
    for call, text in bad:
        assert call() == SC_ERR_ARG, text
        assert who + text in L.sc_last_error(), (text, L.sc_last_error())
    assert np.array_equal(X, keep)
    # nrhs == 0: nothing to do, null arrays are fine; tol = 0 is legal and runs to max_iter
    assert pcg(nrhs=0, b=None, x=None) == 0
    info = (sc.PcgInfo * 2)()
    assert L.sc_solve_pcg_host_multi(num.h, ctypes.byref(_opts(tol=0.0, max_iter=2)), 2, _p(3.0 * A.x), _p(B), n, _p(X),
                                     n, info) == 0
    assert all(i.state in (sc.SC_PCG_MAXITER, sc.SC_PCG_BREAKDOWN) and i.iters <= 2 for i in info)
    # the device form names itself
    assert L.sc_solve_pcg_device_multi(num.h, None, 1, None, None, n, None, n, None) == SC_ERR_ARG
    assert b"sc_solve_pcg_device_multi: null B" in L.sc_last_error()


def test_state_rules_and_null_values(gpu):
    A, num = _handle(factor=False)
    L = sc.lib()
    n = A.size()
    B, X = np.ones((n, 1), order="F"), np.full((n, 1), 7.0, order="F")
    assert L.sc_solve_pcg_host_multi(num.h, None, 1, _p(A.x), _p(B), n, _p(X), n, None) == SC_ERR_STATE
    assert np.all(X == 7.0)
    # after sc_factor: NULL is the copy it made
    assert num.factor(A.x) == 0
    X1, info = num.solve_pcg(B)
    assert info["state"][0] == 0 and info["iters"][0] == 0
    # after sc_factor_device: the library holds only the caller's pointer, NULL is an error
    d_Ax = torch.tensor(2.0 * A.x, device="cuda")
    assert num.factor_device(d_Ax.data_ptr()) == 0
    assert L.sc_solve_pcg_host_multi(num.h, None, 1, None, _p(B), n, _p(X), n, None) == SC_ERR_ARG
    assert b"sc_solve_pcg_host_multi: null values stand for the copy sc_factor made" in L.sc_last_error()
    # explicit device values work: the factor is of 2 A, the values say 6 A
    d6 = 3.0 * d_Ax
    dB, dX = torch.tensor(B.T.copy(), device="cuda"), torch.zeros((1, n), dtype=torch.float64, device="cuda")
    info = num.solve_pcg_device_multi(d6.data_ptr(), dB.data_ptr(), 1, n, dX.data_ptr(), n)
    assert info["state"][0] == 0 and 1 <= info["iters"][0] <= 2
    assert np.allclose(dX.cpu().numpy()[0], X1[:, 0] / 6.0, rtol=1e-9)
    # a warm start from that solution: nothing to do, X untouched
    keep = dX.clone()
    info = num.solve_pcg_device_multi(d6.data_ptr(), dB.data_ptr(), 1, n, dX.data_ptr(), n, use_x0=True)
    assert info["iters"][0] == 0 and torch.equal(dX, keep)


def test_failed_factorization_writes_nothing(gpu):
    A = sc.laplacian3d(4, nd=False)
    x = A.x.copy()
    x[A.find_index(5, 5)] = -1.0
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(x)
    assert st > 0
    n = A.size()
    B, X = np.ones((n, 2), order="F"), np.full((n, 2), 7.0, order="F")
    info = (sc.PcgInfo * 2)()
    info[0].iters = info[1].iters = -9
    assert sc.lib().sc_solve_pcg_host_multi(num.h, None, 2, None, _p(B), n, _p(X), n, info) == st
    assert np.all(X == 7.0) and info[0].iters == -9 and info[1].iters == -9


def test_emulated_handle_is_not_implemented(gpu):
    A, num = _handle(nranks=2, virtual=True)
    n = A.size()
    B, X = np.ones((n, 1), order="F"), np.full((n, 1), 7.0, order="F")
    L = sc.lib()
    assert L.sc_solve_pcg_host_multi(num.h, None, 1, None, _p(B), n, _p(X), n, None) == SC_ERR_NOTIMPL
    assert b"sc_solve_pcg_host_multi" in L.sc_last_error() and b"single-device" in L.sc_last_error()
    assert np.all(X == 7.0)


def _documented_bytes(n):
    """The header's formula (sparsecholesky.h, the conjugate gradients' 'Device memory')."""
    return 3 * 128 * max(n, 1) + 256 * max(-(-n // 1024), 1) + 512


@pytest.mark.parametrize("k", [6, 11])  # n = 216: one group of partials; n = 1331: two
def test_memory_grows_once_by_the_documented_amount(gpu, k):
    A = sc.laplacian3d(k, nd=False)
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    B = np.random.default_rng(0).standard_normal((A.size(), 3))
    num.solve_refined(B)  # the panel solve's and the refinement section's memory are not this feature's
    m0 = num.memory()["total"]
    X, info = num.solve_pcg(B, Ax=3.0 * A.x)
    m1 = num.memory()["total"]
    num.solve_pcg(B, Ax=pc_values(A), tol=1e-12)
    num.solve_pcg(np.random.default_rng(1).standard_normal((A.size(), 20)), Ax=3.0 * A.x, x0=np.zeros((A.size(), 20)))
    m2 = num.memory()["total"]
    want = _documented_bytes(A.size())
    print(f"PCG memory lap{k}: first call +{m1 - m0} bytes (documented {want}), later calls +{m2 - m1}")
    assert m1 - m0 == want and m2 == m1
    assert np.all(info["state"] == 0)
    # and a handle whose first such call is this one allocates the refinement section's share too
    fresh = sc.Numeric(sc.Symbolic(A))
    assert fresh.factor(A.x) == 0
    fresh.solve(np.asfortranarray(B))
    f0 = fresh.memory()["total"]
    fresh.solve_pcg(B, Ax=3.0 * A.x)
    assert fresh.memory()["total"] - f0 == (m1 - m0) + (m0 - _before_refine(A, B))


def pc_values(A):
    x = np.array(A.x)
    x[A.find_index(3, 3)] *= 4.0
    return x


def _before_refine(A, B):
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    num.solve(np.asfortranarray(B))
    return num.memory()["total"]
