"""Products, residuals and refinement at the C-ABI boundary: argument and state rules with
their sc_last_error texts, the NULL-values rule, a failed factorization, an emulated
handle, the documented device memory, and in-place calls (rejected: refinement needs B
after X exists)."""
import ctypes

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import refine_cases as rc

pytestmark = pytest.mark.gpu

SC_ERR_ARG, SC_ERR_STATE, SC_ERR_NOTIMPL = -1, -5, -7
VP = ctypes.c_void_p
ENTRY = ["sc_default_refine_options", "sc_spmv_structure", "sc_spmv_host_multi", "sc_spmv_device_multi",
         "sc_residual_host_multi", "sc_residual_device_multi", "sc_solve_refine_host_multi",
         "sc_solve_refine_device_multi", "sc_debug_spmv"]


def _p(a):
    return a.ctypes.data_as(VP)


def _handle(factor=True, **kw):
    A = sc.laplacian3d(4, nd=False)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    if factor:
        assert num.factor(A.x) == 0
    return A, num


def _opts(**kw):
    o = sc.RefineOptions()
    sc.lib().sc_default_refine_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_symbols_defaults_and_bindings(gpu):
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in sc.exported_symbols() and hasattr(so, name), name
    for meth in ("spmv", "residual", "solve_refined", "spmv_device_multi", "residual_device_multi",
                 "solve_refined_device_multi"):
        assert callable(getattr(sc.Numeric, meth))
    assert callable(sc.Symbolic.spmv_structure)
    o = _opts()
    assert (o.struct_size, o.max_iter, o.residual, o.rho_max) == (ctypes.sizeof(sc.RefineOptions), 10, 1, 0.5)
    assert ctypes.sizeof(sc.RefineOptions) == 24 and ctypes.sizeof(sc.RefineInfo) == 32


def test_argument_rules(gpu):
    A, num = _handle()
    L = sc.lib()
    n = A.size()
    B, X = np.ones((n, 2), order="F"), np.zeros((n, 2), order="F")
    keep = X.copy()
    ax = _p(A.x)

    def refine(h=num.h, opt=None, nrhs=2, b=B, ldb=n, x=X, ldx=n):
        return L.sc_solve_refine_host_multi(h, opt, nrhs, ax, None if b is None else _p(b), ldb,
                                            None if x is None else _p(x), ldx, None)

    def residual(h=num.h, mode=1, nrhs=2, b=B, ldb=n, x=B, ldx=n, r=X, ldr=n):
        return L.sc_residual_host_multi(h, mode, nrhs, ax, None if b is None else _p(b), ldb,
                                        None if x is None else _p(x), ldx, None if r is None else _p(r), ldr, None, None)

    def spmv(h=num.h, nrhs=2, x=B, ldx=n, y=X, ldy=n):
        return L.sc_spmv_host_multi(h, nrhs, ax, None if x is None else _p(x), ldx, None if y is None else _p(y), ldy)

    bad = [
        (lambda: refine(h=None), b"sc_solve_refine_host_multi: null handle"),
        (lambda: refine(nrhs=-1), b"sc_solve_refine_host_multi: nrhs < 0"),
        (lambda: refine(b=None), b"sc_solve_refine_host_multi: null B"),
        (lambda: refine(x=None), b"sc_solve_refine_host_multi: null X"),
        (lambda: refine(ldb=n - 1), b"sc_solve_refine_host_multi: leading dimension of B below n"),
        (lambda: refine(ldx=n - 1), b"sc_solve_refine_host_multi: leading dimension of X below n"),
        (lambda: refine(opt=ctypes.byref(_opts(struct_size=16))), b"sc_solve_refine_host_multi: sc_refine_options.struct_size"),
        (lambda: refine(opt=ctypes.byref(_opts(max_iter=-1))), b"sc_solve_refine_host_multi: max_iter < 0"),
        (lambda: refine(opt=ctypes.byref(_opts(rho_max=0.0))), b"sc_solve_refine_host_multi: rho_max outside (0, 1)"),
        (lambda: refine(opt=ctypes.byref(_opts(rho_max=1.0))), b"sc_solve_refine_host_multi: rho_max outside (0, 1)"),
        (lambda: refine(opt=ctypes.byref(_opts(rho_max=float("nan")))), b"sc_solve_refine_host_multi: rho_max outside"),
        (lambda: refine(opt=ctypes.byref(_opts(residual=2))), b"sc_solve_refine_host_multi: residual is neither"),
        (lambda: refine(x=B), b"sc_solve_refine_host_multi: X aliases B"),  # in place: rejected
        (lambda: residual(h=None), b"sc_residual_host_multi: null handle"),
        (lambda: residual(mode=5), b"sc_residual_host_multi: residual is neither"),
        (lambda: residual(r=None), b"sc_residual_host_multi: null R"),
        (lambda: residual(ldr=3), b"sc_residual_host_multi: leading dimension of R below n"),
        (lambda: residual(r=B), b"sc_residual_host_multi: R aliases B or X"),
        (lambda: spmv(h=None), b"sc_spmv_host_multi: null handle"),
        (lambda: spmv(nrhs=-2), b"sc_spmv_host_multi: nrhs < 0"),
        (lambda: spmv(x=None), b"sc_spmv_host_multi: null X"),
        (lambda: spmv(ldy=0), b"sc_spmv_host_multi: leading dimension of Y below n"),
        (lambda: spmv(y=B), b"sc_spmv_host_multi: Y aliases X"),
    ]
    for call, text in bad:
        assert call() == SC_ERR_ARG, text
        assert text in L.sc_last_error(), (text, L.sc_last_error())
    assert np.array_equal(X, keep)
    # nrhs == 0: nothing to do, null arrays are fine
    assert refine(nrhs=0, b=None, x=None) == 0 and residual(nrhs=0, b=None, x=None, r=None) == 0
    assert spmv(nrhs=0, x=None, y=None) == 0
    # the device forms name themselves
    assert L.sc_solve_refine_device_multi(num.h, None, 1, None, None, n, None, n, None) == SC_ERR_ARG
    assert b"sc_solve_refine_device_multi: null B" in L.sc_last_error()
    assert L.sc_residual_device_multi(None, 1, 1, None, None, n, None, n, None, n, None, None) == SC_ERR_ARG
    assert b"sc_residual_device_multi: null handle" in L.sc_last_error()
    assert L.sc_spmv_device_multi(None, 1, None, None, n, None, n) == SC_ERR_ARG
    assert b"sc_spmv_device_multi: null handle" in L.sc_last_error()


def test_state_rules_and_null_values(gpu):
    A, num = _handle(factor=False)
    L = sc.lib()
    n = A.size()
    B, X = np.ones((n, 1), order="F"), np.full((n, 1), 7.0, order="F")
    # before a factorization: refinement is out of order; product and residual work with explicit values
    assert L.sc_solve_refine_host_multi(num.h, None, 1, _p(A.x), _p(B), n, _p(X), n, None) == SC_ERR_STATE
    assert np.all(X == 7.0)
    Y = num.spmv(B, Ax=A.x)
    E = rc.Exact.of(A)
    assert np.array_equal(Y[:, 0], [float(v) for v in E.mul(B[:, 0])])  # small integers: exact in fp64
    R, bn, bc = num.residual(Y, B, Ax=A.x)
    assert np.all(R == 0.0) and np.all(bn == 0.0) and np.all(bc == 0.0)
    # NULL values before any sc_factor: no copy to stand for
    assert L.sc_spmv_host_multi(num.h, 1, None, _p(B), n, _p(X), n) == SC_ERR_ARG
    assert b"sc_spmv_host_multi: null values stand for the copy sc_factor made" in L.sc_last_error()
    # after sc_factor: NULL is that copy
    assert num.factor(A.x) == 0
    assert np.array_equal(num.spmv(B), Y)
    X1, info = num.solve_refined(B)
    assert info["state"][0] == 0
    # after sc_factor_device: the library holds only the caller's pointer, NULL is an error
    d_Ax = torch.tensor(2.0 * A.x, device="cuda")
    assert num.factor_device(d_Ax.data_ptr()) == 0
    for call, name in ((lambda: L.sc_spmv_host_multi(num.h, 1, None, _p(B), n, _p(X), n), b"sc_spmv_host_multi"),
                       (lambda: L.sc_residual_host_multi(num.h, 1, 1, None, _p(B), n, _p(Y), n, _p(X), n, None, None),
                        b"sc_residual_host_multi"),
                       (lambda: L.sc_solve_refine_host_multi(num.h, None, 1, None, _p(B), n, _p(X), n, None),
                        b"sc_solve_refine_host_multi")):
        assert call() == SC_ERR_ARG
        assert name + b": null values stand for the copy sc_factor made" in L.sc_last_error()
    # explicit device values work, and describe 2 A
    dB, dX = torch.tensor(B.T.copy(), device="cuda"), torch.zeros((1, n), dtype=torch.float64, device="cuda")
    info = num.solve_refined_device_multi(d_Ax.data_ptr(), dB.data_ptr(), 1, n, dX.data_ptr(), n)
    assert info["state"][0] == 0
    assert np.allclose(dX.cpu().numpy()[0], 0.5 * X1[:, 0], rtol=1e-12)
    dY = torch.zeros((1, n), dtype=torch.float64, device="cuda")
    assert num.spmv_device_multi(d_Ax.data_ptr(), dB.data_ptr(), 1, n, dY.data_ptr(), n) == 0
    assert np.array_equal(dY.cpu().numpy()[0], 2.0 * Y[:, 0])
    bn, bc = num.residual_device_multi(d_Ax.data_ptr(), dY.data_ptr(), 1, n, dB.data_ptr(), n, dX.data_ptr(), n)
    assert bn[0] == 0.0 and bc[0] == 0.0 and np.all(dX.cpu().numpy() == 0.0)


def test_failed_factorization_writes_nothing(gpu):
    A = sc.laplacian3d(4, nd=False)
    x = A.x.copy()
    x[A.find_index(5, 5)] = -1.0
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(x)
    assert st > 0
    n = A.size()
    B, X = np.ones((n, 2), order="F"), np.full((n, 2), 7.0, order="F")
    info = (sc.RefineInfo * 2)()
    info[0].iters = info[1].iters = -9
    assert sc.lib().sc_solve_refine_host_multi(num.h, None, 2, None, _p(B), n, _p(X), n, info) == st
    assert np.all(X == 7.0) and info[0].iters == -9 and info[1].iters == -9
    # the product does not look at the factor
    assert np.all(np.isfinite(num.spmv(B)))


def test_emulated_handle_is_not_implemented(gpu):
    A = sc.laplacian3d(4, nd=False)
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    n = A.size()
    B, X = np.ones((n, 1), order="F"), np.full((n, 1), 7.0, order="F")
    L = sc.lib()
    for call, name in ((lambda: L.sc_solve_refine_host_multi(num.h, None, 1, None, _p(B), n, _p(X), n, None),
                        b"sc_solve_refine_host_multi"),
                       (lambda: L.sc_spmv_host_multi(num.h, 1, _p(A.x), _p(B), n, _p(X), n), b"sc_spmv_host_multi"),
                       (lambda: L.sc_residual_host_multi(num.h, 1, 1, _p(A.x), _p(B), n, _p(B), n, _p(X), n, None, None),
                        b"sc_residual_host_multi")):
        assert call() == SC_ERR_NOTIMPL
        assert name in L.sc_last_error() and b"single-device" in L.sc_last_error()
    assert np.all(X == 7.0)


def _documented_bytes(symb):
    """The header's formula (sparsecholesky.h, 'Device memory')."""
    rp, ci, _ = symb.spmv_structure()
    n, nz = symb.n, len(ci)
    ln = np.diff(rp)
    chunks = -(-ln // 256)
    ntask = int(np.maximum(chunks, 1).sum())
    nlong = int((ln > 256).sum())
    nslots = int(chunks[ln > 256].sum())
    groups = -(-ntask // 256) + -(-nlong // 16)
    return (8 * (n + 1) + 12 * max(nz, 1) + 16 * ntask + 8 * max(nlong, 1) + 512 * max(nslots, 1)
            + 640 * max(groups, 1) + 2 * 128 * max(n, 1) + 8960)


@pytest.mark.parametrize("which", ["lap6", "arrow"])
def test_memory_grows_once_by_the_documented_amount(gpu, which):
    if which == "lap6":
        A = sc.laplacian3d(6, nd=False)
    else:  # one row of 600 entries: three chunks
        n = 600
        i = np.concatenate([np.arange(n), np.zeros(n - 1, dtype=np.int64)]).astype(np.int32)
        j = np.concatenate([np.arange(n), np.arange(1, n)]).astype(np.int32)
        A = sc.triplet_to_csc_matrix(i, j, np.concatenate([np.full(n, 2.0 * n), np.ones(n - 1)]), n)
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    B = np.random.default_rng(0).standard_normal((A.size(), 3))
    num.solve(np.asfortranarray(B))  # what the first panel solve allocates is not this feature's
    m0 = num.memory()["total"]
    X, info = num.solve_refined(B)
    m1 = num.memory()["total"]
    num.solve_refined(B, residual="fp64")
    num.residual(B, X)
    num.spmv(B)
    m2 = num.memory()["total"]
    want = _documented_bytes(num.symb)
    print(f"REFINE memory {which}: first call +{m1 - m0} bytes (documented {want}), later calls +{m2 - m1}")
    assert m1 - m0 == want and m2 == m1
    assert np.all(info["state"] == 0)
