"""The eigensolver at the C-ABI boundary: symbols and defaults, argument and state rules with their
sc_last_error texts, the NULL-values rule, a failed factorization, an emulated handle, and the
documented device memory (first call, later calls, a call that asks for more blocks)."""
import ctypes

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

SC_ERR_ARG, SC_ERR_STATE, SC_ERR_NOTIMPL = -1, -5, -7
VP = ctypes.c_void_p
ENTRY = ["sc_default_eigs_options", "sc_eigs_host", "sc_eigs_device", "sc_debug_eigs_gram", "sc_debug_eigs_update",
         "sc_debug_eigs_dense"]


def _p(a):
    return None if a is None else a.ctypes.data_as(VP)


def _handle(factor=True, **kw):
    A = sc.laplacian3d(4, nd=False)
    num = sc.Numeric(sc.Symbolic(A), **kw)
    if factor:
        assert num.factor(A.x) == 0
    return A, num


def _opts(**kw):
    o = sc.EigsOptions()
    sc.lib().sc_default_eigs_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_symbols_defaults_and_bindings(gpu):
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in sc.exported_symbols() and hasattr(so, name), name
    for meth in ("eigsh", "eigsh_device"):
        assert callable(getattr(sc.Numeric, meth))
    o = _opts()
    assert (o.struct_size, o.max_blocks, o.use_x0, o.seed, o.tol, o.sigma) == (ctypes.sizeof(sc.EigsOptions), 32, 0, 1,
                                                                                1e-10, 0.0)
    assert sc.lib().sc_version() == 121


def test_argument_rules(gpu):
    A, num = _handle()
    L = sc.lib()
    n = A.size()
    X, lam, X0 = np.full((n, 3), 7.0, order="F"), np.full(3, 7.0), np.ones((n, 16), order="F")
    info = (sc.EigsInfo * 3)()
    info[0].blocks = info[2].blocks = -9
    ax = _p(A.x)

    def eigs(h=num.h, opt=None, nev=3, x0=None, ldx0=n, l=lam, x=X, ldx=n):
        return L.sc_eigs_host(h, opt, nev, ax, _p(x0), ldx0, _p(l), _p(x), ldx, info)

    R = ctypes.byref
    who = b"sc_eigs_host: "
    bad = [
        (lambda: eigs(h=None), b"null handle"),
        (lambda: eigs(l=None), b"null lambda"),
        (lambda: eigs(x=None), b"null X"),
        (lambda: eigs(opt=R(_opts(use_x0=1))), b"null X0"),
        (lambda: eigs(nev=-1), b"nev < 0"),
        (lambda: eigs(nev=n + 1), b"nev > min(n, 16 max_blocks)"),
        (lambda: eigs(nev=33, opt=R(_opts(max_blocks=2))), b"nev > min(n, 16 max_blocks)"),
        (lambda: eigs(ldx=n - 1), b"leading dimension of X below n"),
        (lambda: eigs(opt=R(_opts(use_x0=1)), x0=X0, ldx0=n - 1), b"leading dimension of X0 below n"),
        (lambda: eigs(opt=R(_opts(struct_size=32))), b"sc_eigs_options.struct_size"),
        (lambda: eigs(opt=R(_opts(max_blocks=0))), b"max_blocks outside 1..32"),
        (lambda: eigs(opt=R(_opts(max_blocks=33))), b"max_blocks outside 1..32"),
        (lambda: eigs(opt=R(_opts(tol=-1e-3))), b"tol outside [0, 1)"),
        (lambda: eigs(opt=R(_opts(tol=1.0))), b"tol outside [0, 1)"),
        (lambda: eigs(opt=R(_opts(tol=float("nan")))), b"tol outside [0, 1)"),
        (lambda: eigs(opt=R(_opts(use_x0=2))), b"use_x0 is neither 0 nor 1"),
        (lambda: eigs(opt=R(_opts(use_x0=-1))), b"use_x0 is neither 0 nor 1"),
        (lambda: eigs(opt=R(_opts(sigma=float("inf")))), b"sigma is not finite"),
        (lambda: eigs(opt=R(_opts(sigma=float("nan")))), b"sigma is not finite"),
    ]
    for call, text in bad:
        assert call() == SC_ERR_ARG, text
        assert who + text in L.sc_last_error(), (text, L.sc_last_error())
    assert np.all(X == 7.0) and np.all(lam == 7.0) and info[0].blocks == -9 and info[2].blocks == -9
    # nev == 0: nothing to do, null arrays are fine, nothing touched
    assert eigs(nev=0, l=None, x=None) == 0
    assert info[0].blocks == -9
    # ldx0 is not looked at without use_x0; a leading dimension above n is honoured and the padding kept
    Xp = np.full((n + 2, 3), 7.0, order="F")
    assert eigs(x=Xp, ldx=n + 2, ldx0=0) == 0
    assert np.all(Xp[n:] == 7.0) and np.allclose(np.linalg.norm(Xp[:n], axis=0), 1.0, rtol=1e-12)
    assert info[0].state == sc.SC_EIGS_CONVERGED and info[0].blocks >= 1
    X0p = np.full((n + 1, 16), np.nan, order="F")
    X0p[:n] = np.random.default_rng(0).uniform(-1, 1, (n, 16))
    assert eigs(opt=R(_opts(use_x0=1)), x0=X0p, ldx0=n + 1) == 0 and np.all(np.isfinite(X))
    # the device form names itself
    assert L.sc_eigs_device(num.h, None, 1, None, None, n, _p(lam), None, n, None) == SC_ERR_ARG
    assert b"sc_eigs_device: null X" in L.sc_last_error()


def test_state_rules_and_null_values(gpu):
    A, num = _handle(factor=False)
    L = sc.lib()
    n = A.size()
    X, lam = np.full((n, 2), 7.0, order="F"), np.full(2, 7.0)
    assert L.sc_eigs_host(num.h, None, 2, _p(A.x), None, n, _p(lam), _p(X), n, None) == SC_ERR_STATE
    assert np.all(X == 7.0) and np.all(lam == 7.0)
    # after sc_factor: NULL is the copy it made
    assert num.factor(A.x) == 0
    l1, X1, info = num.eigsh(2, return_info=True)
    assert np.all(info["state"] == 0)
    # after sc_factor_device: the library holds only the caller's pointer, NULL is an error
    d_Ax = torch.tensor(2.0 * A.x, device="cuda")
    assert num.factor_device(d_Ax.data_ptr()) == 0
    assert L.sc_eigs_host(num.h, None, 2, None, None, n, _p(lam), _p(X), n, None) == SC_ERR_ARG
    assert b"sc_eigs_host: null values stand for the copy sc_factor made" in L.sc_last_error()
    assert np.all(X == 7.0) and np.all(lam == 7.0)
    # explicit device values work: the factor is of 2 A
    l2, X2, info2 = num.eigsh_device(2, values=d_Ax, return_info=True)
    assert np.all(info2["state"] == 0) and np.allclose(l2, 2.0 * l1, rtol=1e-9)


def test_failed_factorization_writes_nothing(gpu):
    A = sc.laplacian3d(4, nd=False)
    x = A.x.copy()
    x[A.find_index(5, 5)] = -1.0
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(x)
    assert st > 0
    n = A.size()
    X, lam = np.full((n, 2), 7.0, order="F"), np.full(2, 7.0)
    info = (sc.EigsInfo * 2)()
    info[0].blocks = info[1].blocks = -9
    assert sc.lib().sc_eigs_host(num.h, None, 2, None, None, n, _p(lam), _p(X), n, info) == st
    assert np.all(X == 7.0) and np.all(lam == 7.0) and info[0].blocks == -9 and info[1].blocks == -9


def test_emulated_handle_is_not_implemented(gpu):
    A, num = _handle(nranks=2, virtual=True)
    n = A.size()
    X, lam = np.full((n, 1), 7.0, order="F"), np.full(1, 7.0)
    L = sc.lib()
    assert L.sc_eigs_host(num.h, None, 1, None, None, n, _p(lam), _p(X), n, None) == SC_ERR_NOTIMPL
    assert b"sc_eigs_host" in L.sc_last_error() and b"single-device" in L.sc_last_error()
    assert np.all(X == 7.0) and np.all(lam == 7.0)


def _documented_bytes(n, mb):
    """The header's formula (sparsecholesky.h, the eigensolver's 'Device memory')."""
    n1 = max(n, 1)
    return (mb + 1) * 128 * n1 + 2048 * mb * max(-(-n // 1024), 1) + 4096 * mb + 128 * n1


@pytest.mark.parametrize("k", [6, 11])  # n = 216: one group of partials; n = 1331: two
def test_memory_grows_by_the_documented_amount(gpu, k):
    A = sc.laplacian3d(k, nd=False)
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    B = np.random.default_rng(0).standard_normal((n, 3))
    num.solve_refined(B)  # the panel solve's and the refinement section's memory are not this feature's
    m0 = num.memory()["total"]
    lam, X, info = num.eigsh(3, max_blocks=8, return_info=True)
    m1 = num.memory()["total"]
    num.eigsh(6, max_blocks=8, seed=3)
    num.eigsh(2, max_blocks=5, X0=np.random.default_rng(1).uniform(-1, 1, (n, 16)))
    m2 = num.memory()["total"]
    num.eigsh(3, max_blocks=12)  # more blocks: the basis, the partials and the coefficients are replaced
    m3 = num.memory()["total"]
    num.eigsh(3, max_blocks=8)
    m4 = num.memory()["total"]
    print(f"eigs memory lap{k}: first call +{m1 - m0} bytes (documented {_documented_bytes(n, 8)}), later calls "
          f"+{m2 - m1}, 12 blocks +{m3 - m2} (documented {_documented_bytes(n, 12) - _documented_bytes(n, 8)})")
    assert m1 - m0 == _documented_bytes(n, 8) and m2 == m1
    assert m3 - m0 == _documented_bytes(n, 12) and m4 == m3
    assert np.all(info["blocks"] <= 8) and np.all(np.isfinite(lam))
