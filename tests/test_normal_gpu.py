"""Weighted normal equations end to end on the GPU: form, factor, compose, least squares.

Least-squares figures of the committed cases, measured on an MI355X by this file (max-norm error
against the exact rational solution; every case CONVERGED, in 1 to 3 increments):
    case             plain x_0    refined     cap (8 x numpy lstsq + 8 u)   |g| at x_0 -> refined
    consistent_1e1   4.2e-15      0           7.8e-14                       3.2e-16 -> 0
    random_1e1       7.6e-15      3.1e-16     9.6e-14                       2.5e-16 -> 6.8e-17
    consistent_1e3   8.0e-11      3.3e-36     7.6e-13                       1.4e-15 -> 1.3e-36
    random_1e3       1.1e-09      1.0e-14     2.7e-11                       1.1e-14 -> 1.2e-15
    consistent_1e5   3.1e-08      0           9.3e-11                       3.0e-15 -> 0
    random_1e5       5.1e-03      6.7e-12     1.7e-06                       8.7e-12 -> 3.0e-12
    damped_1e3       5.1e-14      7.6e-16     5.5e-13                       6.5e-16 -> 1.5e-16
    base_1e3         4.0e-16      4.5e-17     9.8e-15                       4.6e-16 -> 3.1e-17
The refined figures of the cases with a residual equal those of the host model
(normal_cases.emulate_lstsq(pair=True), which forms the gradient exactly) to the digits shown; on
the consistent cases both are zero or far below u (consistent_1e3: 3.3e-36 here, 2.0e-34 in the
model).  The gradient at x_0 is already near its floor u ||S|| ||x||, because the Cholesky
solve is backward stable for the normal equations themselves, so "grad_norm decreases from x_0"
is a factor of 3 to 10 on the cases with a residual (in the host model, whose x_0 differs in the
last bits, random_1e5 even goes 1.9e-12 -> 3.0e-12): the error is what the steps improve.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import normal_cases as nc

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


# ---- known answer ----
def test_grid_incidence_forms_the_laplacian_exactly_and_solves_bit_for_bit(gpu):
    k = 6
    J, _ = nc.grid_incidence(k)
    L = nc.grid_laplacian_plus_identity(k)
    ne_ = sc.NormalEquations(J)
    A = ne_.matrix()
    assert np.array_equal(A.p, L.p) and np.array_equal(A.i, L.i)
    S = ne_.values()
    assert np.array_equal(S, L.x)  # every term is +-1 or 1: the sums are exact in any order
    assert np.array_equal(ne_.values(w=np.ones(J.n_rows)), L.x)
    St = ne_.values_device(_dev(J.x))
    assert np.array_equal(St.cpu().numpy(), L.x)
    num = sc.Numeric(sc.Symbolic(A))
    assert ne_.values_ptr == 0  # device calls so far, but no factor call has filled the buffer
    assert ne_.factor(num) == 0
    assert ne_.values_ptr != 0
    ref = sc.Numeric(sc.Symbolic(L))
    assert ref.factor(L.x) == 0
    B = np.random.default_rng(1).standard_normal((k ** 3, 3))
    X, Xr = num.solve(B), ref.solve(B)
    assert X.tobytes() == Xr.tobytes()
    assert num.logdet() == ref.logdet()
    mem = ne_.memory()
    assert mem["device_bytes"] >= 12 * ne_.terms + 8 * len(L.x)


# ---- factor against a host-built S ----
@functools.lru_cache(maxsize=None)
def _weighted_problem():
    m, n = 40, 12
    rng = np.random.default_rng(7)
    J = nc.random_sparse(m, n, 0.3, 8)
    M = np.triu(rng.random((n, n)) < 0.3)
    base = nc.csc_of(np.where(M, 0.05 * rng.standard_normal((n, n)), 0.0), M, upper=True)
    w = rng.uniform(0.25, 4.0, m)
    d = rng.uniform(0.5, 1.0, n)
    lam = 0.125
    Jd, Cd = nc.dense_of(J), nc.dense_of(base)
    Sd = Cd + np.triu(Cd, 1).T + (Jd.T * w) @ Jd + np.diag(d + lam)
    return J, base, w, d, lam, Sd


def test_factor_matches_a_host_built_matrix(gpu):
    J, base, w, d, lam, Sd = _weighted_problem()
    n = J.n_cols
    ne_ = sc.NormalEquations(J, base)
    A = ne_.matrix()
    num = sc.Numeric(sc.Symbolic(A))
    assert ne_.factor(num, w=w, base_values=base.x, d=d, damping=lam) == 0
    host = sc.Numeric(sc.Symbolic(A))
    Sx = np.array([Sd[A.i[e], j] for j in range(n) for e in range(int(A.p[j]), int(A.p[j + 1]))])
    assert host.factor(Sx) == 0
    tp = ne_.term_lists()[0]
    g = nc.gamma(int(np.max(np.diff(tp))) + 3)
    kappa = np.linalg.cond(Sd)
    dl = abs(num.logdet() - host.logdet())
    B = np.random.default_rng(9).standard_normal((n, 2))
    X, Xh = num.solve(B), host.solve(B)
    ds = np.max(np.abs(X - Xh)) / np.max(np.abs(Xh))
    print(f"cond {kappa:.2e}, gamma {g:.2e}: |dlogdet| {dl:.3e} (bound {4 * n * kappa * g:.3e}), "
          f"solve difference {ds:.3e} (bound {4 * kappa * g:.3e})")
    assert dl <= 4 * n * kappa * g
    assert ds <= 4 * kappa * g
    # the values themselves, device forms included
    Sv = ne_.values(w=w, base_values=base.x, d=d, damping=lam)
    St = ne_.values_device(_dev(J.x), _dev(w), _dev(base.x), _dev(d), lam)
    assert np.array_equal(St.cpu().numpy(), Sv)
    num2 = sc.Numeric(sc.Symbolic(A))
    assert ne_.factor_device(num2, _dev(J.x), _dev(w), _dev(base.x), _dev(d), lam) == 0
    assert num2.solve(B).tobytes() == X.tobytes()


# ---- reweighting: a stale factor as the preconditioner of the new values ----
def test_reweighted_values_compose_with_pcg_and_residual(gpu):
    J, base, w0, d, lam, _ = _weighted_problem()
    n, m = J.n_cols, J.n_rows
    ne_ = sc.NormalEquations(J, base)
    num = sc.Numeric(sc.Symbolic(ne_.matrix()))
    assert ne_.factor(num, w=w0, base_values=base.x, d=d, damping=lam) == 0
    rng = np.random.default_rng(11)
    B = rng.standard_normal((n, 3))
    # values_ptr with an existing entry point: the residual of the handle's own solve
    dB = _dev(B.T)
    dX, dR = torch.zeros_like(dB), torch.zeros_like(dB)
    assert num.solve_device_multi(dB.data_ptr(), 3, n, dX.data_ptr(), n) == 0
    bn, bc = num.residual_device_multi(ne_.values_ptr, dB.data_ptr(), 3, n, dX.data_ptr(), n, dR.data_ptr(), n)
    assert np.all(bn < 1e-14)
    # new weights, formed on the device, solved with the stale factor
    w1 = w0 * rng.uniform(0.5, 2.0, m)
    S1 = ne_.values_device(_dev(J.x), _dev(w1), _dev(base.x), _dev(d), lam)
    dX1 = torch.zeros_like(dB)
    info = num.solve_pcg_device_multi(S1.data_ptr(), dB.data_ptr(), 3, n, dX1.data_ptr(), n, tol=1e-12)
    assert np.all(info["state"] == sc.SC_PCG_CONVERGED) and np.all(info["iters"] >= 1)
    Jd, Cd = nc.dense_of(J), nc.dense_of(base)
    S1d = Cd + np.triu(Cd, 1).T + (Jd.T * w1) @ Jd + np.diag(d + lam)
    want = np.linalg.solve(S1d, B)
    got = dX1.cpu().numpy().T
    assert np.max(np.abs(got - want)) <= 1e-10 * np.max(np.abs(want))
    # the buffer of the last factor call is still the w0 matrix
    assert ne_.values_ptr != S1.data_ptr()


# ---- least squares ----
@functools.lru_cache(maxsize=None)
def _lsq(name):
    c = nc.lstsq_case(name)
    J = nc.csc_of(c["J"], np.ones(c["J"].shape, dtype=bool))
    base = None if c["C"] is None else nc.csc_of(c["C"], np.triu(c["C"] != 0), upper=True)
    ne_ = sc.NormalEquations(J, base)
    num = sc.Numeric(sc.Symbolic(ne_.matrix()))
    st = ne_.factor(num, w=c["w"], base_values=None if base is None else base.x, d=c["d"], damping=c["lam"])
    assert st == 0
    xe = nc.lstsq_exact(c)
    X, info = ne_.lstsq(num, c["b"], w=c["w"])
    X0, info0 = ne_.lstsq(num, c["b"], w=c["w"], max_iter=0)
    return c, ne_, num, xe, X, info, X0, info0


@pytest.mark.parametrize("name", sorted(nc.LSQ_CASES))
def test_lstsq_meets_the_cap_and_converges(gpu, name):
    c, ne_, num, xe, X, info, X0, info0 = _lsq(name)
    cap = nc.lstsq_cap(c, xe)
    err, err0 = nc.max_error(X, xe), nc.max_error(X0, xe)
    print(f"{name}: error {err:.3e} (cap {cap:.3e}), plain {err0:.3e}, state {info['state']}, iters {info['iters']}, "
          f"|g| {info0['grad_norm']:.3e} -> {info['grad_norm']:.3e}, resid {info['resid_norm']:.3e}, "
          f"dx_ratio {info['dx_ratio']:.3e}")
    assert err <= cap
    assert info["state"] == sc.SC_REFINE_CONVERGED and 1 <= info["iters"] <= 10
    # max_iter = 0: the plain normal-equations solve, as the host emulation computes it
    assert info0["state"] == sc.SC_REFINE_MAXITER and info0["iters"] == 0
    xp, _ = nc.emulate_lstsq(c["J"], c["w"], c["b"], c["C"], c["d"], c["lam"], max_iter=0)
    assert np.max(np.abs(X0 - xp)) <= 4.0 * nc.max_error(xp, xe)
    # the reported norms describe the returned X
    r = c["b"] - c["J"] @ X
    assert abs(info["resid_norm"] - np.sqrt(np.sum(c["w"] * r * r))) <= 1e-10 * max(1.0, np.linalg.norm(c["b"]))
    assert info["dx_ratio"] <= 2.0 ** -52 or info["grad_norm"] == 0.0  # the two ways to CONVERGED


@pytest.mark.parametrize("name", sorted(nc.LSQ_CASES))
def test_grad_norm_decreases_from_x0(gpu, name):
    _, _, _, _, _, info, _, info0 = _lsq(name)
    print(f"{name}: |g| {info0['grad_norm']:.3e} -> {info['grad_norm']:.3e}")
    assert info["grad_norm"] < info0["grad_norm"]


def test_refinement_gains_three_digits_at_kappa_1e5(gpu):
    _, _, _, xe, X, _, X0, _ = _lsq("consistent_1e5")
    err, err0 = nc.max_error(X, xe), nc.max_error(X0, xe)
    print(f"consistent_1e5: plain {err0:.3e}, refined {err:.3e}")
    assert err * 1e3 <= err0


def test_lstsq_columns_travel_independently_and_device_form_agrees(gpu):
    c, ne_, num, *_ = _lsq("random_1e3")
    rng = np.random.default_rng(13)
    B = np.column_stack([c["b"], rng.standard_normal((nc.LSQ_M, 17))])  # two panels
    X, info = ne_.lstsq(num, B, w=c["w"])
    x1, i1 = ne_.lstsq(num, B[:, 0], w=c["w"])
    assert np.array_equal(X[:, 0], x1) and info["iters"][0] == i1["iters"]
    sub = [3, 16, 17]
    Xs, _ = ne_.lstsq(num, B[:, sub], w=c["w"])
    assert np.array_equal(Xs, X[:, sub])
    Xd, infod = ne_.lstsq_device(num, _dev(B), _dev(ne_.J.x), _dev(c["w"]))
    assert np.array_equal(Xd.cpu().numpy(), X) and np.array_equal(infod["state"], info["state"])
    Xf, infof = ne_.lstsq(num, B[:, :2], w=c["w"], residual="fp64")
    assert np.all(np.isfinite(Xf)) and np.max(np.abs(Xf - X[:, :2])) <= 1e-6 * np.max(np.abs(X[:, :2]))


# ---- failure and misuse ----
def _zero_column_problem():
    J0 = nc.random_sparse(15, 6, 0.6, 17)
    D = nc.dense_of(J0)
    D[:, 3] = 0.0
    return nc.csc_of(D, D != 0)


@pytest.mark.parametrize("ordering", [0, 1])
def test_zero_column_fails_at_that_column_and_damping_cures_it(gpu, ordering):
    J = _zero_column_problem()
    ne_ = sc.NormalEquations(J)
    symb = sc.Symbolic(ne_.matrix(), ordering=ordering)
    num = sc.Numeric(symb)
    b = np.random.default_rng(19).standard_normal(J.n_rows)
    with pytest.raises(sc.LibraryError, match="call out of order"):
        ne_.lstsq(num, b)  # before any factorization
    st = ne_.factor(num)
    where = int(np.flatnonzero(symb.perm() == 3)[0])
    assert st == where + 1
    # a failed factorization: its status, nothing written
    L = sc.lib()
    X = np.full(J.n_cols, 7.0)
    o = sc.Numeric._refine_options(10, "dd", 0.5)
    rc = L.sc_normal_lstsq_host_multi(ne_.h, num.h, ctypes.byref(o), 1, J.x.ctypes.data_as(vp), None,
                                      b.ctypes.data_as(vp), J.n_rows, X.ctypes.data_as(vp), J.n_cols, None)
    assert rc == st and np.all(X == 7.0)
    assert ne_.factor(num, damping=0.5) == 0
    x, info = ne_.lstsq(num, b)
    assert info["state"] == sc.SC_REFINE_CONVERGED
    Jd = nc.dense_of(J)
    want = np.linalg.solve(Jd.T @ Jd + 0.5 * np.eye(J.n_cols), Jd.T @ b)
    assert np.max(np.abs(x - want)) <= 1e-12 * np.max(np.abs(want))


def test_misuse_is_rejected_with_messages(gpu):
    J, base, w, d, lam, _ = _weighted_problem()
    ne_ = sc.NormalEquations(J, base)
    num = sc.Numeric(sc.Symbolic(ne_.matrix()))
    assert ne_.factor(num, w=w, base_values=base.x, d=d, damping=lam) == 0
    L = sc.lib()
    m, n = J.n_rows, J.n_cols
    o = sc.Numeric._refine_options(10, "dd", 0.5)
    buf = np.zeros(max(m, n))
    jx = J.x.ctypes.data_as(vp)
    # X == B
    rc = L.sc_normal_lstsq_host_multi(ne_.h, num.h, ctypes.byref(o), 1, jx, None, buf.ctypes.data_as(vp), m,
                                      buf.ctypes.data_as(vp), n, None)
    assert rc == -1 and L.sc_last_error().decode().startswith("sc_normal_lstsq_host_multi: X aliases B")
    # a numeric handle of another analysis
    other = sc.Numeric(sc.Symbolic(sc.laplacian3d(3)))
    with pytest.raises(sc.LibraryError, match="sc_normal_factor_host: the numeric handle's analysis"):
        ne_.factor(other, w=w)
    # a factor that did not come from this handle
    S = ne_.values(w=w, base_values=base.x, d=d, damping=lam)
    assert num.factor(S) == 0
    with pytest.raises(sc.LibraryError, match="was not made by the last sc_normal_factor"):
        ne_.lstsq(num, np.zeros(m), w=w)
    # two numeric handles factored through one sc_normal: the handle remembers the last call's values
    # and base only, so the earlier factor is refused instead of being refined against the wrong base
    assert ne_.factor(num, w=w, base_values=base.x, d=d, damping=lam) == 0
    x_first, _ = ne_.lstsq(num, np.ones(m), w=w)
    second = sc.Numeric(sc.Symbolic(ne_.matrix()))
    assert ne_.factor(second, w=w, base_values=base.x, d=d, damping=4.0 * lam) == 0
    with pytest.raises(sc.LibraryError, match="was not made by the last sc_normal_factor"):
        ne_.lstsq(num, np.ones(m), w=w)
    x_second, _ = ne_.lstsq(second, np.ones(m), w=w)
    assert not np.array_equal(x_first, x_second)
    # before any factorization: SC_ERR_STATE with a message of its own, whatever failed earlier
    fresh = sc.Numeric(sc.Symbolic(ne_.matrix()))
    with pytest.raises(sc.LibraryError, match="sc_normal_lstsq_host_multi: the numeric handle holds no factorization"):
        ne_.lstsq(fresh, np.ones(m), w=w)
    # emulated ranks
    emu = sc.Numeric(sc.Symbolic(ne_.matrix()), nranks=2, virtual=True)
    with pytest.raises(sc.LibraryError, match="not implemented"):
        ne_.factor(emu, w=w)
    # bad options
    o.rho_max = 1.5
    X = np.zeros(n)
    rc = L.sc_normal_lstsq_host_multi(ne_.h, num.h, ctypes.byref(o), 1, jx, None, buf.ctypes.data_as(vp), m,
                                      X.ctypes.data_as(vp), n, None)
    assert rc == -1 and "rho_max" in L.sc_last_error().decode()
