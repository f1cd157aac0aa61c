"""Products with A, residuals with backward errors and iterative refinement on the GPU.

The reference is exact: refine_cases.Exact evaluates products and residuals in rational
arithmetic and builds x_ref by refinement with exact residuals (~1e-70), from the raw input
arrays, independently of the library's own structure.  u = 2^-53.

Bounds.
  * Forward error of the refined solution with compensated residuals: |x - x_ref|_inf /
    |x_ref|_inf <= 4 u.  Refinement with a residual of precision u^2 converges to u + cond u^2,
    the last operation being one rounded x + d; the factor 4 is the margin.
  * Backward error: berr_comp <= 2 u with compensated residuals, <= (k_max + 2) u with fp64
    ones (k_max the longest row: the fp64 residual itself carries gamma_{k+2} (|b| + |A||x|)).
  * Products and residuals: the per-row bounds of test_spmv_kernels_gpu.py.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import sparsecholesky_amd as sc

import refine_cases as rc
import schur_cases

pytestmark = pytest.mark.gpu

U = rc.U
CONVERGED, STALLED, MAXITER, DIVERGED = range(4)


def _scaled_lap8():
    A = sc.laplacian3d(8, nd=False)
    d = 10.0 ** np.random.default_rng(21).uniform(-4, 4, A.size())
    cols = np.repeat(np.arange(A.size()), np.diff(A.p))
    return sc.csc_matrix(A.size(), A.size(), A.p, A.i, A.x * d[A.i] * d[cols])


# name -> (matrix, Symbolic keywords, right-hand sides)
CASES = {
    "bcsstk01_td0": lambda: (rc.load("bcsstk01"), dict(tiny_dense=0), 2),
    "bcsstk01_td1": lambda: (rc.load("bcsstk01"), dict(tiny_dense=1), 2),
    "bus_nat": lambda: (rc.load("1138_bus"), dict(ordering=0), 2),
    "bus_nd": lambda: (rc.load("1138_bus"), dict(ordering=1), 2),
    "bus_amd": lambda: (rc.load("1138_bus"), dict(ordering=2), 2),
    "lap8": lambda: (sc.laplacian3d(8, nd=False), {}, 2),
    "lap16": lambda: (sc.laplacian3d(16, nd=False), dict(ordering=1), 1),
    "lap8_schur": lambda: (sc.laplacian3d(8, nd=False), dict(schur=schur_cases.plane(8, 4)), 2),
    "dense100": lambda: (schur_cases.dense_spd(100), {}, 2),
    "lap8_scaled": lambda: (_scaled_lap8(), {}, 2),
}
# The inputs whose plain solve must miss the forward-error bar by at least 100 x.  1138_bus
# only: on bcsstk01 the GPU panel solve is better than that (measured 6.4e1 to 4.3e2 u against
# the 4e2 u the assertion needs, where the reference's algorithm on a CPU gave 6.6e2 u).
ILL = ("bus_nat", "bus_nd", "bus_amd")


@functools.lru_cache(maxsize=None)
def _input(case):
    A, kw, k = CASES[case]()
    key = "bus" if case.startswith("bus") else "bcsstk01" if case.startswith("bcsstk01") else case
    return A, kw, _shared(key, k)


@functools.lru_cache(maxsize=None)
def _matrix_of(key):
    return {"bus": "bus_nat", "bcsstk01": "bcsstk01_td0"}.get(key, key)


@functools.lru_cache(maxsize=None)
def _shared(key, k):
    """What depends on the matrix alone, computed once: exact operator, B, x_ref per column."""
    A = CASES[_matrix_of(key)]()[0]
    E = rc.Exact.of(A)
    B = np.random.default_rng(3).standard_normal((A.size(), k))
    B.setflags(write=False)
    xref = [E.solve(B[:, c]) for c in range(k)]
    res = max(float(max(abs(v) for v in E.residual(B[:, c], xref[c]))) for c in range(k))
    assert res < 1e-40, res
    return E, B, xref


def _fresh(case):
    A, kw, _ = _input(case)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x) == 0
    return num


@functools.lru_cache(maxsize=None)
def _numeric(case):
    return _fresh(case)


def _row_bounds(E):
    k = E.rowlen
    return [Fraction(rc.gamma(int(v) + 2)) for v in k], [Fraction(rc.gamma(2 * int(v) + 4)) ** 2 for v in k]


def _worst(err, bound):
    w = 0.0
    for e, b in zip(err, bound):
        if e != 0:
            assert b > 0
            w = max(w, float(e / b))
    return w


# ---- 1. product and residual ----
@pytest.mark.parametrize("case", list(CASES))
def test_product_and_residual_vs_exact(gpu, case):
    A, kw, (E, B, xref) = _input(case)
    num = _numeric(case)
    k = B.shape[1]
    g1, g2 = _row_bounds(E)
    rng = np.random.default_rng(8)
    # a solution perturbed in the third digit: the residual is far above its own rounding
    X = num.solve(np.asfortranarray(B)) * (1.0 + 1e-3 * rng.standard_normal(B.shape))
    Y = num.spmv(X)
    Yx = num.spmv(X, Ax=A.x)
    assert np.array_equal(rc.bits(Y), rc.bits(Yx))
    out = {m: num.residual(B, X, mode=m) for m in ("fp64", "dd")}
    w = dict(mul=0.0, fp64=0.0, dd=0.0)
    for c in range(k):
        y, r, s = E.mul(X[:, c]), E.residual(B[:, c], X[:, c]), E.denom(B[:, c], X[:, c])
        ax = E.mul(X[:, c], absolute=True)
        w["mul"] = max(w["mul"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(Y[:, c], y)],
                                        [g * a for g, a in zip(g1, ax)]))
        w["fp64"] = max(w["fp64"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(out["fp64"][0][:, c], r)],
                                          [g * a for g, a in zip(g1, s)]))
        w["dd"] = max(w["dd"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(out["dd"][0][:, c], r)],
                                      [Fraction(U) * abs(e) + g * a for e, g, a in zip(r, g2, s)]))
        bn, bc = E.berr(B[:, c], X[:, c])
        for m in ("fp64", "dd"):
            dn, dc = abs(out[m][1][c] - bn) / bn, abs(out[m][2][c] - bc) / bc
            print(f"REFINE {case} col {c} {m}: berr_norm {out[m][1][c]:.6e} (exact {bn:.6e}, rel {dn:.1e}), "
                  f"berr_comp {out[m][2][c]:.6e} (exact {bc:.6e}, rel {dc:.1e}); bar 1e-10")
            assert dn <= 1e-10 and dc <= 1e-10
    print(f"REFINE {case}: worst error / bound: product {w['mul']:.3f}, fp64 residual {w['fp64']:.3f}, "
          f"compensated {w['dd']:.3f} (each <= 1)")
    assert w["mul"] <= 1 and w["fp64"] <= 1 and w["dd"] <= 1
    # 1-D in, 1-D out
    y1 = num.spmv(X[:, 0])
    r1, bn1, bc1 = num.residual(B[:, 0], X[:, 0])
    assert y1.shape == (A.size(),) and np.array_equal(rc.bits(y1), rc.bits(Y[:, 0]))
    assert np.array_equal(rc.bits(r1), rc.bits(out["dd"][0][:, 0])) and bc1 == out["dd"][2][0]


# ---- 2. forward and backward error of the refined solution ----
@pytest.mark.parametrize("case", list(CASES))
def test_forward_error_compensated(gpu, case):
    A, kw, (E, B, xref) = _input(case)
    num = _numeric(case)
    X, info = num.solve_refined(B)
    X0 = num.solve(np.asfortranarray(B))
    for c in range(B.shape[1]):
        fe, fe0 = rc.ferr(X[:, c], xref[c]), rc.ferr(X0[:, c], xref[c])
        bn, bc = E.berr(B[:, c], X[:, c])
        print(f"REFINE {case} col {c}: forward error {fe / U:.3f} u (bar 4 u), plain solve {fe0 / U:.3e} u; "
              f"iters {info['iters'][c]} state {info['state'][c]}; berr_comp {info['berr_comp'][c] / U:.3f} u "
              f"(exact {bc / U:.3f} u, bar 2 u), berr_norm {info['berr_norm'][c]:.3e} (exact {bn:.3e}), "
              f"dx_ratio {info['dx_ratio'][c]:.3e}")
        assert fe <= 4 * U, (case, c, fe / U)
        assert info["state"][c] == CONVERGED and 1 <= info["iters"][c] <= 10
        assert info["berr_comp"][c] <= 2 * U
        assert abs(info["berr_comp"][c] - bc) <= 1e-10 * bc and abs(info["berr_norm"][c] - bn) <= 1e-10 * bn
        if case in ILL:
            # the plain solve of the same b misses the bar by at least 100 x: refinement is what meets it
            assert fe0 >= 100 * 4 * U, (case, c, fe0 / U)


@pytest.mark.parametrize("case", list(CASES))
def test_backward_error_fp64_residuals(gpu, case):
    A, kw, (E, B, xref) = _input(case)
    num = _numeric(case)
    X, info = num.solve_refined(B, residual="fp64")
    kmax = int(E.rowlen.max())
    for c in range(B.shape[1]):
        bn, bc = E.berr(B[:, c], X[:, c])
        print(f"REFINE {case} col {c} fp64: berr_comp {info['berr_comp'][c] / U:.3f} u (exact {bc / U:.3f} u, bar "
              f"{kmax + 2} u), iters {info['iters'][c]} state {info['state'][c]}, forward error "
              f"{rc.ferr(X[:, c], xref[c]) / U:.3e} u")
        assert info["berr_comp"][c] <= (kmax + 2) * U
        # the reported value comes from an fp64 residual: within that residual's own bound of the exact one
        assert abs(info["berr_comp"][c] - bc) <= 1.01 * rc.gamma(kmax + 2)


# ---- 3. the stopping rules ----
@pytest.mark.parametrize("case", ["bus_nd", "lap8", "bcsstk01_td1"])
def test_max_iter_zero_is_the_plain_solve(gpu, case):
    A, kw, (E, B, xref) = _input(case)
    num = _numeric(case)
    X0 = num.solve(np.asfortranarray(B))
    X, info = num.solve_refined(B, max_iter=0)
    assert np.array_equal(rc.bits(X), rc.bits(X0))
    assert np.all(info["iters"] == 0) and np.all(info["state"] == MAXITER)
    for c in range(B.shape[1]):
        bn, bc = E.berr(B[:, c], X0[:, c])
        assert abs(info["berr_comp"][c] - bc) <= 1e-10 * bc and abs(info["berr_norm"][c] - bn) <= 1e-10 * bn
    assert np.all(info["dx_ratio"] == 0.0)


def _representable_rhs(A, Ax2, k, seed):
    """B = A' X* for solutions X* with short mantissas (multiples of 1/8 below 128), so that
    B is exact in fp64 and the exact solution is itself a fixed point of x + d in fp64."""
    E2 = rc.Exact.of(A, Ax2)
    Xs = np.random.default_rng(seed).integers(-1000, 1001, (A.size(), k)) / 8.0
    B = np.zeros_like(Xs)
    for c in range(k):
        y = E2.mul(Xs[:, c])
        B[:, c] = [float(v) for v in y]
        assert all(Fraction(float(v)) == w for v, w in zip(B[:, c], y))
    return B, [[Fraction(float(v)) for v in Xs[:, c]] for c in range(k)]


def test_stale_factor_converging(gpu):
    """The factor of A as a preconditioner for 1.25 A: every step contracts by 1/4, so
    |d_k| = 1.25 * 4^-k |x| falls below u |x| at k = 27.

    The rule |d_k| <= u |x| sits on the rounding floor of x + d here: with a stale factor the
    next increment is 1.25 x the rounding error of the last update, which may exceed u |x| by
    that factor.  Whether a generic right-hand side ends CONVERGED or, at the same accuracy,
    STALLED is then decided by the mantissa of its largest entry (measured: STALLED after 28
    increments at 0.7 u).  The assertion on the state therefore uses solutions that fp64
    represents exactly, for which the last update lands on the solution and the next increment
    is zero; the generic right-hand sides are held to the same count and accuracy, in either of
    the two states."""
    A, kw, (E, Bg, xref) = _input("lap8")
    num = _numeric("lap8")
    Ax2 = 1.25 * A.x  # exact in fp64 (entries -1 and 6)
    B, x2 = _representable_rhs(A, Ax2, 2, 31)
    X0 = num.solve(np.asfortranarray(B))
    X, info = num.solve_refined(B, Ax=Ax2, max_iter=40)
    Xs, infos = num.solve_refined(B, Ax=Ax2)
    for c in range(B.shape[1]):
        fe, fe0, fes = rc.ferr(X[:, c], x2[c]), rc.ferr(X0[:, c], x2[c]), rc.ferr(Xs[:, c], x2[c])
        print(f"REFINE stale 1.25 A col {c}: {info['iters'][c]} increments (24..30), state {info['state'][c]}, forward "
              f"error {fe / U:.3f} u (bar 4 u); after 10: error ratio to the plain solve {fes / fe0:.3e} "
              f"(4^-11 = {4.0 ** -11:.3e} .. 4^-9 = {4.0 ** -9:.3e})")
        assert info["state"][c] == CONVERGED and 24 <= info["iters"][c] <= 30
        assert fe <= 4 * U
        assert infos["state"][c] == MAXITER and infos["iters"][c] == 10
        assert 4.0 ** -11 <= fes / fe0 <= 4.0 ** -9
    # generic right-hand sides: the same count and accuracy, CONVERGED or STALLED on the floor
    E2 = rc.Exact.of(A, Ax2)
    X, info = num.solve_refined(Bg, Ax=Ax2, max_iter=40)
    for c in range(Bg.shape[1]):
        fe = rc.ferr(X[:, c], E2.solve(Bg[:, c]))
        print(f"REFINE stale 1.25 A generic col {c}: {info['iters'][c]} increments, state {info['state'][c]}, forward "
              f"error {fe / U:.3f} u (bar 4 u)")
        assert info["state"][c] in (CONVERGED, STALLED) and 24 <= info["iters"][c] <= 30 and fe <= 4 * U


def test_stale_factor_diverging(gpu):
    A, kw, (E, B, xref) = _input("lap8")
    num = _numeric("lap8")
    X0 = num.solve(np.asfortranarray(B))
    X, info = num.solve_refined(B, Ax=3.0 * A.x)
    print(f"REFINE stale 3 A: state {info['state']} iters {info['iters']} dx_ratio {info['dx_ratio']}")
    assert np.all(info["state"] == DIVERGED) and np.all(info["iters"] == 0)
    assert np.array_equal(rc.bits(X), rc.bits(X0))
    assert np.all(np.abs(info["dx_ratio"] - 2.0) < 1e-6)  # every increment is -2 x_0


# ---- 4. columns are independent ----
def _same(a, b):
    Xa, ia = a
    Xb, ib = b
    return np.array_equal(rc.bits(Xa), rc.bits(Xb)) and all(
        np.array_equal(rc.bits(np.asarray(ia[f], dtype=np.float64)), rc.bits(np.asarray(ib[f], dtype=np.float64)))
        for f in ia)


@pytest.mark.parametrize("mode", ["dd", "fp64"])
def test_columns_do_not_depend_on_their_company(gpu, mode):
    A, kw, (E, B, xref) = _input("bus_nd")
    num = _numeric("bus_nd")
    P = np.zeros((A.size(), 3))
    P[:, 0], P[:, 1] = B[:, 0], 1e-8 * B[:, 0]
    X, info = num.solve_refined(P, residual=mode)
    print(f"REFINE independence {mode}: iters {info['iters']} states {info['state']} berr_comp {info['berr_comp']}")
    for c in range(3):
        xa, ia = num.solve_refined(P[:, c:c + 1].copy(), residual=mode)
        assert np.array_equal(rc.bits(xa[:, 0]), rc.bits(X[:, c])), c
        for f in info:
            assert np.array_equal(rc.bits(np.float64(ia[f][0])), rc.bits(np.float64(info[f][c]))), (c, f)
    # the zero column: exact zeros, zero backward errors, nothing to improve
    assert np.array_equal(rc.bits(X[:, 2]), rc.bits(np.zeros(A.size())))
    assert info["berr_comp"][2] == 0.0 and info["berr_norm"][2] == 0.0 and info["iters"][2] == 0
    assert info["state"][2] == CONVERGED
    # 17 columns = the calls of 16 and of 1
    W = np.random.default_rng(12).standard_normal((A.size(), 17)) * 10.0 ** np.arange(-8, 9)
    full = num.solve_refined(W, residual=mode)
    a, b = num.solve_refined(W[:, :16].copy(), residual=mode), num.solve_refined(W[:, 16:].copy(), residual=mode)
    assert np.array_equal(rc.bits(full[0][:, :16]), rc.bits(a[0])) and np.array_equal(rc.bits(full[0][:, 16:]), rc.bits(b[0]))
    for f in full[1]:
        assert np.array_equal(full[1][f], np.concatenate([a[1][f], b[1][f]]))
    # a repeat and a second handle: the same bits
    assert _same(full, num.solve_refined(W, residual=mode))
    assert _same(full, _fresh("bus_nd").solve_refined(W, residual=mode))


# ---- 5. nothing else changes ----
@pytest.mark.parametrize("case", ["bus_amd", "lap8_schur"])
def test_neighbours_unchanged(gpu, case):
    A, kw, (E, B, xref) = _input(case)
    num = _fresh(case)
    Bf = np.asfortranarray(B)

    def snapshot():
        st, L = num.export()
        return [num.solve(B[:, 0].copy()), num.solve(Bf), np.float64(num.logdet()), L.x.copy()]

    before = snapshot()
    num.solve_refined(B)
    num.solve_refined(B, residual="fp64", Ax=1.01 * A.x)
    num.residual(B, before[1])
    num.spmv(B)
    after = snapshot()
    for p, q in zip(before, after):
        assert np.array_equal(rc.bits(p), rc.bits(q))
