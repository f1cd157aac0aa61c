"""Conjugate gradients preconditioned with the factor (Numeric.solve_pcg) on the GPU.

References: pcg_cases.emulate, the numpy model of the documented algorithm (pinned by
test_pcg_cases_cpu.py), for iteration counts and residual histories; refine_cases.Exact for
an exact-rational x_ref.  Values are per call, so "A'" below is always the whole panel's.

Bounds.
  * k eigenvalues of inv(A) A' away from 1: at most k + 1 steps in exact arithmetic, k + 2
    allowed (rank 3: 5; A' = 3 A: 2).
  * relres_true <= 2 tol: the recurrence's residual is at most tol at the stop, and its gap
    to the true one is below 1e-15 |b| on the inputs of that check (the model's own gap).
  * forward error <= cond_2(A') relres_true in 2-norms: |x - x*| = |inv(A') r| <= |inv(A')| |r|
    and |b| <= |A'| |x*|.
  * Everything about company, position, repetition and a second handle is bitwise.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

import sparsecholesky_amd as sc

import pcg_cases as pc
import refine_cases as rc
from refine_cases import bits

pytestmark = pytest.mark.gpu

INPUTS = ("bcsstk01", "lap8", "lap8_nd", "bus_nd", "lap4_schur")
RANK3_INPUTS = ("bcsstk01", "lap8", "lap8_nd", "bus_nd")
DIVERGED = 3  # SC_REFINE_DIVERGED


@functools.lru_cache(maxsize=None)
def _numeric(name):
    A, kw = pc.matrix(name)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x) == 0
    return num


def _fresh(name):
    A, kw = pc.matrix(name)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x) == 0
    return num


@functools.lru_cache(maxsize=None)
def _dense(name):
    M = pc.dense(pc.matrix(name)[0])
    M.setflags(write=False)
    return M


@functools.lru_cache(maxsize=None)
def _B(name, k=17):
    return pc.rhs(pc.matrix(name)[0].size(), k)


def _model(name, Ax, c, **kw):
    A = pc.matrix(name)[0]
    return pc.emulate(pc.dense(A, Ax), _dense(name), _B(name)[:, c], **kw)


# ---- 1. the factored values: the panel solve, bit for bit ----
@pytest.mark.parametrize("name", INPUTS)
def test_factored_values_return_the_panel_solve(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)
    for k in (1, 16, 17):
        Bk = np.asfortranarray(B[:, :k])
        X, info = num.solve_pcg(Bk)
        Xe, infoe = num.solve_pcg(Bk, Ax=A.x)
        print(f"PCG {name} factored values k {k}: relres {info['relres'].max():.2e}, "
              f"true {info['relres_true'].max():.2e}")
        assert not info["iters"].any() and np.all(info["state"] == pc.CONVERGED)
        assert np.array_equal(bits(X), bits(num.solve(Bk))) and np.array_equal(bits(X), bits(Xe))
        assert np.all(info["relres"] <= 1e-10) and np.array_equal(info["relres"], info["relres_true"])
    x, i1 = num.solve_pcg(B[:, 0])  # 1-D in, 1-D and scalars out
    assert x.shape == (A.size(),) and i1["iters"] == 0 and np.array_equal(bits(x), bits(X[:, 0]))


# ---- 2. A' = 3 A: one eigenvalue, where refinement diverges ----
@pytest.mark.parametrize("name", INPUTS)
def test_three_a(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)[:, :2]
    X, info = num.solve_pcg(B, Ax=3.0 * A.x, tol=1e-10)
    _, rinfo = num.solve_refined(B, Ax=3.0 * A.x)
    print(f"PCG {name} 3 A: iters {info['iters']}, relres {info['relres']}, true {info['relres_true']}; "
          f"refinement states {rinfo['state']}")
    assert np.all(rinfo["state"] == DIVERGED)
    assert np.all(info["state"] == pc.CONVERGED) and np.all((1 <= info["iters"]) & (info["iters"] <= 2))
    assert np.all(info["relres_true"] <= 2e-10)


# ---- 3. three diagonal entries changed ----
@pytest.mark.parametrize("name", RANK3_INPUTS)
def test_rank3(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)[:, :2]
    Ax = pc.values_rank3(A)
    X, info = num.solve_pcg(B, Ax=Ax, tol=1e-12)
    for c in range(2):
        e = _model(name, Ax, c, tol=1e-12)
        print(f"PCG {name} rank 3 col {c}: iters {info['iters'][c]} (model {e['iters']}, bar 5), relres "
              f"{info['relres'][c]:.2e} (model {e['relres']:.2e}), true {info['relres_true'][c]:.2e}")
        assert info["state"][c] == pc.CONVERGED and info["relres"][c] <= 1e-12
        assert info["iters"][c] <= 5 and info["iters"][c] <= e["iters"] + 1


# ---- 4. D A D with 10 % on lap 8^3 ----
@pytest.mark.parametrize("name", ["lap8", "lap8_nd"])
def test_scaled_ten_percent(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)[:, :2]
    Ax = pc.values_dad(A, 0.1)
    tol = 1e-10
    X, info = num.solve_pcg(B, Ax=Ax, tol=tol)
    E = rc.Exact.of(A, Ax)
    kappa = np.linalg.cond(E.dense())
    for c in range(2):
        e = _model(name, Ax, c, tol=tol)
        assert abs(e["relres"] - e["relres_true"]) < 1e-15
        xref = E.solve(B[:, c])
        err = np.array([float(Fraction(float(a)) - b) for a, b in zip(X[:, c], xref)])
        ferr = np.linalg.norm(err) / np.linalg.norm([float(v) for v in xref])
        print(f"PCG {name} DAD 0.1 col {c}: iters {info['iters'][c]} (model {e['iters']}), "
              f"relres {info['relres'][c]:.2e}, true {info['relres_true'][c]:.2e}, forward {ferr:.2e} "
              f"(bar {kappa * info['relres_true'][c]:.2e})")
        assert info["state"][c] == pc.CONVERGED and abs(int(info["iters"][c]) - e["iters"]) <= 2
        assert info["relres_true"][c] <= 2 * tol
        assert ferr <= kappa * info["relres_true"][c]
        # the closing pass is an fp64 residual: |r_fl - r| <= gamma_{k+2} (|b| + |A'| |x|) per row (k
        # the longest row), which moves either backward error by at most that gamma
        bn, bc = E.berr(B[:, c], X[:, c])
        slack = rc.gamma(int(E.rowlen.max()) + 2)
        assert abs(info["berr_norm"][c] - bn) <= slack + 1e-10 * bn
        assert abs(info["berr_comp"][c] - bc) <= slack + 1e-10 * bc


# ---- 5. the ill-conditioned end: a MAXITER case ----
def test_bus_scaled_stops_at_max_iter(gpu):
    name = "bus_nd"
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)[:, :2]
    Ax = pc.values_dad(A, 0.1)
    X, info = num.solve_pcg(B, Ax=Ax, tol=1e-10, max_iter=5)
    for c in range(2):
        e = _model(name, Ax, c, tol=1e-10, max_iter=5)
        gap = abs(info["relres"][c] - e["relres"]) / e["relres"]
        print(f"PCG {name} DAD 0.1 col {c}: relres after 5 steps {info['relres'][c]:.6e}, model {e['relres']:.6e}, "
              f"relative gap {gap:.2e} (bar 1e-6)")
        assert (info["iters"][c], info["state"][c]) == (5, pc.MAXITER) and e["state"] == pc.MAXITER
        assert gap <= 1e-6


# ---- 6. values that are not positive definite ----
@pytest.mark.parametrize("name", INPUTS)
def test_minus_a_breaks_down(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], np.asfortranarray(_B(name)[:, :3])
    X, info = num.solve_pcg(B, Ax=-A.x)
    assert np.all(info["state"] == pc.BREAKDOWN) and not info["iters"].any()
    assert np.array_equal(bits(X), bits(num.solve(B)))
    assert np.allclose(info["relres"], 2.0) and np.allclose(info["relres_true"], 2.0)


def test_negative_diagonal_is_never_converged(gpu):
    num, A, B = _numeric("lap8"), pc.matrix("lap8")[0], _B("lap8")[:, :4]
    X, info = num.solve_pcg(B, Ax=pc.values_diag(A, 100, -1e3))
    print(f"PCG lap8 diagonal -1e3: states {info['state']}, iters {info['iters']}, true {info['relres_true']}")
    assert np.all((info["state"] == pc.BREAKDOWN) | (info["state"] == pc.MAXITER))
    assert np.all(np.isfinite(info["relres_true"])) and np.all(np.isfinite(X))


# ---- 7. a warm start ----
def test_warm_start(gpu):
    num, A, B = _numeric("lap8"), pc.matrix("lap8")[0], _B("lap8")[:, :2]
    Ax = pc.values_rank3(A)
    E = rc.Exact.of(A, Ax)
    X0 = np.asfortranarray(np.array([[float(v) for v in E.solve(B[:, c])] for c in range(2)]).T)
    X, info = num.solve_pcg(B, Ax=Ax, x0=X0)
    assert not info["iters"].any() and np.all(info["state"] == pc.CONVERGED)
    assert np.array_equal(bits(X), bits(X0)) and np.all(info["relres_true"] < 1e-14)
    _, cold = num.solve_pcg(B, Ax=Ax)
    Xz, zero = num.solve_pcg(B, Ax=Ax, x0=np.zeros_like(B))
    print(f"PCG lap8 rank 3: cold start {cold['iters']} steps, from zero {zero['iters']}")
    assert np.all(zero["state"] == pc.CONVERGED) and np.all(np.abs(cold["iters"] - zero["iters"]) <= 1)
    assert np.allclose(Xz, X0, rtol=1e-8)


# ---- 8. independence of company and position, repeatability ----
def _same(a, b):
    return all(np.array_equal(bits(a[1][f]), bits(b[1][f])) for f in a[1]) and np.array_equal(bits(a[0]), bits(b[0]))


@pytest.mark.parametrize("name", ["lap8_nd", "bus_nd"])
def test_columns_are_independent_and_repeatable(gpu, name):
    num, A, B = _numeric(name), pc.matrix(name)[0], _B(name)
    Ax = pc.values_rank3(A)
    b = B[:, 5]
    x, i1 = num.solve_pcg(b, Ax=Ax, tol=1e-12)
    assert i1["iters"] >= 2
    for pos in (0, 16):
        Bp = np.array(B, order="F")
        Bp[:, pos] = b
        Bp[:, (pos + 1) % 17] = 0.0  # a neighbour that stops at once
        X, info = num.solve_pcg(Bp, Ax=Ax, tol=1e-12)
        assert np.array_equal(bits(X[:, pos]), bits(x)), pos
        for f in info:
            assert info[f][pos] == i1[f], (f, pos)
    full = num.solve_pcg(B, Ax=Ax, tol=1e-12)
    assert _same(full, num.solve_pcg(B, Ax=Ax, tol=1e-12))
    assert _same(full, _fresh(name).solve_pcg(B, Ax=Ax, tol=1e-12))


def test_mixed_panels_keep_each_column_s_bits(gpu):
    """Columns that stop at once, after some steps and by a breakdown share a panel; each has the
    bits of its solo run with the same values."""
    num, A, B = _numeric("lap8"), pc.matrix("lap8")[0], _B("lap8")
    n = A.size()
    e5 = np.zeros(n)
    e5[5] = 1.0
    easy = rc.Exact.of(A).dense() @ e5  # x_0 = e_5 to rounding: row 100 of the residual is tiny
    for Ax, cols, want in (
            (pc.values_rank3(A), [np.zeros(n), B[:, 0], 1e6 * B[:, 1], B[:, 2]], None),
            (pc.values_diag(A, 100, -1e3), [easy, B[:, 0], np.zeros(n), B[:, 1]],
             [pc.CONVERGED, pc.BREAKDOWN, pc.CONVERGED, pc.BREAKDOWN]),
            (3.0 * A.x, [np.zeros(n), B[:, 0]], [pc.CONVERGED, pc.CONVERGED]),
            (-A.x, [np.zeros(n), B[:, 0]], [pc.CONVERGED, pc.BREAKDOWN])):
        P = np.asfortranarray(np.array(cols).T)
        X, info = num.solve_pcg(P, Ax=Ax)
        print(f"PCG lap8 mixed panel: states {info['state']}, iters {info['iters']}")
        if want is not None:
            assert list(info["state"]) == want
        else:
            assert info["iters"][0] == 0 and info["iters"][1] >= 2
        for c, b in enumerate(cols):
            x, i1 = num.solve_pcg(b, Ax=Ax)
            assert np.array_equal(bits(X[:, c]), bits(x)), c
            assert all(info[f][c] == i1[f] for f in info), c


# ---- 9. a factor that has moved away from the values ----
def test_after_an_update_the_values_still_rule(gpu):
    name = "lap8_nd"
    num, A, B = _fresh(name), pc.matrix(name)[0], _B(name)[:, :2]
    n = A.size()
    rows = pc.rank3_rows(n)
    W = (np.arange(4, dtype=np.int64), np.array(rows, dtype=np.int32), np.array([2.0, 3.0, 5.0]))
    assert num.update(W) == 0  # the factor now describes A + W W^T
    tol = 1e-10
    X, info = num.solve_pcg(B, Ax=A.x, tol=tol)
    print(f"PCG {name} after a rank-3 update: iters {info['iters']}, true {info['relres_true']}")
    assert np.all(info["state"] == pc.CONVERGED) and np.all((1 <= info["iters"]) & (info["iters"] <= 5))
    assert np.all(info["relres_true"] <= 2 * tol)
    assert np.allclose(X, _numeric(name).solve(np.asfortranarray(B)), rtol=1e-7)
