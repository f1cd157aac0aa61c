"""What the conjugate-gradient tests share: the inputs, a numpy model of the algorithm the
header documents, and exact arithmetic for the vector kernels' bounds.

The model is the yardstick of the GPU tests, so it is pinned by test_pcg_cases_cpu.py: dense
Cholesky of A as the preconditioner M, products with the dense A', 2-norms, and the stopping
and breakdown rules of include/sparsecholesky.h, step for step.
"""
import functools
from fractions import Fraction

import numpy as np

import sparsecholesky_amd as sc

import refine_cases as rc

U = rc.U
CONVERGED, MAXITER, BREAKDOWN = range(3)
RANK3 = (1.5, 3.0, 8.0)


def gamma(m):
    return m * U / (1.0 - m * U)


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def matrix(name):
    """name -> (upper CSC matrix, Symbolic keywords)."""
    if name == "bcsstk01":
        return rc.load("bcsstk01"), {}
    if name == "lap8":
        return sc.laplacian3d(8, nd=False), {}
    if name == "lap8_nd":
        return sc.laplacian3d(8, nd=False), dict(ordering=1)
    if name == "bus_nd":
        return rc.load("1138_bus"), dict(ordering=1)
    if name == "lap4_schur":
        import schur_cases

        return sc.laplacian3d(4, nd=False), dict(schur=schur_cases.plane(4, 2))
    raise KeyError(name)


def rank3_rows(n):
    return (1, n // 2, n - 2)


def values_rank3(A):
    """Three diagonal entries times 1.5, 3 and 8: inv(A) A' has three eigenvalues away from 1."""
    x = np.array(A.x, dtype=np.float64)
    for i, f in zip(rank3_rows(A.size()), RANK3):
        x[A.find_index(i, i)] *= f
    return x


def values_dad(A, eps, seed=5):
    """D A D with D = diag(1 + eps U(-1, 1))."""
    d = 1.0 + eps * np.random.default_rng(seed).uniform(-1.0, 1.0, A.size())
    cols = np.repeat(np.arange(A.size()), np.diff(A.p))
    return np.asarray(A.x, dtype=np.float64) * d[A.i] * d[cols]


def values_diag(A, i, v):
    x = np.array(A.x, dtype=np.float64)
    x[A.find_index(i, i)] = v
    return x


def dense(A, Ax=None):
    return rc.Exact.of(A, Ax).dense()


def rhs(n, k, seed=3):
    B = np.random.default_rng(seed).standard_normal((n, k))
    B.setflags(write=False)
    return B


# ---- the model ----
def emulate(Ad, Md, b, tol=1e-10, max_iter=100, x0=None, wrong=None):
    """One column of the documented algorithm in numpy: Ad the dense A', Md the dense factored
    matrix.  wrong: None, or a deliberate mistake ("beta_inverted": beta = rho / rho';
    "alpha_old_rho": alpha from the rho of the step before) for the tests that show the
    yardstick tells such a method from the right one.  Returns a dict: x, iters, state, relres
    (recurrence), relres_true, and the per-step relres history."""
    import scipy.linalg as sla

    c = sla.cho_factor(Md, lower=True)

    def M(v):
        return sla.cho_solve(c, v)

    def ok(v):
        return v > 0.0 and np.isfinite(v)

    b = np.asarray(b, dtype=np.float64)
    nb = np.linalg.norm(b)
    x = M(b) if x0 is None else np.array(x0, dtype=np.float64)
    r = b - Ad @ x
    hist = [np.linalg.norm(r)]
    iters, state = 0, None
    if hist[-1] <= tol * nb:
        state = CONVERGED
    elif max_iter == 0:
        state = MAXITER
    rho = rho_old = None
    p = None
    while state is None:
        z = M(r)
        rho_new = float(r @ z)
        if not ok(rho_new):
            state = BREAKDOWN
            break
        if p is None:
            p = z
        else:
            beta = rho / rho_new if wrong == "beta_inverted" else rho_new / rho
            p = z + beta * p
        rho_old, rho = rho, rho_new
        q = Ad @ p
        pq = float(p @ q)
        if not ok(pq):
            state = BREAKDOWN
            break
        alpha = (rho_old if wrong == "alpha_old_rho" and rho_old is not None else rho) / pq
        x = x + alpha * p
        r = r - alpha * q
        iters += 1
        hist.append(np.linalg.norm(r))
        if hist[-1] <= tol * nb:
            state = CONVERGED
        elif iters >= max_iter:
            state = MAXITER

    def rel(v):
        return 0.0 if v == 0.0 else v / nb

    return dict(x=x, iters=iters, state=state, relres=rel(hist[-1]), relres_true=rel(np.linalg.norm(b - Ad @ x)),
                hist=[rel(v) for v in hist])


# ---- exact arithmetic for the vector kernels ----
def frac(a):
    return [Fraction(float(v)) for v in a]


def exact_dot(u, v):
    """(sum u_i v_i, sum |u_i v_i|) as Fractions."""
    pr = [a * b for a, b in zip(frac(u), frac(v))]
    return sum(pr, Fraction(0)), sum((abs(t) for t in pr), Fraction(0))


def dot_within(fl, u, v):
    """|fl - u.v| <= gamma_n sum |u_i v_i|: any order of summation, products fused or not."""
    ex, ab = exact_dot(u, v)
    return abs(Fraction(float(fl)) - ex) <= Fraction(gamma(len(u))) * ab


def axpy_worst(fl, a, p, x):
    """max over the entries of |fl - (x + a p)| / (u (|a p| + |x + a p|) (1 + u)): at most 1 for
    a fused x + a p (one rounding) and for an unfused one (two)."""
    a = Fraction(float(a))
    w = 0.0
    for f, pi, xi in zip(frac(fl), frac(p), frac(x)):
        ex = xi + a * pi
        err = abs(f - ex)
        if err == 0:
            continue
        bound = Fraction(U) * (abs(a * pi) + abs(ex)) * (1 + Fraction(U))
        if bound == 0:
            return float("inf")
        w = max(w, float(err / bound))
    return w


def cancelling(n, k, seed):
    """(u, v, w), n x k: magnitudes over 2^-20 .. 2^20, v = +-u with alternating signs so the
    sum of u v is what is left of terms 2^40 apart; w independent of u."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, k)) * 2.0 ** rng.integers(-20, 21, (n, k))
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)[:, None]
    v = u * sign
    w = rng.standard_normal((n, k)) * 2.0 ** rng.integers(-20, 21, (n, k))
    return u, v, w
