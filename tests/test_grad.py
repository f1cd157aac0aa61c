"""Gradients on A's pattern on the GPU (Numeric.logdet_grad / solve_grad / pattern_outer /
pattern_dot) against the dense numpy model of tests/grad_cases.py and against identities that
need no reference.

Bars.  logdet_grad is c_k times an entry of the selected inverse, so it takes the bar
test_selinv.py holds Z to: normwise over the entries, max(1e-12, 100 x the disagreement of two
dense CPU inverses in the same metric).  solve_grad's Bbar is the panel solve (forward-error bar
1e-10 of test_solve_multi.py on these inputs), and an error dBbar moves G_k by at most sum_c
(|dbbar_i| |x_j| + |dbbar_j| |x_i|) <= 2 sum_c |dbbar_c|_2 |x_c|_2; the dense reference takes the
same allowance, and the sum itself of 2 nrhs products rounds within 2 nrhs u of its terms' sizes:
    |G_k - ref_k| <= 4e-10 sum_c |bbar_c|_2 |x_c|_2 + 2 nrhs u sum_c (|bbar_i| |x_j| + |bbar_j| |x_i|).
Homogeneity: sum_k a_k dlogdet/da_k = tr(inv(A) A) = n (bar 1e-10 n, test_trace_of_A_times_Z's),
and sum_k a_k Abar_k = -<Bbar, A X> = -<Xbar, X> up to the residuals of the two solves, each
within the backward-error bar 1e-14 of test_solve_multi.py times n."""
import ctypes
import functools

import numpy as np
import pytest

import grad_cases as gc
import sparsecholesky_amd as sc
from test_solve_multi import _matrix

pytestmark = pytest.mark.gpu

SC_ERR_STATE = -5
NAMES = ("lap8", "bcsstk01", "1138_bus")
_handles = {}


def _numeric(name):
    """One factored handle per input, shared by the tests that only read."""
    if name not in _handles:
        A = _matrix(name)
        num = sc.Numeric(sc.Symbolic(A))
        assert num.factor(A.x) == 0
        _handles[name] = num
    return _handles[name]


@functools.lru_cache(maxsize=None)
def _dense_refs(name, scale=1.0):
    """(c Z1, c Z2) on the value slots: two dense inverses of scale x A, left unchanged."""
    import scipy.linalg as sla

    A = _matrix(name)
    n = A.size()
    D = gc.dense(n, A.p, A.i, A.x * scale)
    rows, cols, _ = gc.classify(n, A.p, A.i)
    c = np.where(rows == cols, 1.0, 2.0)
    Z1 = np.linalg.inv(D)
    X = sla.solve_triangular(np.linalg.cholesky(D), np.eye(n), lower=True)
    Z2 = X.T @ X
    r1, r2 = c * Z1[rows, cols], c * Z2[rows, cols]
    r1.setflags(write=False)
    r2.setflags(write=False)
    return r1, r2


def _logdet_check(name, g, scale=1.0):
    r1, r2 = _dense_refs(name, scale)
    d = np.abs(r1 - r2).max() / np.abs(r1).max()
    bar = max(1e-12, 100 * d)
    err = np.abs(g - r1).max() / np.abs(r1).max()
    print(f"{name}: logdet_grad normwise {err:.3e} (bar {bar:.3e}, references differ {d:.3e})")
    assert err < bar, (name, err, bar)


@pytest.mark.parametrize("name", NAMES)
def test_logdet_grad_vs_dense(gpu, name):
    _logdet_check(name, _numeric(name).logdet_grad())


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("nrhs", [1, 20])
def test_solve_grad_vs_dense(gpu, name, nrhs):
    A = _matrix(name)
    n = A.size()
    num = _numeric(name)
    rng = np.random.default_rng(nrhs)
    B, Xbar = rng.standard_normal((n, nrhs)), rng.standard_normal((n, nrhs))
    X = num.solve(B)
    Bbar, G = num.solve_grad(Xbar, X)
    assert np.array_equal(Bbar, num.solve(Xbar))
    assert np.array_equal(G, num.pattern_outer(Bbar, X, alpha=-1.0))
    _, ref = gc.solve_grad(n, A.p, A.i, A.x, Xbar, X)
    bound = (4e-10 * (np.linalg.norm(Bbar, axis=0) * np.linalg.norm(X, axis=0)).sum()
             + 2 * nrhs * gc.U * gc.outer(n, A.p, A.i, np.abs(Bbar), np.abs(X)))
    print(f"{name} nrhs {nrhs}: worst |G - ref| / bound {np.max(np.abs(G - ref) / bound):.3e}")
    assert np.all(np.abs(G - ref) <= bound)


def test_one_dimensional_right_hand_side(gpu):
    A = _matrix("bcsstk01")
    n = A.size()
    num = _numeric("bcsstk01")
    rng = np.random.default_rng(2)
    xbar, b = rng.standard_normal(n), rng.standard_normal(n)
    x = num.solve(b)
    bbar, G = num.solve_grad(xbar, x)
    assert bbar.shape == (n,)
    assert np.array_equal(bbar, num.solve(xbar[:, None])[:, 0])  # the panel solve of one column
    assert np.array_equal(G, num.pattern_outer(bbar, x, alpha=-1.0))
    assert np.array_equal(G, num.solve_grad(xbar[:, None], x[:, None])[1])


@pytest.mark.parametrize("name", NAMES)
def test_homogeneity_of_logdet(gpu, name):
    A = _matrix(name)
    num = _numeric(name)
    t = num.pattern_dot(num.logdet_grad(), A.x)
    print(f"{name}: sum a_k dlogdet/da_k - n = {t - A.size():.3e}")
    assert abs(t - A.size()) <= 1e-10 * A.size()


@pytest.mark.parametrize("name", NAMES)
def test_homogeneity_of_solve(gpu, name):
    A = _matrix(name)
    n = A.size()
    num = _numeric(name)
    rng = np.random.default_rng(6)
    B, Xbar = rng.standard_normal((n, 5)), rng.standard_normal((n, 5))
    X = num.solve(B)
    Bbar, G = num.solve_grad(Xbar, X)
    t = num.pattern_dot(G, A.x)
    nA = np.linalg.norm(gc.dense(n, A.p, A.i, A.x))
    fro = np.linalg.norm
    bar = 1e-14 * n * ((nA * fro(X) + fro(B)) * fro(Bbar) + (nA * fro(Bbar) + fro(Xbar)) * fro(X))
    print(f"{name}: sum a_k Abar_k + <Xbar, X> = {t + np.sum(Xbar * X):.3e} (bar {bar:.3e})")
    assert abs(t + np.sum(Xbar * X)) <= bar


def test_logdet_grad_follows_new_values(gpu):
    A = _matrix("bcsstk01")
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    g1 = num.logdet_grad()
    assert num.factor(2.0 * A.x) == 0  # the Z panel is stale now
    g2 = num.logdet_grad()
    _logdet_check("bcsstk01", g1)
    _logdet_check("bcsstk01", g2, scale=2.0)
    assert num.factor(A.x) == 0
    assert np.array_equal(num.logdet_grad(), g1)


def test_not_positive_definite_gives_the_status_and_writes_nothing(gpu):
    A = _matrix("bcsstk01")
    n, nnz = A.size(), len(A.x)
    x = A.x.copy()
    j = 20
    x[A.p[j + 1] - 1] = -1.0  # the diagonal of column j
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(x)
    assert st > 0
    L = sc.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    G = np.full(nnz, -7.0)
    Bbar = np.full((n, 2), -7.0, order="F")
    X = np.ones((n, 2), order="F")
    assert L.sc_logdet_grad_host(num.h, p(G)) == st
    assert L.sc_solve_grad_host(num.h, 2, p(X), n, p(X), n, p(Bbar), n, p(G)) == st
    assert np.all(G == -7.0) and np.all(Bbar == -7.0)
    with pytest.raises(sc.LibraryError, match="not positive definite"):
        num.logdet_grad()
    with pytest.raises(sc.LibraryError, match="not positive definite"):
        num.solve_grad(X, X)
    assert num.factor(A.x) == 0  # the handle recovers
    assert np.array_equal(num.logdet_grad(), _numeric("bcsstk01").logdet_grad())


def test_before_factorization(gpu):
    A = _matrix("bcsstk01")
    n, nnz = A.size(), len(A.x)
    num = sc.Numeric(sc.Symbolic(A))
    L = sc.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    G = np.full(nnz, -7.0)
    Bbar = np.full((n, 1), -7.0, order="F")
    X = np.ones((n, 1), order="F")
    assert L.sc_logdet_grad_host(num.h, p(G)) == SC_ERR_STATE
    assert L.sc_solve_grad_host(num.h, 1, p(X), n, p(X), n, p(Bbar), n, p(G)) == SC_ERR_STATE
    assert np.all(G == -7.0) and np.all(Bbar == -7.0)
    # the outer product and the dot never look at the factor
    rng = np.random.default_rng(8)
    U, V = rng.integers(-8, 9, (n, 3)).astype(float), rng.integers(-8, 9, (n, 3)).astype(float)
    g = num.pattern_outer(U, V)
    assert np.array_equal(g, gc.outer(n, A.p, A.i, U, V))
    assert num.pattern_dot(g, g) == float(np.sum(g * g))


def test_empty_panels_and_empty_matrix(gpu):
    A = _matrix("bcsstk01")
    n, nnz = A.size(), len(A.x)
    num = _numeric("bcsstk01")
    Z = np.zeros((n, 0))
    G0 = np.arange(nnz, dtype=np.float64)
    assert np.array_equal(num.pattern_outer(Z, Z), np.zeros(nnz))
    assert np.array_equal(num.pattern_outer(Z, Z, alpha=-1.0, beta=0.5, G=G0), 0.5 * G0)
    Bbar, G = num.solve_grad(Z, Z)
    assert Bbar.shape == (n, 0) and np.array_equal(G, np.zeros(nnz)) and not np.signbit(G).any()
    E = sc.csc_matrix(0, 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    e = sc.Numeric(sc.Symbolic(E))
    assert e.factor(np.zeros(0)) == 0
    assert e.logdet_grad().shape == (0,)
    assert e.pattern_outer(np.zeros((0, 2)), np.zeros((0, 2))).shape == (0,)
    assert e.pattern_dot(np.zeros(0), np.zeros(0)) == 0.0
    assert e.solve_grad(np.zeros((0, 2)), np.zeros((0, 2)))[1].shape == (0,)
