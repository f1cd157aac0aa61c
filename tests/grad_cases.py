"""A numpy model of the gradient entry points (sc_value_entries, sc_pattern_outer_*,
sc_pattern_dot_*, sc_logdet_grad_*, sc_solve_grad_*) from (Ap, Ai, values) alone, the inputs the
gradient tests share, and the complex-step check that pins the model.

The model follows the header's definitions: a value slot is effective when its row is <= its
column and it is the last of the duplicates of its (row, column); the matrix is the symmetric one
those slots stand for, every other slot has derivative zero.

Complex step: for an analytic f and a real a, Im f(a + i h) / h = f'(a) (1 + O(h^2)), with no
subtraction, so h = 1e-30 |a_k| costs no digit.  log det is taken from numpy.linalg.slogdet on
the complex matrix (the argument of its unit `sign` is Im log det), the solve from
numpy.linalg.solve.  What is left is the rounding of two dense LU factorizations, of relative size
u cond_2(A) times a modest factor: the bar is 64 u cond_2(A) (6e-8 for 1138_bus)."""
import functools
import os

import numpy as np

import sparsecholesky_amd as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
NAMES = ("lap2", "lap3", "bcsstk01", "1138_bus", "six")
SAMPLES = 12


def six():
    """6 x 6, diagonally dominant, with entries below the diagonal (ignored) and duplicates (the
    last one counts): (Ap, Ai, Ax).  Rows ascend within a column, duplicates are adjacent."""
    cols = [
        [(0, 4.0), (2, 9.0)],                          # (2, 0) lies below the diagonal
        [(0, -1.0), (1, 7.0), (1, 4.5)],               # (1, 1) twice: 4.5 counts
        [(1, -0.5), (2, 4.0), (4, 3.0)],               # (4, 2) below
        [(0, 0.25), (0, -0.75), (3, 3.5)],             # (0, 3) twice: -0.75 counts
        [(2, -1.0), (3, 0.5), (4, 5.0)],
        [(1, -0.25), (4, 0.75), (5, 2.5), (5, 3.0)],   # (5, 5) twice: 3.0 counts
    ]
    Ap = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
    Ai = np.array([r for c in cols for r, _ in c], dtype=np.int32)
    Ax = np.array([v for c in cols for _, v in c], dtype=np.float64)
    return Ap, Ai, Ax


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The input as an sc.csc_matrix (arrays left unchanged by every user)."""
    if name == "six":
        Ap, Ai, Ax = six()
        A = sc.csc_matrix(6, 6, Ap, Ai, Ax)
    elif name.startswith("lap"):
        A = sc.laplacian3d(int(name[3:]), nd=False)
    else:
        A = sc.load_matrix_market_to_csc(os.path.join(GOLDEN, name + ".mtx"))
    for a in (A.p, A.i, A.x):
        a.setflags(write=False)
    return A


def classify(n, Ap, Ai):
    """(rows, cols, effective) per value slot."""
    Ap = np.asarray(Ap, dtype=np.int64)
    rows = np.asarray(Ai, dtype=np.int64)
    cols = np.repeat(np.arange(n, dtype=np.int64), np.diff(Ap))
    eff = rows <= cols
    last = {}
    for p in range(len(rows)):
        if eff[p]:
            key = (int(rows[p]), int(cols[p]))
            if key in last:
                eff[last[key]] = False
            last[key] = p
    return rows, cols, eff


def dense(n, Ap, Ai, x):
    """The symmetric matrix the effective slots stand for (dtype of x)."""
    rows, cols, eff = classify(n, Ap, Ai)
    x = np.asarray(x)
    A = np.zeros((n, n), dtype=x.dtype)
    A[rows[eff], cols[eff]] = x[eff]
    A[cols[eff], rows[eff]] = x[eff]
    return A


def outer(n, Ap, Ai, Um, Vm, alpha=1.0, beta=0.0, G=None, one_sided=False):
    rows, cols, eff = classify(n, Ap, Ai)
    Um = np.reshape(Um, (n, -1))
    Vm = np.reshape(Vm, (n, -1))
    s = (Um[rows] * Vm[cols]).sum(axis=1)
    if not one_sided:
        s = s + np.where(rows != cols, (Um[cols] * Vm[rows]).sum(axis=1), 0.0)
    out = alpha * s if beta == 0.0 else beta * np.asarray(G, dtype=np.float64) + alpha * s
    return np.where(eff, out, 0.0)


def dot(n, Ap, Ai, G, H):
    _, _, eff = classify(n, Ap, Ai)
    return float(np.sum(np.asarray(G)[eff] * np.asarray(H)[eff]))


def logdet_grad(n, Ap, Ai, x, off_factor=2.0, ignored=0.0):
    """off_factor and ignored: the knobs of the deliberately wrong models."""
    rows, cols, eff = classify(n, Ap, Ai)
    Z = np.linalg.inv(dense(n, Ap, Ai, x))
    g = np.where(rows == cols, 1.0, off_factor) * Z[rows, cols]
    return np.where(eff, g, ignored * Z[rows, cols])


def solve_grad(n, Ap, Ai, x, Xbar, X, one_sided=False):
    """(Bbar, G) for an upstream Xbar of X = inv(A) B."""
    Bbar = np.linalg.solve(dense(n, Ap, Ai, x), np.reshape(Xbar, (n, -1)))
    return Bbar.reshape(np.shape(Xbar)), outer(n, Ap, Ai, Bbar, X, alpha=-1.0, one_sided=one_sided)


@functools.lru_cache(maxsize=None)
def cond2(name):
    A = matrix(name)
    return float(np.linalg.cond(dense(A.size(), A.p, A.i, A.x)))


def sample_slots(name):
    """The slots the complex step visits: all of the 6 x 6, else 12 drawn with a fixed seed."""
    nnz = len(matrix(name).x)
    if name == "six" or nnz <= SAMPLES:
        return np.arange(nnz)
    return np.sort(np.random.default_rng(1138).choice(nnz, SAMPLES, replace=False))


def _step(x, k):
    xc = np.asarray(x, dtype=np.complex128).copy()
    h = 1e-30 * abs(x[k])
    xc[k] += 1j * h
    return xc, h


def complex_step_logdet(name, k):
    A = matrix(name)
    xc, h = _step(A.x, k)
    sign, _ = np.linalg.slogdet(dense(A.size(), A.p, A.i, xc))
    return float(np.angle(sign)) / h


@functools.lru_cache(maxsize=None)
def solve_data(name, nrhs=3):
    """(B, X, Xbar) for the solve checks: seeded, X = inv(A) B by the dense solve."""
    A = matrix(name)
    n = A.size()
    rng = np.random.default_rng(7)
    B = rng.standard_normal((n, nrhs))
    Xbar = rng.standard_normal((n, nrhs))
    X = np.linalg.solve(dense(n, A.p, A.i, A.x), B)
    for a in (B, X, Xbar):
        a.setflags(write=False)
    return B, X, Xbar


def complex_step_solve(name, k):
    """d <Xbar, X> / d a_k."""
    A = matrix(name)
    B, _, Xbar = solve_data(name)
    xc, h = _step(A.x, k)
    Xc = np.linalg.solve(dense(A.size(), A.p, A.i, xc), B.astype(np.complex128))
    return float(np.sum(Xbar * Xc.imag)) / h


def solve_scale(name):
    """Per slot sum_c (|bbar_i| |x_j| + |bbar_j| |x_i|): the size of the terms a solve gradient
    adds up, against which its deviation is measured (the sum itself may cancel)."""
    A = matrix(name)
    n = A.size()
    _, X, Xbar = solve_data(name)
    Bbar, _ = solve_grad(n, A.p, A.i, A.x, Xbar, X)
    return outer(n, A.p, A.i, np.abs(Bbar), np.abs(X)) + np.where(classify(n, A.p, A.i)[2], 0.0, 1.0)


def check_logdet_model(name, g):
    """Worst relative deviation of the model gradient g from the complex step over the samples.  An
    ignored slot has derivative zero exactly; a nonzero model value there counts as deviation 1."""
    worst = 0.0
    for k in sample_slots(name):
        cs = complex_step_logdet(name, int(k))
        dev = abs(g[k] - cs) / abs(cs) if cs != 0.0 else (0.0 if g[k] == 0.0 else 1.0)
        worst = max(worst, dev)
    return worst


def check_solve_model(name, g):
    worst = 0.0
    scale = solve_scale(name)
    for k in sample_slots(name):
        cs = complex_step_solve(name, int(k))
        worst = max(worst, abs(g[k] - cs) / scale[k])
    return worst
