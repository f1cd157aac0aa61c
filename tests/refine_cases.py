"""Exact arithmetic shared by the product / residual / refinement tests.

Everything a test compares against is computed in rational arithmetic (fractions.Fraction
over the few thousand entries of A), so nothing under test is its own yardstick:
  * products, residuals and |b| + |A| |x| are evaluated exactly from the full symmetric
    matrix given as (rows, cols, values);
  * x_ref is the exact solution to ~1e-70: refinement with exact residuals and a dense scipy
    Cholesky as the inner solver, 8 steps (each step gains a factor cond(A) u).
"""
import os
from fractions import Fraction

import numpy as np

import sparsecholesky_amd as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53


def gamma(m):
    return m * U / (1.0 - m * U)


def load(name):
    return sc.load_matrix_market_to_csc(os.path.join(GOLDEN, name + ".mtx"))


def expected_structure(A):
    """The full symmetric matrix of an upper CSC input by the factorization's rules (entries
    with row > column ignored, of duplicates the last one), as (rp, ci, sp): built here from
    the raw arrays with a dictionary and scipy.sparse, independently of the library."""
    import scipy.sparse as sp

    n = A.size()
    last = {}
    for k in range(n):
        for p in range(int(A.p[k]), int(A.p[k + 1])):
            i = int(A.i[p])
            if i <= k:
                last[(i, k)] = p
    rows, cols, idx = [], [], []
    for (i, k), p in last.items():
        rows.append(i), cols.append(k), idx.append(p + 1)
        if i != k:
            rows.append(k), cols.append(i), idx.append(p + 1)
    M = sp.csr_matrix((np.array(idx, dtype=np.int64), (np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64))),
                      shape=(n, n))
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.int64) - 1


class Exact:
    """A full (already mirrored) sparse matrix with exact products."""

    def __init__(self, n, rows, cols, vals):
        self.n = n
        self.rows = [int(r) for r in rows]
        self.cols = [int(c) for c in cols]
        self.fvals = np.asarray(vals, dtype=np.float64)
        self.vals = [Fraction(float(v)) for v in vals]
        self.rowlen = np.bincount(np.asarray(rows, dtype=np.int64), minlength=n) if n else np.zeros(0, dtype=np.int64)

    @classmethod
    def of(cls, A, Ax=None):
        """Of an upper CSC input, with other values than A.x if given."""
        rp, ci, sp = expected_structure(A)
        rows = np.repeat(np.arange(A.size()), np.diff(rp))
        return cls(A.size(), rows, ci, np.asarray(A.x if Ax is None else Ax, dtype=np.float64)[sp])

    def dense(self):
        M = np.zeros((self.n, self.n))
        M[self.rows, self.cols] = self.fvals
        return M

    def mul(self, x, absolute=False):
        """A x (or |A| |x|) exactly; x floats or Fractions."""
        xf = [Fraction(v) for v in x]
        if absolute:
            xf = [abs(v) for v in xf]
        y = [Fraction(0)] * self.n
        for r, c, v in zip(self.rows, self.cols, self.vals):
            y[r] += (abs(v) if absolute else v) * xf[c]
        return y

    def residual(self, b, x):
        return [Fraction(bi) - yi for bi, yi in zip(b, self.mul(x))]

    def denom(self, b, x):
        """|b| + |A| |x| exactly."""
        return [abs(Fraction(bi)) + yi for bi, yi in zip(b, self.mul(x, absolute=True))]

    def norm_inf(self):
        s = [Fraction(0)] * self.n
        for r, v in zip(self.rows, self.vals):
            s[r] += abs(v)
        return max(s) if s else Fraction(0)

    def solve(self, b, steps=8):
        """The exact solution of A x = b (Fractions) by refinement with exact residuals."""
        import scipy.linalg as sla

        c = sla.cho_factor(self.dense(), lower=True)
        x = [Fraction(0)] * self.n
        for _ in range(steps):
            r = np.array([float(v) for v in self.residual(b, x)])
            x = [xi + Fraction(float(di)) for xi, di in zip(x, sla.cho_solve(c, r))]
        return x

    def berr(self, b, x):
        """(normwise, componentwise) backward error of x, exactly, as floats; 0 / 0 = 0,
        nonzero / 0 = inf."""
        r = [abs(v) for v in self.residual(b, x)]
        w = self.denom(b, x)
        comp = Fraction(0)
        for ri, wi in zip(r, w):
            if wi == 0:
                if ri != 0:
                    return _norm_berr(self, r, b, x), float("inf")
            else:
                comp = max(comp, ri / wi)
        return _norm_berr(self, r, b, x), float(comp)


def _norm_berr(E, r, b, x):
    den = E.norm_inf() * max(abs(Fraction(v)) for v in x) + max(abs(Fraction(v)) for v in b)
    return 0.0 if den == 0 else float(max(r) / den)


def ferr(x, xref):
    """|x - xref|_inf / |xref|_inf, exactly, as a float."""
    num = max(abs(Fraction(float(a)) - b) for a, b in zip(x, xref))
    den = max(abs(b) for b in xref)
    return 0.0 if num == 0 else float(num / den)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)
