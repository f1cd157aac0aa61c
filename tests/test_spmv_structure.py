"""sc_spmv_structure: the full symmetric A by rows, in A's own numbering, as the products and
residuals read it.  Host only.  The expectation is built from the raw CSC arrays with a
dictionary and scipy.sparse (refine_cases.expected_structure), by the factorization's rules:
entries with row > column ignored, of duplicates the last one, every off-diagonal entry in
both rows, columns ascending, sp pointing at the input entry."""
import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc

import refine_cases as rc


def _diag(n):
    return sc.csc_matrix(n, n, np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32),
                         np.arange(1, n + 1, dtype=np.float64))


def _with_lower():
    """4 x 4 upper CSC with two entries below the diagonal, which the analysis ignores."""
    p = np.array([0, 2, 4, 7, 9], dtype=np.int64)
    i = np.array([0, 2, 0, 1, 1, 2, 3, 2, 3], dtype=np.int32)  # (2,0) and (3,2) lie below
    x = np.array([4.0, 99.0, 1.0, 5.0, 1.5, 6.0, 77.0, 0.5, 7.0])
    return sc.csc_matrix(4, 4, p, i, x)


def _with_duplicates():
    """5 x 5 upper CSC with (0,2) given three times, (3,3) twice and (1,4) twice: the last wins."""
    p = np.array([0, 1, 3, 7, 10, 14], dtype=np.int64)
    i = np.array([0, 0, 1, 0, 0, 2, 0, 2, 3, 3, 1, 3, 1, 4], dtype=np.int32)
    x = np.array([9.0, 1.0, 8.0, 100.0, -50.0, 7.0, 0.5, 1.0, -3.0, 6.0, 40.0, 0.25, -1.0, 5.0])
    return sc.csc_matrix(5, 5, p, i, x)


CASES = {
    "bcsstk01": lambda: rc.load("bcsstk01"),
    "1138_bus": lambda: rc.load("1138_bus"),
    "lap4": lambda: sc.laplacian3d(4, nd=False),
    "diag7": lambda: _diag(7),
    "n1": lambda: _diag(1),
    "n0": lambda: _diag(0),
    "lower_ignored": _with_lower,
    "duplicates": _with_duplicates,
}


def _symbolics(A):
    """The same input under every numbering the handle may use internally."""
    n = A.size()
    out = [("natural", sc.Symbolic(A, ordering=0))]
    if n > 1:
        out += [("nd", sc.Symbolic(A, ordering=1)), ("amd", sc.Symbolic(A, ordering=2)),
                ("schur", sc.Symbolic(A, schur=np.array([n - 1, 0], dtype=np.int32), ordering=1))]
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_structure_matches_scipy(case):
    A = CASES[case]()
    n = A.size()
    erp, eci, esp = rc.expected_structure(A)
    for name, S in _symbolics(A):
        rp, ci, sp = S.spmv_structure()
        count = sc.lib().sc_spmv_structure(S.h, None, None, None)
        print(f"SPMV-STRUCT {case}/{name}: n={n} entries={len(ci)} (expected {len(eci)}), count query {count}")
        assert count == len(ci) == len(eci)
        assert np.array_equal(rp, erp) and rp[0] == 0 and rp[-1] == len(ci)
        assert np.array_equal(ci, eci) and np.array_equal(sp, esp)
        for r in range(n):  # columns ascend strictly in every row
            assert np.all(np.diff(ci[rp[r]:rp[r + 1]]) > 0)
        # sp points at an input entry that holds this (row, column), mirrored or not
        rows = np.repeat(np.arange(n), np.diff(rp))
        cols_in = np.repeat(np.arange(n), np.diff(A.p))
        lo, hi = np.minimum(rows, ci), np.maximum(rows, ci)
        assert np.array_equal(A.i[sp], lo) and np.array_equal(cols_in[sp], hi)


def test_lower_entries_are_ignored():
    A = _with_lower()
    rp, ci, sp = sc.Symbolic(A, ordering=0).spmv_structure()
    assert 1 not in sp.tolist() and 6 not in sp.tolist()  # the two entries below the diagonal
    M = np.zeros((4, 4))
    M[np.repeat(np.arange(4), np.diff(rp)), ci] = A.x[sp]
    assert np.array_equal(M, np.array([[4, 1, 0, 0], [1, 5, 1.5, 0], [0, 1.5, 6, 0.5], [0, 0, 0.5, 7.0]]))


def test_duplicates_last_wins_like_the_oracle():
    """L L^T of the oracle's factor of the same arrays is the structure's dense matrix."""
    A = _with_duplicates()
    rp, ci, sp = sc.Symbolic(A, ordering=0).spmv_structure()
    n = A.size()
    M = np.zeros((n, n))
    M[np.repeat(np.arange(n), np.diff(rp)), ci] = A.x[sp]
    assert M[0, 2] == 0.5 and M[3, 3] == 6.0 and M[1, 4] == -1.0 and np.array_equal(M, M.T)
    st, Lp, Li, Lx = oracle.chol(A)
    assert st == 0
    L = np.zeros((n, n))
    L[Li, np.repeat(np.arange(n), np.diff(Lp))] = Lx
    err = np.abs(L @ L.T - M).max() / np.abs(M).max()
    print(f"SPMV-STRUCT duplicates: |L L^T - M|_max / |M|_max = {err:.3e} (bar {8 * n * rc.U:.3e})")
    assert err <= 8 * n * rc.U


def test_argument_rules():
    S = sc.Symbolic(_diag(3))
    L = sc.lib()
    ci = np.zeros(3, dtype=np.int32)
    assert L.sc_spmv_structure(None, None, None, None) == -1
    assert L.sc_spmv_structure(S.h, None, ci.ctypes.data, None) == -1
    assert b"sc_spmv_structure" in L.sc_last_error()
