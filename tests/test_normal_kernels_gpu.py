"""The three normal-equations kernels alone, through sc_debug_normal_*, against exact arithmetic.

Bounds (derived, valid for any summation order; u = 2^-53, gamma_k = k u / (1 - k u)):
  * form entry, t its list length:  |S_e - exact| <= gamma_{t+3} (|c_e| + |d_i + lambda| + sum |J w J|)
    (two roundings per term, the sum, the base);
  * fp64 products, k the row / column length:  |R - exact| <= gamma_{k+2} (|b| + sum |a| |x|)
    (for the transposed product a = J w, one rounding more per term, inside the same gamma);
  * compensated residual:  |R - r| <= u |r| + gamma_{2k+4}^2 (|b| + sum |J| |x|), the Dot2 bound
    of test_spmv_kernels_gpu.py.
The residual data is cancellation-heavy, b = fl(J x), so a plain fp64 accumulation misses the
compensated bound by many orders of magnitude.
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import normal_cases as nc

pytestmark = pytest.mark.gpu

vp = ctypes.c_void_p
K = sc.NormalEquations.constants()
SHORT, LANES, CH, PCH = K["short"], K["lanes"], K["chunk"], K["product_chunk"]
MUL, FP64, DD = 0, 1, 2


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _p(t):
    return None if t is None else vp(t.data_ptr())


def _hp(a):
    return a.ctypes.data_as(vp)


# ---------------------------------------------------------------- the form
def _upper_pattern(n, seed, density):
    rng = np.random.default_rng(seed)
    M = np.triu(rng.random((n, n)) < density)
    return nc.csc_of(np.where(M, rng.standard_normal((n, n)), 0.0), M, upper=True)


def _inside(J, seed):
    rng = np.random.default_rng(seed)
    Sp, Si = nc.expected_pattern(J)
    n = J.n_cols
    M = np.zeros((n, n), dtype=bool)
    for j in range(n):
        for e in range(int(Sp[j]), int(Sp[j + 1])):
            M[Si[e], j] = rng.random() < 0.6
    return nc.csc_of(np.where(M, rng.standard_normal((n, n)), 0.0), M, upper=True)


_SMALL = np.zeros((7, 6))
_SMALL[[0, 1], 0] = 1.5, 2.0
_SMALL[[1, 2], 1] = -1.0, 0.5
_SMALL[3, 3] = 1.25
_SMALL[[3, 4], 4] = 2.0, 3.0
_SMALL[6, 5] = 0.75


def _form_cases():
    c = {
        # column 2 empty: its diagonal entry has no terms; columns 3 and 5 hold one entry: 1-term lists
        "empty_col_and_one_term": lambda: (nc.csc_of(_SMALL), None, "wd"),
        "wide_3x7": lambda: (nc.random_sparse(3, 7, 0.6, 41), None, "wd"),
        "one_row": lambda: (nc.random_sparse(1, 4, 1.0, 42), None, "w"),
        "one_col": lambda: (nc.random_sparse(6, 1, 0.8, 43), None, "d"),
        "no_rows": lambda: (nc.random_sparse(0, 3, 0.5, 44), _upper_pattern(3, 45, 0.7), "d"),
        "base_outside": lambda: (nc.random_sparse(12, 9, 0.2, 46), _upper_pattern(9, 47, 0.4), "wd"),
        "base_inside": lambda: (nc.random_sparse(12, 9, 0.3, 48), _inside(nc.random_sparse(12, 9, 0.3, 48), 49), "wd"),
        "negative_and_zero_weights": lambda: (nc.random_sparse(20, 6, 0.5, 50), None, "wneg"),
        "no_weights": lambda: (nc.random_sparse(20, 6, 0.5, 51), None, ""),
        "dense_1000": lambda: (nc.two_dense_columns(1000, 52), None, "wd"),
        "dense_1000_plus_chunk": lambda: (nc.two_dense_columns(1000 + CH, 53), None, "w"),
    }
    # one below, at and one above every boundary between the mappings: short | grouped | chunked,
    # and around the group width, where a lane's share goes from one term to two
    for L in sorted({SHORT - 1, SHORT, SHORT + 1, LANES - 1, LANES, LANES + 1, CH - 1, CH, CH + 1, 2 * CH, 2 * CH + 1}):
        if L >= 1:
            c[f"list_{L}"] = (lambda L=L: (nc.two_dense_columns(L, 60 + L), None, "w"))
    return c


FORM_CASES = _form_cases()


@functools.lru_cache(maxsize=None)
def _form_problem(name):
    J, base, flags = FORM_CASES[name]()
    rng = np.random.default_rng(len(name) + 7)
    m, n = J.n_rows, J.n_cols
    w = None
    if "wneg" in flags:
        w = rng.standard_normal(m)
        w[::3] = 0.0
    elif "w" in flags:
        w = rng.uniform(0.25, 4.0, m)
    d = rng.uniform(0.1, 1.0, n) if "d" in flags else None
    lam = 0.375 if "d" in flags else 0.0
    Cx = None if base is None else base.x
    ne_ = sc.NormalEquations(J, base)
    tp, pa, pb, r, cpos = ne_.term_lists()
    A = ne_.matrix()
    dcol = nc.diag_of(A.p, A.i)
    exact = nc.exact_form(J, J.x, w, base, Cx, d, lam)
    return J, base, w, d, lam, (tp, pa, pb, r, cpos, dcol), exact


def _run_form(name):
    J, base, w, d, lam, (tp, pa, pb, r, cpos, dcol), _ = _form_problem(name)
    ne = len(dcol)
    dJ = _dev(J.x) if len(J.x) else None
    dw = None if w is None else _dev(w)
    dC = None if base is None else _dev(base.x)
    dd = None if d is None else _dev(d)
    out = _dev(np.full(ne + 2, np.nan))  # a sentinel on either side of the window
    st = sc.lib().sc_debug_normal_form(
        ne, _hp(tp), _hp(pa), _hp(pb), _hp(r), _hp(cpos), _hp(dcol), len(J.x), J.n_rows,
        0 if base is None else len(base.x), J.n_cols, _p(dJ), _p(dw), _p(dC), _p(dd), lam,
        vp(out.data_ptr() + 8))
    assert st == 0, (st, sc.lib().sc_last_error())
    o = out.cpu().numpy()
    assert np.isnan(o[0]) and np.isnan(o[-1])
    return o[1:-1].copy()


@pytest.mark.parametrize("name", sorted(FORM_CASES))
def test_form_against_exact_arithmetic(name):
    vals, mags, lens = _form_problem(name)[6]
    S = _run_form(name)
    assert len(S) == len(vals) and np.all(np.isfinite(S))
    worst = 0.0
    for e in range(len(vals)):
        err = abs(Fraction(float(S[e])) - vals[e])
        bound = nc.gamma(lens[e] + 3) * mags[e]
        if mags[e]:
            worst = max(worst, float(err / mags[e]) / nc.gamma(lens[e] + 3))
        assert err <= bound, (e, lens[e], float(err), float(bound))
    print(f"{name}: lists {sorted(set(lens))}, worst error / bound {worst:.3f}")
    if name.startswith("list_"):
        assert set(lens) == {int(name[5:])}
    if name == "empty_col_and_one_term":
        J, _, _, d, lam = _form_problem(name)[:5]
        A = sc.NormalEquations(J).matrix()
        e = int(A.p[3]) - 1  # the diagonal entry of the empty column 2
        assert lens[e] == 0 and S[e] == d[2] + lam
        assert 1 in lens


def test_form_is_bitwise_repeatable():
    for name in ("dense_1000_plus_chunk", "base_outside", f"list_{LANES + 1}"):
        a, b = _run_form(name), _run_form(name)
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- the products
def _rows_of_lengths(lengths, ncols, seed):
    """A matrix whose row r has lengths[r] entries (the first columns)."""
    rng = np.random.default_rng(seed)
    M = np.zeros((len(lengths), ncols), dtype=bool)
    for r, k in enumerate(lengths):
        M[r, :k] = True
    return nc.csc_of(np.where(M, rng.standard_normal(M.shape), 0.0), M)


def _transposed(J):
    return nc.csc_of(nc.dense_of(J).T, nc.mask_of(J).T)


PROD_CASES = {
    "sparse_37x23": lambda: nc.random_sparse(37, 23, 0.2, 71, empty_cols=(5,), empty_rows=(11,)),
    "wide_3x7": lambda: nc.random_sparse(3, 7, 0.6, 72),
    "one_row": lambda: nc.random_sparse(1, 4, 1.0, 73),
    "one_col": lambda: nc.random_sparse(6, 1, 0.8, 74),
    # rows one below, at and one above the chunk, and one of two chunks and a bit
    "long_rows": lambda: _rows_of_lengths([PCH - 1, PCH, PCH + 1, 2 * PCH + 3, 0, 1], 2 * PCH + 3, 75),
    "long_cols": lambda: _transposed(_rows_of_lengths([PCH - 1, PCH, PCH + 1, 2 * PCH + 3, 0, 1], 2 * PCH + 3, 76)),
}


@functools.lru_cache(maxsize=None)
def _prod_problem(name, nrhs):
    J = PROD_CASES[name]()
    m, n = J.n_rows, J.n_cols
    rng = np.random.default_rng(80 + nrhs)
    X = rng.standard_normal((n, nrhs))
    Y = rng.standard_normal((m, nrhs))
    w = rng.uniform(-1.0, 3.0, m)
    w[::4] = 0.0
    ne_ = sc.NormalEquations(J)
    B = np.zeros((m, nrhs))
    mul, res, mult = [], [], []
    for c in range(nrhs):
        s, a, k = nc.exact_mul(J, J.x, X[:, c])
        mul.append((s, a, k))
        B[:, c] = [float(v) for v in s]  # b = fl(J x): the residual is all cancellation
        res.append(nc.exact_mul(J, J.x, X[:, c], b=B[:, c]))
        mult.append(nc.exact_mult(J, J.x, w, Y[:, c]))
    return J, ne_.rows(), X, Y, w, B, mul, res, mult


def _padded(M, ld, extra_cols=1):
    rows, k = M.shape
    buf = np.full((k + extra_cols, ld), np.nan)
    buf[:k, :rows] = M.T
    return _dev(buf)


def _unpad(t, rows, k):
    o = t.cpu().numpy()
    assert np.all(np.isnan(o[:, rows:])) and np.all(np.isnan(o[k:]))  # nothing outside the window
    return o[:k, :rows].T.copy()


def _run_mul(name, mode, X, B, pad=3):
    J, (rp, ci, sp) = _prod_problem(name, 1)[:2]
    m, n = J.n_rows, J.n_cols
    nrhs = X.shape[1]
    ldx, ldr = n + pad, m + pad
    dX, dB = _padded(X, ldx), _padded(B, ldr)
    dR = _padded(np.full((m, nrhs), np.nan), ldr)
    dJ = _dev(J.x)
    st = sc.lib().sc_debug_normal_mul(mode, m, n, _hp(rp), _hp(ci), _hp(sp), len(J.x), _p(dJ), nrhs, _p(dX), ldx,
                                      _p(dB), ldr, _p(dR), ldr)
    assert st == 0, (st, sc.lib().sc_last_error())
    return _unpad(dR, m, nrhs)


def _run_mult(name, Y, w, pad=3):
    J = _prod_problem(name, 1)[0]
    m, n = J.n_rows, J.n_cols
    nrhs = Y.shape[1]
    ldy, ldg = m + pad, n + pad
    dY = _padded(Y, ldy)
    dG = _padded(np.full((n, nrhs), np.nan), ldg)
    dJ, dw = _dev(J.x), (None if w is None else _dev(w))
    Jp, Ji = np.ascontiguousarray(J.p, dtype=np.int64), np.ascontiguousarray(J.i, dtype=np.int32)
    st = sc.lib().sc_debug_normal_mult(m, n, _hp(Jp), _hp(Ji), _p(dJ), _p(dw), nrhs, _p(dY), ldy, _p(dG), ldg)
    assert st == 0, (st, sc.lib().sc_last_error())
    return _unpad(dG, n, nrhs)


def _check(R, exact, extra, compensated=False):
    """Every entry of R against the exact column data (values, magnitudes, lengths)."""
    for c, (s, a, k) in enumerate(exact):
        for i in range(len(s)):
            err = abs(Fraction(float(R[i, c])) - s[i])
            if compensated:
                bound = Fraction(nc.U) * abs(s[i]) + Fraction(nc.gamma(2 * k[i] + 4)) ** 2 * a[i]
            else:
                bound = Fraction(nc.gamma(k[i] + extra)) * a[i]
            assert err <= bound, (i, c, k[i], float(err), float(bound))


@pytest.mark.parametrize("nrhs", [1, 3, 16])
@pytest.mark.parametrize("name", sorted(PROD_CASES))
def test_products_against_exact_arithmetic(name, nrhs):
    J, _, X, Y, w, B, mul, res, mult = _prod_problem(name, nrhs)
    _check(_run_mul(name, MUL, X, B), mul, 2)
    _check(_run_mul(name, FP64, X, B), res, 2)
    R = _run_mul(name, DD, X, B)
    _check(R, res, 0, compensated=True)
    _check(_run_mult(name, Y, w), mult, 2)
    if nrhs == 3:
        unweighted = [nc.exact_mult(J, J.x, None, Y[:, c]) for c in range(nrhs)]
        _check(_run_mult(name, Y, None), unweighted, 2)


def test_compensated_residual_needs_its_error_terms():
    # the fp64 residual of the same data misses the compensated bound: the bound is not vacuous
    name, nrhs = "long_rows", 3
    _, _, X, _, _, B, _, res, _ = _prod_problem(name, nrhs)
    R = _run_mul(name, FP64, X, B)
    with pytest.raises(AssertionError):
        _check(R, res, 0, compensated=True)


@pytest.mark.parametrize("name", ["sparse_37x23", "long_rows", "long_cols"])
def test_products_are_repeatable_and_columns_independent(name):
    nrhs = 16
    J, _, X, Y, w, B, *_ = _prod_problem(name, nrhs)
    perm = np.random.default_rng(9).permutation(nrhs)
    sub = [2, 7, 11]
    for run, A, Bm in ((lambda A, Bm, pad=3: _run_mul(name, MUL, A, Bm, pad), X, B),
                       (lambda A, Bm, pad=3: _run_mul(name, DD, A, Bm, pad), X, B),
                       (lambda A, Bm, pad=3: _run_mult(name, A, w, pad), Y, B)):
        full = run(A, Bm)
        assert run(A, Bm).tobytes() == full.tobytes()
        assert np.array_equal(run(A[:, perm], Bm[:, perm]), full[:, perm])
        assert np.array_equal(run(A[:, sub], Bm[:, sub]), full[:, sub])
        assert np.array_equal(run(A, Bm, pad=0), full)  # leading dimensions equal to the row counts


@pytest.mark.parametrize("nrhs", [17, 40])
def test_panel_loop_of_the_handle(nrhs):
    # more than one panel of 16 through the handle's device entry points; column c of a wide
    # call equals the same column sent through the kernels alone
    name = "sparse_37x23"
    J = _prod_problem(name, 1)[0]
    m, n = J.n_rows, J.n_cols
    rng = np.random.default_rng(90 + nrhs)
    X, Y, w = rng.standard_normal((n, nrhs)), rng.standard_normal((m, nrhs)), rng.uniform(0.5, 2.0, m)
    ne_ = sc.NormalEquations(J)
    Jx = _dev(J.x)
    R = ne_.mul_device(_dev(X), Jx).cpu().numpy()
    G = ne_.mul_t_device(_dev(Y), Jx, _dev(w)).cpu().numpy()
    zero = np.zeros((m, 16))
    for c0 in range(0, nrhs, 16):
        c1 = min(nrhs, c0 + 16)
        assert np.array_equal(R[:, c0:c1], _run_mul(name, MUL, X[:, c0:c1], zero[:, :c1 - c0]))
        assert np.array_equal(G[:, c0:c1], _run_mult(name, Y[:, c0:c1], w))
    assert np.array_equal(ne_.mul(X), R) and np.array_equal(ne_.mul_t(Y, w), G)  # the host forms: the same bits
    # and the wide results stand on their own against exact arithmetic
    _check(R, [nc.exact_mul(J, J.x, X[:, c]) for c in range(nrhs)], 2)
    _check(G, [nc.exact_mult(J, J.x, w, Y[:, c]) for c in range(nrhs)], 2)


def test_device_forms_wait_for_what_torch_has_queued():
    # a 16-column panel of 300,000 rows handed over row-major: the transposing copy torch queues
    # for it (and the zero fill of the output) must be done before the library's own stream reads
    # and writes the same memory; the host form of the same call is the yardstick
    m, n = 300_000, 1000
    rng = np.random.default_rng(97)
    rows = np.repeat(np.arange(m), 2)
    cols = (rng.integers(0, n, m)[:, None] + np.array([0, 1 + rng.integers(0, n - 1)])) .ravel() % n
    order = np.lexsort((rows, cols))
    p = np.zeros(n + 1, dtype=np.int64)
    np.add.at(p, cols + 1, 1)
    J = sc.csc_matrix(m, n, np.cumsum(p), rows[order].astype(np.int32), rng.standard_normal(2 * m), sc.sym.none)
    ne_ = sc.NormalEquations(J)
    Y, w = rng.standard_normal((m, 16)), rng.uniform(0.5, 2.0, m)
    want = ne_.mul_t(Y, w)
    Jx, dw = _dev(J.x), _dev(w)
    for _ in range(3):
        dY = _dev(Y)  # row-major (m, 16): contiguous() of its transpose is a real copy
        G = ne_.mul_t_device(dY, Jx, dw)
        assert np.array_equal(G.cpu().numpy(), want)
    X = rng.standard_normal((n, 16))
    assert np.array_equal(ne_.mul_device(_dev(X), Jx).cpu().numpy(), ne_.mul(X))


# ---------------------------------------------------------------- the pair path of the least-squares gradient
def _run_pair(name, X, B, w, pad=3):
    J, (rp, ci, sp) = _prod_problem(name, 1)[:2]
    m, n = J.n_rows, J.n_cols
    nrhs = X.shape[1]
    ldx, ldr, ldg = n + pad, m + pad, n + pad
    dX, dB = _padded(X, ldx), _padded(B, ldr)
    dR, dRl = (_padded(np.full((m, nrhs), np.nan), ldr) for _ in range(2))
    dG, dGl = (_padded(np.full((n, nrhs), np.nan), ldg) for _ in range(2))
    dJ, dw = _dev(J.x), (None if w is None else _dev(w))
    Jp, Ji = np.ascontiguousarray(J.p, dtype=np.int64), np.ascontiguousarray(J.i, dtype=np.int32)
    st = sc.lib().sc_debug_normal_pair(m, n, _hp(Jp), _hp(Ji), _hp(rp), _hp(ci), _hp(sp), _p(dJ), _p(dw), nrhs,
                                       _p(dX), ldx, _p(dB), ldr, _p(dR), _p(dRl), ldr, _p(dG), _p(dGl), ldg)
    assert st == 0, (st, sc.lib().sc_last_error())
    return _unpad(dR, m, nrhs), _unpad(dRl, m, nrhs), _unpad(dG, n, nrhs), _unpad(dGl, n, nrhs)


@pytest.mark.parametrize("name", ["sparse_37x23", "long_rows", "long_cols"])
def test_pair_path_is_twice_the_working_precision(name):
    """Bounds, k the row / column length.  The residual pair is Dot2 before its final rounding:
    |R + Rl - r| <= gamma_{2k+4}^2 (|b| + sum |J| |x|).  The pair product of the exact pair r =
    R + Rl: every product J w and (J w) R is split exactly, the three cross terms and the k
    additions of error terms are rounded (each relative u on quantities of size u |term|), J w's
    error times Rl is dropped: |G + Gl - sum J w r| <= gamma_{3k+6}^2 sum |J w r|.  Both halves
    are normalised: |low| <= u |high|.  long_rows / long_cols cut rows and columns above the
    chunk, so the chunked combine of the pair modes runs."""
    nrhs = 3
    J, _, X, _, w, B, _, res, _ = _prod_problem(name, nrhs)
    R, Rl, G, Gl = _run_pair(name, X, B, w)
    assert np.all(np.abs(Rl) <= nc.U * np.abs(R)) and np.all(np.abs(Gl) <= nc.U * np.abs(G))
    worst = 0.0
    for c in range(nrhs):
        s, a, k = res[c]
        for i in range(J.n_rows):
            err = abs(Fraction(float(R[i, c])) + Fraction(float(Rl[i, c])) - s[i])
            assert err <= Fraction(nc.gamma(2 * k[i] + 4)) ** 2 * a[i], (i, c, float(err))
        rr = [Fraction(float(R[i, c])) + Fraction(float(Rl[i, c])) for i in range(J.n_rows)]
        for j in range(J.n_cols):
            g = ga = Fraction(0)
            for q in range(int(J.p[j]), int(J.p[j + 1])):
                t = Fraction(float(J.x[q])) * Fraction(float(w[J.i[q]])) * rr[J.i[q]]
                g += t
                ga += abs(t)
            kj = int(J.p[j + 1] - J.p[j])
            err = abs(Fraction(float(G[j, c])) + Fraction(float(Gl[j, c])) - g)
            bound = Fraction(nc.gamma(3 * kj + 6)) ** 2 * ga
            assert err <= bound, (j, c, kj, float(err), float(bound))
            if ga:
                worst = max(worst, float(err / ga) / nc.U ** 2)
    print(f"{name}: worst pair-product error {worst:.2f} u^2 of the magnitude")
    # the rounded pair is the compensated residual kernel's own result, and a repeat gives equal bits
    assert np.array_equal(R + Rl, _run_mul(name, DD, X, B))
    again = _run_pair(name, X, B, w)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((R, Rl, G, Gl), again))


def test_debug_entry_points_validate_before_launching():
    L = sc.lib()
    J = nc.random_sparse(5, 4, 1.0, 95)
    ne_ = sc.NormalEquations(J)
    rp, ci, sp = ne_.rows()
    dJ, dX, dR = _dev(J.x), _dev(np.zeros((2, 4))), _dev(np.zeros((2, 5)))
    bad_ci = ci.copy()
    bad_ci[0] = 4
    assert L.sc_debug_normal_mul(MUL, 5, 4, _hp(rp), _hp(bad_ci), _hp(sp), len(J.x), _p(dJ), 2, _p(dX), 4, None, 0,
                                 _p(dR), 5) == -1
    assert L.sc_last_error().decode().startswith("sc_debug_normal_mul: ")
    assert L.sc_debug_normal_mul(MUL, 5, 4, _hp(rp), _hp(ci), _hp(sp), len(J.x), _p(dJ), 2, _p(dX), 3, None, 0,
                                 _p(dR), 5) == -1
    assert L.sc_debug_normal_mul(7, 5, 4, _hp(rp), _hp(ci), _hp(sp), len(J.x), _p(dJ), 2, _p(dX), 4, None, 0,
                                 _p(dR), 5) == -1
    assert L.sc_debug_normal_mul(MUL, 5, 4, _hp(rp), _hp(ci), _hp(sp), len(J.x), _p(dJ), 17, _p(dX), 4, None, 0,
                                 _p(dR), 5) == -1
    Jp, Ji = np.ascontiguousarray(J.p, dtype=np.int64), np.ascontiguousarray(J.i, dtype=np.int32)
    assert L.sc_debug_normal_mult(4, 4, _hp(Jp), _hp(Ji), _p(dJ), None, 2, _p(dR), 5, _p(dX), 4) == -1  # a row index == m
    assert L.sc_last_error().decode().startswith("sc_debug_normal_mult: ")
    tp, pa, pb, r, cpos = ne_.term_lists()
    A = ne_.matrix()
    dcol = nc.diag_of(A.p, A.i)
    dS = _dev(np.zeros(len(dcol)))
    assert L.sc_debug_normal_form(len(dcol), _hp(tp), _hp(pa), _hp(pb), _hp(r), _hp(cpos), _hp(dcol), len(J.x) - 1, 5,
                                  0, 4, _p(dJ), None, None, None, 0.0, _p(dS)) == -1  # a position outside Jx
    assert L.sc_last_error().decode().startswith("sc_debug_normal_form: ")
