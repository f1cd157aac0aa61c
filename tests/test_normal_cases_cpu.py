"""The normal-equations structure, the exact references and the emulations, without a GPU.

sc_normal_create is host code: its pattern, term lists and row structure are compared with
dense boolean algebra and dictionaries over J's raw arrays.  The exact evaluator is checked on
a hand-worked example, the emulations against it (and deliberately wrong variants must miss
the bound the GPU tests use), and the least-squares cap is asserted for the emulation on the
committed seeds before test_normal_gpu.py relies on it.
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest

import sparsecholesky_amd as sc

import normal_cases as nc

vp = ctypes.c_void_p


def _base_pattern(n, seed, inside_of=None):
    rng = np.random.default_rng(seed)
    if inside_of is not None:
        Sp, Si = nc.expected_pattern(inside_of)
        M = np.zeros((n, n), dtype=bool)
        for j in range(n):
            for e in range(int(Sp[j]), int(Sp[j + 1])):
                M[Si[e], j] = rng.random() < 0.5
    else:
        M = np.triu(rng.random((n, n)) < 0.3)
    return nc.csc_of(np.where(M, rng.standard_normal((n, n)), 0.0), M, upper=True)


STRUCT_CASES = {
    "sparse_12x9": lambda: (nc.random_sparse(12, 9, 0.3, 1, empty_cols=(4,)), None),
    "wide_3x7": lambda: (nc.random_sparse(3, 7, 0.5, 2), None),
    "one_row": lambda: (nc.random_sparse(1, 4, 1.0, 3), None),
    "one_col": lambda: (nc.random_sparse(6, 1, 0.7, 4), None),
    "no_rows": lambda: (nc.random_sparse(0, 3, 0.5, 5), _base_pattern(3, 6)),
    "base_outside": lambda: (nc.random_sparse(12, 9, 0.2, 7), _base_pattern(9, 8)),
    "base_inside": lambda: (nc.random_sparse(12, 9, 0.3, 9), _base_pattern(9, 10, inside_of=nc.random_sparse(12, 9, 0.3, 9))),
    "two_dense": lambda: (nc.two_dense_columns(40, 11), None),
}


@pytest.mark.parametrize("name", sorted(STRUCT_CASES))
def test_pattern_terms_and_rows_match_dense_algebra(name):
    J, base = STRUCT_CASES[name]()
    ne_ = sc.NormalEquations(J, base)
    Sp, Si = nc.expected_pattern(J, base)
    A = ne_.matrix()
    assert A.S == sc.sym.upper and A.n_rows == A.n_cols == J.n_cols
    assert np.array_equal(A.p, Sp) and np.array_equal(A.i, Si)
    lists, cpos = nc.expected_terms(J, base)
    tp, pa, pb, r, cp = ne_.term_lists()
    assert tp[0] == 0 and np.array_equal(np.diff(tp), [len(t) for t in lists])
    got = [list(zip(pa[tp[e]:tp[e + 1]].tolist(), pb[tp[e]:tp[e + 1]].tolist(), r[tp[e]:tp[e + 1]].tolist()))
           for e in range(len(lists))]
    assert got == lists
    assert cp.tolist() == cpos
    m = J.n_rows
    assert ne_.terms == sum(k * (k + 1) // 2 for k in nc.mask_of(J).sum(axis=1).tolist()) == int(tp[-1])
    # J by rows against a transpose built from the dense positions
    pos = np.full((m, J.n_cols), -1, dtype=np.int64)
    for j in range(J.n_cols):
        for q in range(int(J.p[j]), int(J.p[j + 1])):
            pos[J.i[q], j] = q
    rp, ci, sp = ne_.rows()
    assert rp[0] == 0 and len(rp) == m + 1
    for i in range(m):
        cols = np.flatnonzero(pos[i] >= 0)
        assert np.array_equal(ci[rp[i]:rp[i + 1]], cols) and np.array_equal(sp[rp[i]:rp[i + 1]], pos[i, cols])
    mem = ne_.memory()
    assert mem["terms"] == ne_.terms and mem["entries"] == len(Si) and mem["device_bytes"] == 0
    assert mem["host_bytes"] >= 12 * ne_.terms


def test_exact_evaluator_on_a_hand_worked_example():
    # J = [[1, 2], [0, 3], [4, 0]], w = (2, 1, 1/2), C = [[1, 1/4], [., 0]] upper, d = (1/2, 1), lambda = 1/8:
    # J^T W J = [[2 + 8, 4], [4, 8 + 9]]; S = [[10 + 1 + 5/8, 4 + 1/4], [., 17 + 9/8]]
    J = nc.csc_of(np.array([[1.0, 2.0], [0.0, 3.0], [4.0, 0.0]]))
    base = nc.csc_of(np.array([[1.0, 0.25], [0.0, 0.0]]), np.array([[True, True], [False, False]]), upper=True)
    w, d = np.array([2.0, 1.0, 0.5]), np.array([0.5, 1.0])
    vals, mags, lens = nc.exact_form(J, J.x, w, base, base.x, d, 0.125)
    assert vals == [Fraction(93, 8), Fraction(17, 4), Fraction(145, 8)]
    assert mags == vals and lens == [2, 1, 2]
    s, a, k = nc.exact_mul(J, J.x, np.array([1.0, -1.0]))
    assert s == [-1, -3, 4] and a == [3, 3, 4] and k == [2, 1, 1]
    s, a, k = nc.exact_mul(J, J.x, np.array([1.0, -1.0]), b=np.array([1.0, 1.0, 1.0]))
    assert s == [2, 4, -3] and a == [4, 4, 5]
    g, ga, k = nc.exact_mult(J, J.x, w, np.array([1.0, 1.0, -2.0]))
    assert g == [2 - 4, 4 + 3] and ga == [6, 7] and k == [2, 2]
    assert nc.exact_solve([[Fraction(2), Fraction(1)], [Fraction(1), Fraction(3)]], [Fraction(3), Fraction(5)]) == \
        [Fraction(4, 5), Fraction(7, 5)]
    # least squares by hand: J = [[1], [1]], w = (1, 3), b = (0, 4), lambda = 1: x = 12 / 5
    assert nc.exact_lstsq(np.array([[1.0], [1.0]]), np.array([1.0, 3.0]), np.array([0.0, 4.0]), lam=1.0) == \
        [Fraction(12, 5)]


def _form_problem():
    J = nc.random_sparse(12, 9, 0.4, 21)
    base = _base_pattern(9, 22)
    rng = np.random.default_rng(23)
    w = rng.uniform(0.5, 2.0, 12)
    d = rng.uniform(0.1, 1.0, 9)
    return J, base, w, d, 0.375


def _form_misses(vals, J, base, w, d, lam):
    ex, mags, lens = nc.exact_form(J, J.x, w, base, base.x, d, lam)
    return [e for e in range(len(ex))
            if abs(Fraction(float(vals[e])) - ex[e]) > nc.gamma(lens[e] + 3) * mags[e]]


def test_form_emulation_meets_the_bound_and_wrong_ones_do_not():
    J, base, w, d, lam = _form_problem()
    lists, cpos = nc.expected_terms(J, base)
    Sp, Si = nc.expected_pattern(J, base)
    diag = nc.diag_of(Sp, Si)
    good = nc.emulate_form(lists, cpos, diag, J.x, w, base.x, d, lam)
    assert _form_misses(good, J, base, w, d, lam) == []
    assert _form_misses(nc.emulate_form(lists, cpos, diag, J.x, w, base.x, d, lam, drop_weight=True), J, base, w, d, lam)
    off = _form_misses(nc.emulate_form(lists, cpos, diag, J.x, w, base.x, d, lam, shift_everywhere=True), J, base, w, d, lam)
    assert off and all(diag[e] < 0 for e in off)


@pytest.mark.parametrize("name", sorted(nc.LSQ_CASES))
def test_lstsq_emulation_stays_under_the_cap(name):
    c = nc.lstsq_case(name)
    assert c["J"].shape == (nc.LSQ_M, nc.LSQ_N) and np.all(c["J"] * 2.0 ** 20 == np.round(c["J"] * 2.0 ** 20))
    kexp = nc.LSQ_CASES[name][1]
    assert 0.3 * 10.0 ** kexp < np.linalg.cond(c["J"]) < 3.0 * 10.0 ** kexp
    xe = nc.lstsq_exact(c)
    if c["consistent"]:
        assert all(v.denominator == 1 for v in xe)  # b = J x_true exactly, x_true integers
    cap = nc.lstsq_cap(c, xe)
    for pair in (False, True):
        x, info = nc.emulate_lstsq(c["J"], c["w"], c["b"], c["C"], c["d"], c["lam"], pair=pair)
        err = nc.max_error(x, xe)
        print(f"{name} pair={pair}: err {err:.3e} cap {cap:.3e} state {info['state']} iters {info['iters']}")
        assert err <= cap
    # the compensated mode's model converges on every case; so the GPU test may ask for that state
    assert info["state"] == nc.CONVERGED


def test_refinement_is_the_point_at_kappa_1e5():
    c = nc.lstsq_case("consistent_1e5")
    xe = nc.lstsq_exact(c)
    x0, i0 = nc.emulate_lstsq(c["J"], c["w"], c["b"], max_iter=0)
    x, _ = nc.emulate_lstsq(c["J"], c["w"], c["b"])
    assert i0["state"] == nc.MAXITER and i0["iters"] == 0
    assert nc.max_error(x0, xe) > 1e-9  # the plain normal equations lose cond(J)^2 u
    assert nc.max_error(x, xe) * 1e3 <= nc.max_error(x0, xe)


def test_lstsq_emulation_with_a_missing_mirrored_term_misses_the_cap():
    c = nc.lstsq_case("base_1e3")
    xe = nc.lstsq_exact(c)
    x, _ = nc.emulate_lstsq(c["J"], c["w"], c["b"], c["C"], c["d"], c["lam"], mirrored=False)
    assert nc.max_error(x, xe) > nc.lstsq_cap(c, xe)


def test_known_answer_generators_agree():
    J, edges = nc.grid_incidence(3)
    assert J.n_rows == len(edges) + 27 and len(edges) == 3 * 9 * 2
    D = nc.dense_of(J)
    L = nc.grid_laplacian_plus_identity(3)
    Ld = nc.dense_of(L)
    assert np.array_equal(np.triu(D.T @ D), Ld)
    ne_ = sc.NormalEquations(J)
    A = ne_.matrix()
    assert np.array_equal(A.p, L.p) and np.array_equal(A.i, L.i)
    assert ne_.terms == 3 * len(edges) + 27


def _create(m, n, Jp, Ji, Cp=None, Ci=None):
    h = vp()
    a = [np.ascontiguousarray(v, dtype=t) if v is not None else None
         for v, t in ((Jp, np.int64), (Ji, np.int32), (Cp, np.int64), (Ci, np.int32))]
    rc = sc.lib().sc_normal_create(m, n, *[None if v is None else v.ctypes.data_as(vp) for v in a], -1, ctypes.byref(h))
    msg = sc.lib().sc_last_error().decode()
    if rc == 0:
        sc.lib().sc_normal_free(h)
    return rc, msg


def test_argument_errors_name_the_entry_point():
    ok = _create(3, 2, [0, 2, 3], [0, 2, 1])
    assert ok[0] == 0
    bad = [
        _create(3, 2, [0, 2, 3], [2, 0, 1]),           # rows descend
        _create(3, 2, [0, 2, 3], [0, 0, 1]),           # a row twice
        _create(3, 2, [0, 2, 3], [0, 3, 1]),           # row index == m
        _create(3, 2, [0, 2, 3], [-1, 2, 1]),          # negative row index
        _create(3, 2, [0, 2, 1], [0, 2, 1]),           # Jp descends
        _create(3, 2, [1, 2, 3], [0, 2, 1]),           # Jp[0] != 0
        _create(3, 2, [0, 2, 3], [0, 2, 1], [0, 1, 2], [1, 1]),  # base entry (1, 0): row > column
        _create(3, 2, [0, 2, 3], [0, 2, 1], [0, 0, 2], [1, 0]),  # base rows descend
        _create(-1, 2, [0, 0, 0], []),
    ]
    for rc, msg in bad:
        assert rc == -1 and msg.startswith("sc_normal_create: "), (rc, msg)
    assert "ascend" in bad[0][1] and "below the diagonal" in bad[6][1]
    # a term count above 2^40 is refused before anything of that size is allocated: 2^21 rows ... is
    # too large to build here, so the limit is exercised through its formula on one dense row
    n = 1 << 21
    rc, msg = _create(1, n, np.arange(n + 1), np.zeros(n, dtype=np.int32))
    assert rc == -1 and "2^40" in msg
    L = sc.lib()
    assert L.sc_normal_terms(None) == -1 and L.sc_last_error().decode().startswith("sc_normal_terms: ")
    assert L.sc_normal_pattern(None, None, None) == -1 and L.sc_last_error().decode().startswith("sc_normal_pattern: ")
    assert L.sc_normal_rows(None, None, None, None) == -1
    J = nc.random_sparse(5, 4, 0.5, 31)
    ne_ = sc.NormalEquations(J)
    X, Y = np.zeros((4, 2), order="F"), np.zeros((5, 2), order="F")
    for call, name in (
        (lambda: L.sc_normal_mul_host_multi(ne_.h, 2, J.x.ctypes.data_as(vp), X.ctypes.data_as(vp), 3, Y.ctypes.data_as(vp), 5),
         "sc_normal_mul_host_multi"),
        (lambda: L.sc_normal_mul_host_multi(ne_.h, 2, J.x.ctypes.data_as(vp), X.ctypes.data_as(vp), 4, Y.ctypes.data_as(vp), 4),
         "sc_normal_mul_host_multi"),
        (lambda: L.sc_normal_mult_host_multi(ne_.h, 2, J.x.ctypes.data_as(vp), None, Y.ctypes.data_as(vp), 4,
                                     X.ctypes.data_as(vp), 4), "sc_normal_mult_host_multi"),
        (lambda: L.sc_normal_mul_host_multi(ne_.h, -1, J.x.ctypes.data_as(vp), X.ctypes.data_as(vp), 4, Y.ctypes.data_as(vp), 5),
         "sc_normal_mul_host_multi"),
        (lambda: L.sc_normal_values_host(ne_.h, J.x.ctypes.data_as(vp), None, J.x.ctypes.data_as(vp), None, 0.0,
                                 Y.ctypes.data_as(vp)), "sc_normal_values_host"),  # base values without a base
        (lambda: L.sc_normal_values_host(ne_.h, None, None, None, None, 0.0, Y.ctypes.data_as(vp)), "sc_normal_values_host"),
        (lambda: L.sc_normal_factor_host(ne_.h, None, J.x.ctypes.data_as(vp), None, None, None, 0.0), "sc_normal_factor_host"),
        (lambda: L.sc_normal_lstsq_host_multi(ne_.h, None, None, 1, J.x.ctypes.data_as(vp), None, Y.ctypes.data_as(vp), 5,
                                      X.ctypes.data_as(vp), 4, None), "sc_normal_lstsq_host_multi"),
    ):
        rc = call()
        assert rc == -1 and L.sc_last_error().decode().startswith(name + ": "), (rc, name, L.sc_last_error())
    with pytest.raises(ValueError):
        sc.NormalEquations(J, base=nc.csc_of(np.eye(3), upper=True))


def test_the_new_symbols_are_bound_and_the_version_stays():
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ("sc_normal_create", "sc_normal_free", "sc_normal_pattern", "sc_normal_terms", "sc_normal_term_lists",
                 "sc_normal_rows", "sc_normal_memory", "sc_normal_constants", "sc_normal_values_host",
                 "sc_normal_values_device", "sc_normal_factor_host", "sc_normal_factor_device", "sc_normal_values_ptr",
                 "sc_normal_mul_host_multi", "sc_normal_mul_device_multi", "sc_normal_mult_host_multi",
                 "sc_normal_mult_device_multi", "sc_normal_lstsq_host_multi", "sc_normal_lstsq_device_multi",
                 "sc_debug_normal_form", "sc_debug_normal_mul", "sc_debug_normal_mult", "sc_debug_normal_pair"):
        assert name in sc.exported_symbols() and hasattr(so, name), name
    for meth in ("matrix", "rows", "values", "factor", "mul", "mul_t", "lstsq", "values_device", "factor_device",
                 "mul_device", "mul_t_device", "lstsq_device", "term_lists", "memory"):
        assert callable(getattr(sc.NormalEquations, meth))
    assert isinstance(sc.NormalEquations.terms, property) and isinstance(sc.NormalEquations.values_ptr, property)
    assert ctypes.sizeof(sc.LstsqInfo) == 32
    k = sc.NormalEquations.constants()
    assert 1 <= k["short"] < k["lanes"] <= k["chunk"] and k["chunk"] % k["lanes"] == 0 and k["product_chunk"] >= 16
    assert sc.lib().sc_version() == 121
