"""Schur analysis on the host: the constrained ordering (interior by the ordering option on
the induced graph, then the caller's set in the given order) and its symbolic handle."""
import ctypes as C

import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc

import schur_cases as cases

ORDERINGS = [(0, "natural"), (1, "nd"), (2, "amd")]


def _case(name):
    if name == "1138_bus":
        A = cases.load(name)
        return A, cases.random_set(A.size(), 40, 11)
    if name == "bcsstk01":
        return cases.load(name), np.array([3, 47, 10, 22, 0], dtype=np.int32)
    if name == "lap8_plane":
        return sc.laplacian3d(8, nd=False), cases.plane(8, 4)
    assert name == "lap6_two_planes"
    return sc.laplacian3d(6, nd=False), np.concatenate([cases.plane(6, 1), cases.plane(6, 4)])


CASES = ["1138_bus", "bcsstk01", "lap8_plane", "lap6_two_planes"]


@pytest.mark.parametrize("ordering", ORDERINGS, ids=[o[1] for o in ORDERINGS])
@pytest.mark.parametrize("name", CASES)
def test_constrained_ordering_and_pattern(name, ordering):
    A, idx = _case(name)
    n, ns = A.size(), len(idx)
    s = sc.Symbolic(A, ordering=ordering[0], schur=idx)
    p = s.perm()
    assert np.array_equal(np.sort(p), np.arange(n))
    assert np.array_equal(p[n - ns:], idx)
    assert np.array_equal(s.schur_indices(), idx)
    assert sc.lib().sc_symbolic_perm(s.h, None) == 1  # always a permutation in effect
    if ordering[0] == 0:
        assert np.all(np.diff(p[: n - ns]) > 0)
    Lp, Li = s.pattern()
    Op, Oi, _ = oracle.schol(sc.permute_symmetric(A, p))
    assert np.array_equal(Lp, Op) and np.array_equal(Li, Oi)
    assert sc.lib().sc_memory_plan_check(s.h, 1) == 0
    assert sc.lib().sc_memory_plan_check(s.h, 2) == 0


@pytest.mark.parametrize("ordering", ORDERINGS, ids=[o[1] for o in ORDERINGS])
@pytest.mark.parametrize("name", ["1138_bus", "lap8_plane"])
def test_empty_set_is_the_plain_analysis(name, ordering):
    A, _ = _case(name)
    s0 = sc.Symbolic(A, ordering=ordering[0])
    s = sc.Symbolic(A, ordering=ordering[0], schur=[])
    assert len(s.schur_indices()) == 0 and len(s0.schur_indices()) == 0
    assert np.array_equal(s.perm(), s0.perm())
    assert sc.lib().sc_symbolic_perm(s.h, None) == sc.lib().sc_symbolic_perm(s0.h, None)
    assert s.stats() == s0.stats()
    for a, b in zip(s.pattern(), s0.pattern()):
        assert np.array_equal(a, b)
    assert s.schedule_digest() == s0.schedule_digest()


@pytest.mark.parametrize("ordering", ORDERINGS, ids=[o[1] for o in ORDERINGS])
def test_whole_matrix_as_the_set(ordering):
    A = cases.load("bcsstk01")
    n = A.size()
    idx = cases.random_set(n, n, 2)
    s = sc.Symbolic(A, ordering=ordering[0], schur=idx)
    assert np.array_equal(s.perm(), idx) and np.array_equal(s.schur_indices(), idx)
    Lp, Li = s.pattern()
    Op, Oi, _ = oracle.schol(sc.permute_symmetric(A, idx))
    assert np.array_equal(Lp, Op) and np.array_equal(Li, Oi)
    assert sc.lib().sc_memory_plan_check(s.h, 1) == 0


@pytest.mark.parametrize("ordering", [1, 2], ids=["nd", "amd"])
def test_disconnected_and_tiny_interiors(ordering):
    # a separator leaves a disconnected induced graph; all but one or two indices leave a tiny one
    A = sc.laplacian3d(6, nd=False)
    n = A.size()
    for idx in (cases.plane(6, 3), np.arange(1, n, dtype=np.int32), np.arange(2, n, dtype=np.int32),
                np.arange(0, n, 2, dtype=np.int32)):
        s = sc.Symbolic(A, ordering=ordering, schur=idx)
        p = s.perm()
        assert np.array_equal(np.sort(p), np.arange(n)) and np.array_equal(p[n - len(idx):], idx)
        Lp, Li = s.pattern()
        Op, Oi, _ = oracle.schol(sc.permute_symmetric(A, p))
        assert np.array_equal(Lp, Op) and np.array_equal(Li, Oi)


def _analyze_schur(A, ns, idx):
    h = C.c_void_p()
    opt = sc.default_options()
    arr = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32)
    rc = sc.lib().sc_analyze_schur(A.size(), sc._ptr(A.p), sc._ptr(A.i), C.byref(opt), ns, sc._ptr(arr), C.byref(h))
    if h:
        sc.lib().sc_free_symbolic(h)
    return rc, sc.lib().sc_last_error().decode()


def test_argument_errors_name_the_entry():
    A = cases.load("bcsstk01")
    n = A.size()
    rc, msg = _analyze_schur(A, 3, [1, n, 2])
    assert rc == -1 and "schur_idx[1]" in msg and str(n) in msg and "range" in msg
    rc, msg = _analyze_schur(A, 3, [1, -4, 2])
    assert rc == -1 and "schur_idx[1]" in msg and "-4" in msg
    rc, msg = _analyze_schur(A, 4, [7, 3, 9, 3])
    assert rc == -1 and "schur_idx[3]" in msg and "twice" in msg and "schur_idx[1]" in msg
    rc, msg = _analyze_schur(A, -1, [0])
    assert rc == -1 and "ns" in msg and "-1" in msg
    rc, msg = _analyze_schur(A, n + 1, np.arange(n + 1))
    assert rc == -1 and "ns" in msg and str(n + 1) in msg
    rc, msg = _analyze_schur(A, 2, None)
    assert rc == -1 and "null" in msg
    assert sc.lib().sc_analyze_schur(n, sc._ptr(A.p), sc._ptr(A.i), None, 0, None, None) == -1
    assert sc.lib().sc_symbolic_schur(None, None) == -1


def test_version_and_options_layout_unchanged():
    assert sc.lib().sc_version() == 121
    assert sc.default_options().struct_size == C.sizeof(sc.Options)
