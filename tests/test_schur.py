"""Schur complement of a chosen index set on the GPU: S_c = A_SS - A_SI inv(A_II) A_IS from
the trailing block of the factor, and the two partial solves around it.

Reference and bar.  R1 = A_SS - A_IS^T solve(A_II, A_IS) in dense numpy (LU) and R2, the same
through scipy's Cholesky; the error is relative Frobenius over the ns x ns matrix and the bar
per input max(1e-12, 100 x |R2 - R1| / |R1|): the project's rule.  The
condensed right-hand side uses the same rule per column in the 2-norm.  The expansion is
judged by its normwise backward error against A, |A x - b|_inf / (|A|_inf |x|_inf + |b|_inf)
per column, with 10 x the backward error of the handle's own panel solve of the same B as the
bar (the margin of 9.3 for a solve after an update; the dense solve with S_c in between is
backward stable)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import schur_cases as cases

pytestmark = pytest.mark.gpu

SC_ERR_ARG, SC_ERR_STATE, SC_ERR_NOTIMPL = -1, -5, -7


def _bus(ns, ordering):
    return lambda: (cases.load("1138_bus"), cases.random_set(1138, ns, 100 + ns), dict(ordering=ordering))


CASES = {
    "bcsstk01_td1": lambda: (cases.load("bcsstk01"), np.array([3, 47, 10, 22, 0], dtype=np.int32), dict(tiny_dense=1)),
    "bcsstk01_td0": lambda: (cases.load("bcsstk01"), np.array([3, 47, 10, 22, 0], dtype=np.int32), dict(tiny_dense=0)),
    "bus40_nat": _bus(40, 0), "bus40_nd": _bus(40, 1), "bus40_amd": _bus(40, 2),
    "bus130_nat": _bus(130, 0), "bus130_nd": _bus(130, 1), "bus130_amd": _bus(130, 2),
    "lap8_plane": lambda: (sc.laplacian3d(8, nd=False), cases.plane(8, 4), {}),
    "lap12_two_planes": lambda: (sc.laplacian3d(12, nd=False),
                                 np.concatenate([cases.plane(12, 8), cases.plane(12, 3)]), dict(small_front_max=0)),
    "lap16_nd_plane": lambda: (sc.laplacian3d(16, nd=False), cases.plane(16, 8), dict(ordering=1)),
    "dense100_all": lambda: (cases.dense_spd(100), cases.random_set(100, 100, 9), {}),
    "lap8_one": lambda: (sc.laplacian3d(8, nd=False), np.array([77], dtype=np.int32), {}),
}
SOLVE_CASES = ["bcsstk01_td1", "bus130_nd", "lap12_two_planes", "dense100_all", "lap8_one"]


@functools.lru_cache(maxsize=None)
def _input(case):
    A, idx, kw = CASES[case]()
    return A, idx, kw


def _fresh(case, factor=True):
    A, idx, kw = _input(case)
    num = sc.Numeric(sc.Symbolic(A, schur=idx, **kw))
    if factor:
        assert num.factor(A.x) == 0
    return num


@functools.lru_cache(maxsize=None)
def _numeric(case):
    """One factored handle per case, shared by the tests that only read."""
    return _fresh(case)


@functools.lru_cache(maxsize=None)
def _refs(case):
    A, idx, _ = _input(case)
    R1, R2 = cases.schur_refs(A, idx)
    R1.setflags(write=False)
    return R1, cases.bar(R1, R2), np.linalg.norm(R2 - R1) / np.linalg.norm(R1)


def _fro(X, R):
    return np.linalg.norm(X - R) / np.linalg.norm(R)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ---- 1. D and S_c ----
@pytest.mark.parametrize("case", list(CASES))
def test_schur_complement_vs_dense(gpu, case):
    A, idx, _ = _input(case)
    n, ns = A.size(), len(idx)
    num = _numeric(case)
    assert np.array_equal(num.symb.schur_indices(), idx)
    S = num.schur_complement()
    D = num.schur_factor()
    R1, bar, dis = _refs(case)
    err = _fro(S, R1)
    print(f"SCHUR {case}: n={n} ns={ns} |S_c - R1|/|R1| = {err:.3e} (bar {bar:.3e}, references differ {dis:.3e})")
    assert S.shape == (ns, ns) and err < bar, (case, err, bar)
    assert np.array_equal(S, S.T)
    # D: lower triangular, an exactly zero upper triangle, the trailing block of the export bit for bit
    assert np.all(D[np.triu_indices(ns, 1)] == 0.0) and np.all(np.diag(D) > 0)
    st, L = num.export()
    assert st == 0
    cols = np.repeat(np.arange(n), np.diff(L.p))
    T = np.zeros((ns, ns))
    keep = (cols >= n - ns) & (L.i >= n - ns)
    T[L.i[keep] - (n - ns), cols[keep] - (n - ns)] = L.x[keep]
    assert np.array_equal(_bits(D), _bits(T))
    assert _fro(D @ D.T, R1) < bar


@pytest.mark.parametrize("case", ["bcsstk01_td1", "bus130_amd", "lap12_two_planes", "lap8_one"])
def test_padding_and_device_forms(gpu, case):
    _, idx, _ = _input(case)
    ns = len(idx)
    num = _numeric(case)
    ld = ns + 3
    rng = np.random.default_rng(1)
    fill = rng.standard_normal(8 + ld * ns + 8)
    for fn, host in ((num.schur_complement_device, num.schur_complement()), (num.schur_factor_device, num.schur_factor())):
        d = torch.tensor(fill, device="cuda", dtype=torch.float64)
        assert fn(d.data_ptr() + 64, ld) == 0
        out = d.cpu().numpy()
        V, F = out[8:8 + ld * ns].reshape(ns, ld).T, fill[8:8 + ld * ns].reshape(ns, ld).T
        assert np.array_equal(_bits(V[:ns]), _bits(host))
        assert np.array_equal(_bits(V[ns:]), _bits(F[ns:]))
        assert np.array_equal(out[:8], fill[:8]) and np.array_equal(out[-8:], fill[-8:])
    # host forms honour the leading dimension too
    H = np.asfortranarray(fill[: ld * ns].reshape(ns, ld).T.copy())
    keep = H.copy()
    assert sc.lib().sc_schur_matrix_host(num.h, H.ctypes.data_as(ctypes.c_void_p), ld) == 0
    assert np.array_equal(_bits(H[:ns]), _bits(num.schur_complement())) and np.array_equal(H[ns:], keep[ns:])


@pytest.mark.parametrize("case", ["bcsstk01_td0", "bus130_nd", "lap12_two_planes"])
def test_bitwise_repeatable_and_refactorization(gpu, case):
    A, idx, _ = _input(case)
    num = _numeric(case)
    S, D = num.schur_complement(), num.schur_factor()
    assert np.array_equal(_bits(num.schur_complement()), _bits(S))
    other = _fresh(case)
    assert np.array_equal(_bits(other.schur_complement()), _bits(S))
    assert np.array_equal(_bits(other.schur_factor()), _bits(D))
    assert other.factor(A.x) == 0  # the same values again
    assert np.array_equal(_bits(other.schur_complement()), _bits(S))
    # 2 A: 2 S_c to rounding, and no stale D
    assert other.factor(2.0 * A.x) == 0
    R1, bar, _ = _refs(case)
    S2 = other.schur_complement()
    err = _fro(S2, 2.0 * R1)
    print(f"SCHUR {case}: refactored 2A: |S_c - 2 R1|/|2 R1| = {err:.3e} (bar {bar:.3e})")
    assert err < bar
    D2 = other.schur_factor()
    assert not np.array_equal(D2, D) and _fro(D2 @ D2.T, 2.0 * R1) < bar


# ---- 2. the partial solves ----
def _dense_parts(case):
    A, idx, _ = _input(case)
    return (A, idx) + cases.split(A, idx)


@functools.lru_cache(maxsize=None)
def _rhs(case):
    A, _, _ = _input(case)
    B = np.random.default_rng(7).standard_normal((A.size(), 17))
    B.setflags(write=False)
    return B


def _berr(M, X, B):
    X, B = X.reshape(len(X), -1), B.reshape(len(B), -1)
    na = np.abs(M).sum(axis=1).max()
    return np.abs(M @ X - B).max(axis=0) / (na * np.abs(X).max(axis=0) + np.abs(B).max(axis=0))


def _solve_device_multi(num, B):
    n, k = B.shape
    d = torch.tensor(np.asfortranarray(B).T.copy(), device="cuda", dtype=torch.float64)  # (k, n) rows = columns of B
    assert num.solve_device_multi(d.data_ptr(), k, n, d.data_ptr(), n) == 0
    return d.cpu().numpy().T.copy()


@pytest.mark.parametrize("case", SOLVE_CASES)
def test_condense_and_expand(gpu, case):
    import scipy.linalg as sla

    A, idx, AII, AIS, ASS, I = _dense_parts(case)
    n, ns = A.size(), len(idx)
    num = _numeric(case)
    M = sc.csc_to_dense(A)
    Sc = num.schur_complement()
    Ball = _rhs(case)
    for k in (1, 3, 16, 17, 0):  # 0: the 1-D form
        B = Ball[:, 0].copy() if k == 0 else Ball[:, :k].copy()
        B2 = B.reshape(n, -1)
        G = num.schur_condense(B)
        assert G.shape == ((ns,) if k == 0 else (ns, k))
        if len(I):
            g1 = B2[idx] - AIS.T @ np.linalg.solve(AII, B2[I])
            g2 = B2[idx] - AIS.T @ sla.cho_solve(sla.cho_factor(AII, lower=True), B2[I])
        else:
            g1 = g2 = B2[idx]
        dis = (np.linalg.norm(g2 - g1, axis=0) / np.linalg.norm(g1, axis=0)).max()
        gbar = max(1e-12, 100 * dis)
        gerr = (np.linalg.norm(G.reshape(ns, -1) - g1, axis=0) / np.linalg.norm(g1, axis=0)).max()
        XS = np.linalg.solve(Sc, G)
        X = num.schur_expand(B, XS)
        assert X.shape == B.shape
        assert np.array_equal(_bits(X.reshape(n, -1)[idx]), _bits(XS.reshape(ns, -1)))
        be = _berr(M, X, B)
        be0 = _berr(M, _solve_device_multi(num, B2), B2)
        ratio = (be / be0).max()
        print(f"SCHUR {case} k={k}: condense {gerr:.3e} (bar {gbar:.3e}); expand backward error {be.max():.3e}, "
              f"the panel solve's {be0.max():.3e}, worst ratio {ratio:.2f}")
        assert gerr < gbar, (case, k, gerr, gbar)
        assert np.all(be <= 10 * be0), (case, k, ratio)


@pytest.mark.parametrize("case", ["bus130_nd", "lap12_two_planes"])
def test_columns_are_independent_and_repeatable(gpu, case):
    A, idx, _ = _input(case)
    num = _numeric(case)
    B = _rhs(case)
    G17, G1 = num.schur_condense(B), num.schur_condense(B[:, :1])
    assert np.array_equal(_bits(G17[:, 0]), _bits(G1[:, 0]))
    assert np.array_equal(_bits(G17[:, 0]), _bits(num.schur_condense(B[:, 0].copy())))
    assert np.array_equal(_bits(num.schur_condense(B)), _bits(G17))
    XS = np.random.default_rng(8).standard_normal((len(idx), 17))
    X17, X1 = num.schur_expand(B, XS), num.schur_expand(B[:, :1], XS[:, :1])
    assert np.array_equal(_bits(X17[:, 0]), _bits(X1[:, 0]))
    assert np.array_equal(_bits(num.schur_expand(B, XS)), _bits(X17))
    other = _fresh(case)
    assert np.array_equal(_bits(other.schur_condense(B)), _bits(G17))
    assert np.array_equal(_bits(other.schur_expand(B, XS)), _bits(X17))


@pytest.mark.parametrize("case", ["bus130_nd", "lap8_plane"])
def test_device_forms_leading_dimensions_and_aliasing(gpu, case):
    A, idx, _ = _input(case)
    n, ns, k = A.size(), len(idx), 5
    num = _numeric(case)
    B = _rhs(case)[:, :k]
    G = num.schur_condense(B)
    XS = np.random.default_rng(8).standard_normal((ns, k))
    X = num.schur_expand(B, XS)
    ldb, ldg, ldxs, ldx = n + 3, ns + 2, ns + 5, n + 7

    def dev(Mx, ld):
        buf = np.full((Mx.shape[1], ld), -7.0)
        buf[:, : Mx.shape[0]] = Mx.T
        return torch.tensor(buf, device="cuda", dtype=torch.float64)

    dB, dG = dev(B, ldb), dev(np.full((ns, k), -7.0), ldg)
    assert num.schur_condense_device_multi(dB.data_ptr(), k, ldb, dG.data_ptr(), ldg) == 0
    g = dG.cpu().numpy()
    assert np.array_equal(_bits(g[:, :ns].T), _bits(G)) and np.all(g[:, ns:] == -7.0)
    assert np.array_equal(dB.cpu().numpy()[:, :n].T, B)
    dXS, dX = dev(XS, ldxs), dev(np.full((n, k), -7.0), ldx)
    assert num.schur_expand_device_multi(dB.data_ptr(), k, ldb, dXS.data_ptr(), ldxs, dX.data_ptr(), ldx) == 0
    x = dX.cpu().numpy()
    assert np.array_equal(_bits(x[:, :n].T), _bits(X)) and np.all(x[:, n:] == -7.0)
    # X = B
    assert num.schur_expand_device_multi(dB.data_ptr(), k, ldb, dXS.data_ptr(), ldxs, dB.data_ptr(), ldb) == 0
    b = dB.cpu().numpy()
    assert np.array_equal(_bits(b[:, :n].T), _bits(X)) and np.all(b[:, n:] == -7.0)
    # argument rules
    L = sc.lib()
    p = ctypes.c_void_p
    assert L.sc_schur_condense_device_multi(num.h, k, p(dB.data_ptr()), n - 1, p(dG.data_ptr()), ldg) == SC_ERR_ARG
    assert L.sc_schur_condense_device_multi(num.h, k, p(dB.data_ptr()), ldb, p(dG.data_ptr()), ns - 1) == SC_ERR_ARG
    assert L.sc_schur_condense_device_multi(num.h, k, p(dB.data_ptr()), ldb, None, ldg) == SC_ERR_ARG
    assert L.sc_schur_condense_device_multi(num.h, -1, p(dB.data_ptr()), ldb, p(dG.data_ptr()), ldg) == SC_ERR_ARG
    assert L.sc_schur_condense_device_multi(num.h, 0, None, ldb, None, ldg) == 0
    assert L.sc_schur_expand_device_multi(num.h, k, p(dB.data_ptr()), ldb, p(dXS.data_ptr()), ns - 1, p(dX.data_ptr()),
                                          ldx) == SC_ERR_ARG
    assert L.sc_schur_expand_device_multi(num.h, k, p(dB.data_ptr()), ldb, p(dXS.data_ptr()), ldxs, p(dB.data_ptr()),
                                          ldx) == SC_ERR_ARG  # X aliases B with another leading dimension
    assert L.sc_schur_expand_device_multi(num.h, 0, None, ldb, None, ldxs, None, ldx) == 0
    assert L.sc_schur_matrix_device(num.h, p(dX.data_ptr()), ns - 1) == SC_ERR_ARG
    assert L.sc_schur_factor_device(num.h, None, ns) == SC_ERR_ARG
    assert L.sc_schur_matrix_host(None, None, ns) == SC_ERR_ARG


# ---- 3. interplay with the other entry points ----
# The Schur handle and the plain handle eliminate in different orders.  Each solve is backward
# stable, so the two answers differ by up to a modest multiple of cond(A) u: agreement to 1e-12
# is a property of the code only where cond(A) u is far below 1e-12.  That holds for the
# Laplacians (cond_2 about 4 (k + 1)^2 / pi^2: 70 at k = 12, 120 at k = 16) and the dense
# matrix (M M^T + n I, cond_2 about 5); they carry the 1e-12 bar.  1138_bus (cond_2 8.6e6) and
# bcsstk01 (8.8e5) cannot promise it under any ordering: they are held to 10 cond_2(A) u, the
# forward-error bound of a backward-stable solve with a constant of 10, and the measured
# distance is printed.  logdet is held to 1e-12 of 2 sum |log L_jj| on every input.
WELL = ["lap12_two_planes", "lap8_plane", "lap16_nd_plane", "dense100_all"]
ILL = ["bus130_nd", "bcsstk01_td1"]


@pytest.mark.parametrize("case", WELL + ILL)
def test_other_entry_points_on_a_schur_handle(gpu, case):
    A, idx, kw = _input(case)
    n = A.size()
    num = _numeric(case)
    plain = sc.Numeric(sc.Symbolic(A, **kw))
    assert plain.factor(A.x) == 0
    M = sc.csc_to_dense(A)
    tol = 1e-12 if case in WELL else 10 * np.linalg.cond(M) * 2.0 ** -53
    b = np.random.default_rng(3).standard_normal(n)
    rel = lambda x, y: np.linalg.norm(x - y) / np.linalg.norm(y)
    B = _rhs(case)[:, :3]
    worst = max(rel(num.solve(b), plain.solve(b)), rel(num.solve(B), plain.solve(B)))
    # A^-1 = P^T L^-T L^-1 P and A = P^T L L^T P on either handle
    for h in (num, plain):
        worst = max(worst, rel(h.apply_Pt(h.solve_Lt(h.solve_L(h.apply_P(b)))), plain.solve(b)))
    prod = rel(num.apply_Pt(num.mul_L(num.mul_Lt(num.apply_P(b)))), M @ b)
    print(f"SCHUR {case}: solves and half solves against the plain handle {worst:.3e} (bar {tol:.3e}); "
          f"P^T L L^T P b against A b {prod:.3e}")
    assert worst < tol and prod < 1e-12
    st, L = num.export()
    cols = np.repeat(np.arange(n), np.diff(L.p))
    diag = L.x[L.i == cols]
    scale = 2.0 * np.abs(np.log(diag)).sum()
    assert abs(num.logdet() - plain.logdet()) <= 1e-12 * scale
    # log det A = log det A_II + log det S_c
    _, _, AII, _, _, I = _dense_parts(case)
    ld_i = np.linalg.slogdet(AII)[1] if len(I) else 0.0
    ld_s = np.linalg.slogdet(num.schur_complement())[1]
    print(f"SCHUR {case}: logdet {num.logdet():.12e} = {ld_i:.12e} + {ld_s:.12e}")
    assert abs(num.logdet() - (ld_i + ld_s)) <= 1e-12 * scale


@pytest.mark.parametrize("case", ["bus130_nd", "lap12_two_planes"])
def test_update_at_a_schur_index_makes_the_cache_stale(gpu, case):
    A, idx, _ = _input(case)
    n, ns = A.size(), len(idx)
    num = _fresh(case)
    S0 = num.schur_complement()
    q = ns // 3
    w = np.zeros(n)
    w[idx[q]] = 1.0
    assert num.update(w) == 0
    S1 = num.schur_complement()
    R1, bar, _ = _refs(case)
    want = S0.copy()
    want[q, q] += 1.0
    err = _fro(S1, want)
    print(f"SCHUR {case}: after update(e_{int(idx[q])}): |S_c - (S_c + e e^T)|/|.| = {err:.3e} (bar {bar:.3e})")
    assert err < bar and not np.array_equal(S1, S0)
    Rw = np.array(R1)
    Rw[q, q] += 1.0
    assert _fro(S1, Rw) < bar


@pytest.mark.parametrize("case", ["bus130_nd", "lap12_two_planes"])
def test_inverse_diagonal_at_the_schur_indices(gpu, case):
    A, idx, _ = _input(case)
    num = _numeric(case)
    d = num.inverse_diagonal()[idx]
    R1, _, _ = _refs(case)
    r1 = np.diag(np.linalg.inv(R1))
    r2 = np.diag(np.linalg.inv(sc.csc_to_dense(A)))[idx]
    dis = (np.abs(r2 - r1) / np.abs(r1)).max()
    bar = max(1e-12, 100 * dis)  # test_selinv's bar for the diagonal: entrywise, two references
    err = (np.abs(d - r1) / np.abs(r1)).max()
    print(f"SCHUR {case}: diag(A^-1) at S against diag(inv(S_c)): {err:.3e} (bar {bar:.3e})")
    assert err < bar
    ds = np.diag(np.linalg.inv(num.schur_complement()))
    assert (np.abs(d - ds) / np.abs(ds)).max() < bar


# ---- 4. state, status and memory ----
def _outputs(n, ns, k=2):
    return [np.full((max(ns, 1), max(ns, 1)), -7.0, order="F"), np.full((max(ns, 1), k), -7.0, order="F"),
            np.full((n, k), -7.0, order="F")]


def _call_all(num, n, ns, k=2):
    """Status of every numeric entry point with host arrays filled with -7, and the arrays."""
    L = sc.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    D, G, X = _outputs(n, ns, k)
    S = D.copy(order="F")
    B = np.ones((n, k), order="F")
    XS = np.ones((max(ns, 1), k), order="F")
    ld = max(ns, 1)
    rcs = [L.sc_schur_factor_host(num.h, p(D), ld), L.sc_schur_matrix_host(num.h, p(S), ld),
           L.sc_schur_condense_host_multi(num.h, k, p(B), n, p(G), ld),
           L.sc_schur_expand_host_multi(num.h, k, p(B), n, p(XS), ld, p(X), n)]
    return rcs, (D, S, G, X)


def test_before_factorization_is_a_state_error(gpu):
    A, idx, _ = _input("bcsstk01_td1")
    num = _fresh("bcsstk01_td1", factor=False)
    rcs, outs = _call_all(num, A.size(), len(idx))
    assert rcs == [SC_ERR_STATE] * 4
    assert all(np.all(o == -7.0) for o in outs)


@pytest.mark.parametrize("case", ["bcsstk01_td1", "bcsstk01_td0"])
def test_not_positive_definite_returns_the_status(gpu, case):
    A, idx, _ = _input(case)
    x = A.x.copy()
    j = 20
    assert A.i[A.p[j + 1] - 1] == j
    x[A.p[j + 1] - 1] = -1.0
    num = _fresh(case, factor=False)
    st = num.factor(x)
    assert st > 0
    rcs, outs = _call_all(num, A.size(), len(idx))
    assert rcs == [st] * 4
    assert all(np.all(o == -7.0) for o in outs)
    with pytest.raises(sc.LibraryError):
        num.schur_complement()
    assert num.factor(A.x) == 0  # the handle recovers
    assert _fro(num.schur_complement(), _refs(case)[0]) < _refs(case)[1]


def test_handle_without_a_schur_set(gpu):
    A = cases.load("bcsstk01")
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A, schur=[]))
    assert num.factor(A.x) == 0
    rcs, (D, S, G, X) = _call_all(num, n, 0)
    assert rcs == [0] * 4
    assert np.all(D == -7.0) and np.all(S == -7.0) and np.all(G == -7.0)
    # with nothing to prescribe, the expansion is the solve
    assert np.linalg.norm(X - num.solve(np.ones((n, 2)))) <= 1e-12 * np.linalg.norm(X)
    assert num.schur_complement().shape == (0, 0)


def test_emulated_two_rank_handle_is_not_implemented(gpu):
    A, idx, _ = _input("lap12_two_planes")
    num = sc.Numeric(sc.Symbolic(A, schur=idx), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    rcs, outs = _call_all(num, A.size(), len(idx))
    assert rcs == [SC_ERR_NOTIMPL] * 4
    assert b"single-device" in sc.lib().sc_last_error()
    assert all(np.all(o == -7.0) for o in outs)


@pytest.mark.parametrize("case", ["bus130_nd", "lap16_nd_plane"])
def test_memory_growth(gpu, case):
    A, idx, _ = _input(case)
    n, ns = A.size(), len(idx)
    num = _fresh(case)
    num.solve(np.ones((n, 2)))      # the solves' plan and panel buffers
    num.apply_P(np.ones((n, 2)))    # the operators' postorder
    m0 = num.memory()["total"]
    num.schur_factor()
    m1 = num.memory()["total"]
    # the header's account: D, and 12 bytes per Schur index
    print(f"SCHUR {case}: first use +{m1 - m0} bytes (8 ns^2 = {8 * ns * ns})")
    assert 8 * ns * ns <= m1 - m0 <= 8 * ns * ns + 12 * ns
    num.schur_complement()
    num.schur_factor()
    assert num.memory()["total"] == m1
    B = np.ones((n, 3))
    XS = np.linalg.solve(num.schur_complement(), num.schur_condense(B))
    m2 = num.memory()["total"]
    assert m2 - m1 == 128 * n  # the n x 16 panel of the partial solves
    num.schur_expand(B, XS)
    num.schur_condense(B)
    assert num.factor(A.x) == 0
    num.schur_complement()
    assert num.memory()["total"] == m2
