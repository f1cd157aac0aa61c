"""Rank-k update and downdate of the factor on the GPU (sc_updown_host) against the CPU.

References, for D = P A P^T made full symmetric and V = P W: np.linalg.cholesky(D + s V V^T),
and the textbook column-by-column rank-1 loop applied to np.linalg.cholesky(D), one column of
V after the other.  Metric: relative Frobenius error over the exported entries of L.  Bar:
max(1e-12, 100 x the disagreement of the two references in the same metric) -- the rule of
tests/test_selinv.py; 1e-12 is the project's parity bar for L, the factor 100 covers a third
stable algorithm, an indexing error shows as O(1).

W: per column a first row j0 from a seeded generator (the prescribed trees: first columns of
fronts spread over the branches and the trees), then a random subset of the true pattern of
L(:, j0) that holds j0, standard-normal values.  For downdates W is scaled on the CPU so that
the largest eigenvalue of V^T D^-1 V is 1/2: A - W W^T stays safely positive definite."""
import ctypes
import functools

import numpy as np
import pytest

import sparsecholesky_amd as sc
import zoo
from test_selinv import _input

pytestmark = pytest.mark.gpu

SC_ERR_STATE, SC_ERR_NOTIMPL = -5, -7

# case id -> (input, analysis options)
CASES = {
    "bcsstk01_td0": ("bcsstk01", dict(tiny_dense=0)),  # n = 48: every block partial
    "bcsstk01_td1": ("bcsstk01", dict(tiny_dense=1)),
    "1138_bus": ("1138_bus", {}),                      # relaxed supernodes (relaxed-zero positions), long paths
    "1138_bus_nd": ("1138_bus", dict(ordering=1)),     # the permutation
    "1138_bus_amd": ("1138_bus", dict(ordering=2)),
    "lap12_allfronts": ("lap12", dict(small_front_max=0)),  # root w = 144 = 64 + 64 + 16
    "lap16": ("lap16", {}),                            # root w = 256
    "dense100": ("dense100", {}),                      # one front, 64 < w < 128
    "dense700": ("dense700", {}),                      # 10 full blocks + 60 columns; rows below never a tile multiple
}
ZOO = ("forest", "star300_large_root", "fanin300_mid_cb", "chain300_edges")
for _z in ZOO:
    for _tag in ("relax0", "default"):
        CASES[f"{_z}-{_tag}"] = ("zoo:" + _z, zoo.OPTS[_tag])
KS = (1, 3, 16, 17)


def _matrix_of(case):
    name, kw = CASES[case]
    return (zoo.case(name[4:]).A if name.startswith("zoo:") else _input(name)), kw


@functools.lru_cache(maxsize=None)
def _setup(case):
    """(symbolic, perm, D = full symmetric P A P^T, cholesky(D), (Lp, Li)), computed once."""
    A, kw = _matrix_of(case)
    symb = sc.Symbolic(A, **kw)
    perm = symb.perm().astype(np.int64)
    D = sc.csc_to_dense(sc.permute_symmetric(A, perm) if kw.get("ordering", 0) else A)
    D = np.triu(D) + np.triu(D, 1).T
    L0 = np.linalg.cholesky(D)
    for a in (D, L0):
        a.setflags(write=False)
    return symb, perm, D, L0, symb.pattern()


def _fresh(case):
    A, _ = _matrix_of(case)
    num = sc.Numeric(_setup(case)[0])
    assert num.factor(A.x) == 0
    return num


def _first_rows(case, k, rng):
    symb, _, _, _, (Lp, _) = _setup(case)
    n = symb.n
    name = CASES[case][0]
    if name.startswith("zoo:"):
        # first columns of fronts spread evenly over the spec: different leaves (branches),
        # different trees of the forest, the roots among them
        st = zoo.case(name[4:]).st
        fr = np.unique(np.linspace(0, len(st.w) - 1, k).astype(np.int64))
        j0 = st.start[fr]
        extra = rng.integers(0, n, k - len(j0))
        return np.concatenate([j0, extra]).astype(np.int64)
    return rng.integers(0, n, k)


@functools.lru_cache(maxsize=None)
def _W(case, k, seed=0):
    """(V dense in the order of P A P^T, W = (Wp, Wi, Wx) in A's own numbering, scale of the
    safe downdate)."""
    symb, perm, D, L0, (Lp, Li) = _setup(case)
    n = symb.n
    rng = np.random.default_rng(1000 * seed + 17 * k + len(case))
    V = np.zeros((n, k))
    Wp, Wi, Wx = [0], [], []
    for c, j0 in enumerate(_first_rows(case, k, rng)):
        col = Li[Lp[j0]:Lp[j0 + 1]].astype(np.int64)
        assert col[0] == j0
        rows = np.concatenate([[j0], col[1:][rng.random(len(col) - 1) < 0.5]])
        vals = rng.standard_normal(len(rows))
        V[rows, c] = vals
        order = rng.permutation(len(rows))  # rows of a column in no particular order
        Wi += perm[rows[order]].tolist()
        Wx += vals[order].tolist()
        Wp.append(len(Wi))
    import scipy.linalg as sla

    Y = sla.solve_triangular(L0, V, lower=True)
    lam = np.linalg.eigvalsh(Y.T @ Y).max()
    V.setflags(write=False)
    W = (np.array(Wp, dtype=np.int64), np.array(Wi, dtype=np.int32), np.array(Wx))
    return V, W, float(np.sqrt(0.5 / lam))


def _scaled(W, a):
    return (W[0], W[1], a * W[2])


def _rank1_loop(L, x, sign):
    """The textbook rank-1 update / downdate of a dense lower factor, column by column."""
    n = len(x)
    x = x.copy()
    for k in range(n):
        if x[k] == 0.0:
            continue
        r = np.sqrt(L[k, k] ** 2 + sign * x[k] ** 2)
        c, s = r / L[k, k], x[k] / L[k, k]
        L[k, k] = r
        if k + 1 < n:
            L[k + 1:, k] = (L[k + 1:, k] + sign * s * x[k + 1:]) / c
            x[k + 1:] = c * x[k + 1:] - s * L[k + 1:, k]


@functools.lru_cache(maxsize=None)
def _refs(case, k, sign):
    """(reference values on the exported pattern, bar, disagreement of the two references)."""
    symb, perm, D, L0, (Lp, Li) = _setup(case)
    V, _, a = _W(case, k)
    Vs = V if sign > 0 else a * V
    R1 = np.linalg.cholesky(D + sign * Vs @ Vs.T)
    R2 = L0.copy()
    for c in range(k):
        _rank1_loop(R2, Vs[:, c], sign)
    rows, cols = Li.astype(np.int64), np.repeat(np.arange(symb.n), np.diff(Lp))
    r1, r2 = R1[rows, cols], R2[rows, cols]
    dis = np.linalg.norm(r1 - r2) / np.linalg.norm(r1)
    r1.setflags(write=False)
    return r1, max(1e-12, 100 * dis), dis


def _rel(x, ref):
    return float(np.linalg.norm(x - ref) / np.linalg.norm(ref))


# ---- 1 and 2: parity with the references; an update undone by its downdate ----
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", list(CASES))
def test_update_and_downdate_vs_cpu(gpu, case, k):
    A, _ = _matrix_of(case)
    V, W, a = _W(case, k)
    num = _fresh(case)
    st, L0 = num.export()
    ld0 = num.logdet()
    # the update
    ref, bar, dis = _refs(case, k, 1)
    assert num.update(W) == 0
    st, L1 = num.export()
    assert st == 0 and np.array_equal(L1.p, L0.p) and np.array_equal(L1.i, L0.i)
    err_up = _rel(L1.x, ref)
    # undone by the downdate of the same W
    assert num.downdate(W) == 0
    st, L2 = num.export()
    err_back = _rel(L2.x, L0.x)
    ld2 = num.logdet()
    # the downdate of the safely scaled W, from the original factor
    assert num.factor(A.x) == 0
    refd, bard, disd = _refs(case, k, -1)
    assert num.updown(_scaled(W, a), -1) == 0
    st, L3 = num.export()
    err_dn = _rel(L3.x, refd)
    print(f"UPDOWN {case} k={k}: update {err_up:.3e} (bar {bar:.3e}, references differ {dis:.3e}); downdate "
          f"{err_dn:.3e} (bar {bard:.3e}, references differ {disd:.3e}); update then downdate {err_back:.3e}; "
          f"logdet back to {abs(ld2 - ld0) / abs(ld0):.3e} relative")
    assert err_up < bar, (case, k, err_up, bar)
    assert err_dn < bard, (case, k, err_dn, bard)
    assert err_back < bar, (case, k, err_back, bar)
    assert abs(ld2 - ld0) <= 1e-12 * abs(ld0)


# ---- 3: everything that reads the factor describes A + W W^T ----
@pytest.mark.parametrize("case", list(CASES))
def test_readers_after_an_update(gpu, case):
    import scipy.linalg as sla

    k = 17
    A, kw = _matrix_of(case)
    symb, perm, D, L0, _ = _setup(case)
    n = symb.n
    V, W, _ = _W(case, k)
    rng = np.random.default_rng(3)
    b = rng.standard_normal(n)
    num = _fresh(case)
    # the stored block inverses and the Z panel exist before the update: both must be rebuilt
    num.solve(b)
    num.inverse_diagonal()
    assert num.update(W) == 0
    # A' in A's own numbering
    Vo = np.zeros_like(V)
    Vo[perm] = V
    Ad = sc.csc_to_dense(A)
    Ad = np.triu(Ad) + np.triu(Ad, 1).T + Vo @ Vo.T
    Dp = D + V @ V.T

    def backward(x):
        return float(np.linalg.norm(Ad @ x - b, np.inf) /
                     (np.linalg.norm(Ad, np.inf) * np.linalg.norm(x, np.inf) + np.linalg.norm(b, np.inf)))

    # solve: against the freshly factored A' on the same kind of handle
    iu = np.nonzero(np.triu(Ad))
    A2 = sc.triplet_to_csc_matrix(iu[0], iu[1], Ad[iu], n)
    fresh = sc.Numeric(sc.Symbolic(A2, **kw))
    assert fresh.factor(A2.x) == 0
    e_fresh, e_upd = backward(fresh.solve(b)), backward(num.solve(b))
    # logdet(A') = logdet(A) + logdet(I + V^T D^-1 V)
    Y = sla.solve_triangular(L0, V, lower=True)
    ld_ref = 2 * np.log(np.diag(L0)).sum() + np.linalg.slogdet(np.eye(k) + Y.T @ Y)[1]
    ld = num.logdet()
    # diag(A'^-1), test_selinv's bar: two CPU inverses, entrywise relative on the diagonal
    Z1 = np.linalg.inv(Dp)
    X = sla.solve_triangular(np.linalg.cholesky(Dp), np.eye(n), lower=True)
    d1, d2 = np.diag(Z1), np.einsum("ij,ij->j", X, X)
    dis = float((np.abs(d1 - d2) / np.abs(d1)).max())
    bar_dg = max(1e-12, 100 * dis)
    d = num.inverse_diagonal()
    err_dg = float((np.abs(d[perm] - d1) / np.abs(d1)).max())
    # L^-1 then L
    back = num.mul_L(num.solve_L(b))
    err_ll = float(np.linalg.norm(back - b) / np.linalg.norm(b))
    print(f"UPDOWN readers {case}: solve backward error {e_upd:.3e} (fresh factorization of A' {e_fresh:.3e}); "
          f"logdet {abs(ld - ld_ref) / abs(ld_ref):.3e} relative; inverse diagonal {err_dg:.3e} (bar {bar_dg:.3e}, "
          f"references differ {dis:.3e}); mul_L(solve_L(b)) {err_ll:.3e}")
    assert e_upd <= 10 * e_fresh, (e_upd, e_fresh)
    assert abs(ld - ld_ref) <= 1e-12 * abs(ld_ref)
    assert err_dg < bar_dg
    assert err_ll < 1e-10


# ---- 4: bitwise ----
BITWISE = ["bcsstk01_td1", "1138_bus_nd", "lap12_allfronts", "dense700", "forest-relax0", "star300_large_root-default"]


@pytest.mark.parametrize("sign", [1, -1], ids=["update", "downdate"])
@pytest.mark.parametrize("case", BITWISE)
def test_bitwise_repeatable(gpu, case, sign):
    A, _ = _matrix_of(case)
    _, W, a = _W(case, 17)
    Ws = W if sign > 0 else _scaled(W, a)
    one, two = _fresh(case), _fresh(case)
    assert one.updown(Ws, sign) == 0 and two.updown(Ws, sign) == 0
    x1 = one.export()[1].x
    assert np.array_equal(two.export()[1].x.view(np.int64), x1.view(np.int64))
    assert one.factor(A.x) == 0 and one.updown(Ws, sign) == 0  # after a refactorization
    assert np.array_equal(one.export()[1].x.view(np.int64), x1.view(np.int64))


@pytest.mark.parametrize("case", BITWISE)
def test_one_call_equals_its_chunks(gpu, case):
    _, (Wp, Wi, Wx), _ = _W(case, 33)

    def cols(c0, c1):
        p0, p1 = int(Wp[c0]), int(Wp[c1])
        return (Wp[c0:c1 + 1] - p0, Wi[p0:p1], Wx[p0:p1])

    whole, parts = _fresh(case), _fresh(case)
    assert whole.update((Wp, Wi, Wx)) == 0
    for c0, c1 in ((0, 16), (16, 32), (32, 33)):
        assert parts.update(cols(c0, c1)) == 0
    assert np.array_equal(whole.export()[1].x.view(np.int64), parts.export()[1].x.view(np.int64))


# ---- 5: a later factorization forgets the update ----
@pytest.mark.parametrize("case", ["bcsstk01_td0", "bcsstk01_td1", "1138_bus", "lap12_allfronts", "lap16"])
def test_factor_after_update_forgets_it(gpu, case):
    A, _ = _matrix_of(case)
    x0 = _fresh(case).export()[1].x
    num = _fresh(case)
    assert num.update(_W(case, 3)[1]) == 0
    assert not np.array_equal(num.export()[1].x, x0)
    assert num.factor(A.x) == 0
    assert np.array_equal(num.export()[1].x.view(np.int64), x0.view(np.int64))


# ---- 6: a downdate that leaves the matrix not positive definite ----
@pytest.mark.parametrize("case", ["bcsstk01_td0", "bcsstk01_td1", "1138_bus_nd", "lap12_allfronts", "forest-relax0"])
def test_failing_downdate(gpu, case):
    A, _ = _matrix_of(case)
    symb, perm = _setup(case)[:2]
    n = symb.n
    num = _fresh(case)
    st, L = num.export()
    lnn = L.x[-1]  # the last column of P A P^T holds its diagonal alone
    assert L.p[n] - L.p[n - 1] == 1
    # W = alpha e_last, alpha^2 = 2 L(n, n)^2: the new squared diagonal is -L(n, n)^2, and no
    # other pivot is touched
    W = (np.array([0, 1], dtype=np.int64), np.array([perm[n - 1]], dtype=np.int32), np.array([np.sqrt(2.0) * lnn]))
    assert num.downdate(W) == n
    assert num.status() == n
    lib = sc.lib()
    b = np.ones(n)
    x = np.full(n, -7.0)
    assert lib.sc_solve_host(num.h, b.ctypes.data_as(ctypes.c_void_p), x.ctypes.data_as(ctypes.c_void_p)) == n
    assert np.all(x == -7.0)
    v = ctypes.c_double(-7.0)
    assert lib.sc_logdet(num.h, ctypes.byref(v)) == n and v.value == -7.0
    assert num.updown(W, 1) == n  # and no further sweep either
    # a refactorization clears it
    assert num.factor(A.x) == 0 and num.status() == 0
    assert np.array_equal(num.export()[1].x.view(np.int64), L.x.view(np.int64))
    num.solve(b)


# ---- 7: handle state ----
def test_emulated_two_rank_handle_is_not_implemented(gpu):
    A = _input("lap12")
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    x0 = num.export()[1].x
    lib = sc.lib()
    Wp, Wi, Wx = np.array([0, 1], dtype=np.int64), np.array([5], dtype=np.int32), np.array([1.0])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for sign in (1, -1):
        assert lib.sc_updown_host(num.h, sign, 1, p(Wp), p(Wi), p(Wx)) == SC_ERR_NOTIMPL
        assert b"single-device" in lib.sc_last_error()
    assert np.array_equal(num.export()[1].x.view(np.int64), x0.view(np.int64))
    with pytest.raises(sc.LibraryError):
        num.update((Wp, Wi, Wx))


def test_state_and_argument_errors_on_a_handle(gpu):
    A = _input("bcsstk01")
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A))
    lib = sc.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    Wp, Wi, Wx = np.array([0, 1], dtype=np.int64), np.array([5], dtype=np.int32), np.array([1.0])
    assert lib.sc_updown_host(num.h, 1, 1, p(Wp), p(Wi), p(Wx)) == SC_ERR_STATE  # before a factorization
    # a failed factorization: its status, nothing computed
    x = A.x.copy()
    j = 20
    x[A.p[j + 1] - 1] = -1.0
    st = num.factor(x)
    assert st > 0
    assert lib.sc_updown_host(num.h, 1, 1, p(Wp), p(Wi), p(Wx)) == st
    assert num.factor(A.x) == 0
    x0 = num.export()[1].x
    # argument errors name the entry point and leave the factor alone
    assert lib.sc_updown_host(num.h, 2, 1, p(Wp), p(Wi), p(Wx)) == -1
    assert lib.sc_last_error() == b"sc_updown_host: sign must be +1 (update) or -1 (downdate)"
    assert lib.sc_updown_host(num.h, 1, -1, p(Wp), p(Wi), p(Wx)) == -1
    assert lib.sc_last_error() == b"sc_updown_host: k < 0"
    assert lib.sc_updown_host(num.h, 1, 1, p(Wp), p(Wi), None) == -1
    assert lib.sc_last_error() == b"sc_updown_host: null Wx"
    assert lib.sc_updown_host(num.h, 1, 1, p(Wp), p(np.array([n], dtype=np.int32)), p(Wx)) == -1
    assert lib.sc_last_error().startswith(b"sc_updown_host: column 0 of W")
    # an inadmissible column: row 0 and a row outside the pattern of L(:, 0)
    Lp, Li = num.symb.pattern()
    outside = np.setdiff1d(np.arange(n), Li[Lp[0]:Lp[1]])
    assert len(outside)
    bad = (np.array([0, 2], dtype=np.int64), np.array([0, outside[-1]], dtype=np.int32), np.ones(2))
    with pytest.raises(sc.LibraryError, match="column 0 of W is not admissible"):
        num.update(bad)
    # k == 0 and an empty column are no-ops
    assert lib.sc_updown_host(num.h, 1, 0, None, None, None) == 0
    assert num.update((np.array([0, 0], dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))) == 0
    assert np.array_equal(num.export()[1].x.view(np.int64), x0.view(np.int64))
    # an explicit zero is a pattern entry: the sweep runs and changes nothing but signs of zero
    assert num.update((Wp, Wi, np.zeros(1))) == 0
    assert np.array_equal(num.export()[1].x, x0)


# ---- 8: memory ----
@pytest.mark.parametrize("case", ["lap16", "1138_bus_nd"])
def test_memory_grows_once(gpu, case):
    num = _fresh(case)
    n = num.symb.n
    _, W, _ = _W(case, 3)
    m0 = num.memory()["total"]
    assert num.update(W) == 0
    m1 = num.memory()["total"]
    assert m1 - m0 >= 128 * n  # at least the n x 16 workspace
    assert num.downdate(W) == 0
    assert num.update(_W(case, 17)[1]) == 0
    assert num.memory()["total"] == m1
