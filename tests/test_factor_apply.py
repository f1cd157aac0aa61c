"""Factor operators on the GPU (sc_apply_*, sc_logdet): L^-1 b, L^-T b, L z, L^T z, P b,
P^T b and log det A from the factor P A P^T = L L^T, against the oracle's L through scipy.
L is the matrix sc_export_L returns, in its numbering (the order of P A P^T)."""
import ctypes
import functools
import math

import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc
from test_solve_multi import _matrix, _rhs, _sym_full  # the inputs and their caches, shared

pytestmark = pytest.mark.gpu

L_OPS = [sc.SC_OP_SOLVE_L, sc.SC_OP_SOLVE_LT, sc.SC_OP_MUL_L, sc.SC_OP_MUL_LT]
ALL_OPS = [sc.SC_OP_SOLVE_A] + L_OPS + [sc.SC_OP_PERM, sc.SC_OP_PERM_T]
OP_NAME = {sc.SC_OP_SOLVE_A: "solve_A", sc.SC_OP_SOLVE_L: "solve_L", sc.SC_OP_SOLVE_LT: "solve_Lt",
           sc.SC_OP_MUL_L: "mul_L", sc.SC_OP_MUL_LT: "mul_Lt", sc.SC_OP_PERM: "P", sc.SC_OP_PERM_T: "Pt"}

INPUTS = [("lap20", {}), ("lap24", {}), ("lap12", dict(small_front_max=0)), ("bcsstk01", dict(tiny_dense=0)),
          ("bcsstk01", dict(tiny_dense=1)), ("1138_bus", {}), ("random", {})]
INPUT_IDS = ["lap20", "lap24", "lap12_allfronts", "bcsstk01_td0", "bcsstk01_td1", "1138_bus", "random"]


def _key(kw):
    return tuple(sorted(kw.items()))


_handles = {}


def _numeric(name, **kw):
    """One factored handle per (input, options), shared by the tests that only apply."""
    key = (name, _key(kw))
    if key not in _handles:
        A = _matrix(name)
        num = sc.Numeric(sc.Symbolic(A, **kw))
        assert num.factor(A.x) == 0
        _handles[key] = num
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _oracle(name, ordering=0):
    """(full symmetric A, |A|_inf, perm, L, L^T, diag L): the oracle's factor of P A P^T,
    computed once per input and ordering."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import norm as spnorm

    A = _matrix(name)
    n = A.size()
    perm = sc.Symbolic(A, ordering=ordering).perm().astype(np.int64) if ordering else np.arange(n)
    st, Lp, Li, Lx = oracle.chol(sc.permute_symmetric(A, perm) if ordering else A)
    assert st == 0
    L = sp.csc_matrix((Lx, Li, Lp), shape=(n, n)).tocsr()
    Af = _sym_full(A)
    return Af, spnorm(Af, np.inf), perm, L, L.T.tocsr(), L.diagonal()


def _reference(name, op, Z, ordering=0):
    from scipy.sparse.linalg import spsolve_triangular

    _, _, _, L, Lt, _ = _oracle(name, ordering)
    if op == sc.SC_OP_SOLVE_L:
        return spsolve_triangular(L, Z, lower=True)
    if op == sc.SC_OP_SOLVE_LT:
        return spsolve_triangular(Lt, Z, lower=False)
    return (L if op == sc.SC_OP_MUL_L else Lt) @ Z


def _check_rel(what, X, Xo, bar):
    """Per column: relative 2-norm error below bar."""
    X, Xo = np.atleast_2d(X.T).T, np.atleast_2d(Xo.T).T
    assert X.shape == Xo.shape
    for j in range(Xo.shape[1]):
        err = np.linalg.norm(X[:, j] - Xo[:, j]) / np.linalg.norm(Xo[:, j])
        print(f"{what} column {j}: rel err {err:.3e}")
        assert err < bar, (what, j, err)


# ---- 1. oracle parity ----
@pytest.mark.parametrize("name,kw", INPUTS, ids=INPUT_IDS)
def test_ops_vs_oracle_16_and_1d(gpu, name, kw):
    num = _numeric(name, **kw)
    Z = _rhs(name, 16, seed=11)
    for op in L_OPS:
        _check_rel(f"{name} {OP_NAME[op]}", num.apply(Z, op), _reference(name, op, Z), 1e-10)
        z = Z[:, 3].copy()
        x = num.apply(z, op)
        assert x.shape == z.shape
        _check_rel(f"{name} {OP_NAME[op]} 1-D", x, _reference(name, op, z), 1e-10)


@pytest.mark.parametrize("k", [1, 3, 17, 40])
def test_ops_vs_oracle_panels_lap20(gpu, k):
    # a partial panel, full + partial, several panels
    num = _numeric("lap20")
    Z = _rhs("lap20", k, seed=12)
    for op in L_OPS:
        X = num.apply(Z, op)
        assert X.shape == Z.shape
        _check_rel(f"lap20 k={k} {OP_NAME[op]}", X, _reference("lap20", op, Z), 1e-10)


@pytest.mark.parametrize("ordering", [1, 2], ids=["nd", "amd"])
def test_ops_vs_oracle_with_ordering_1138(gpu, ordering):
    # L is the factor of P A P^T: the oracle factors permute_symmetric(A, perm)
    name = "1138_bus"
    num = _numeric(name, ordering=ordering)
    perm = _oracle(name, ordering)[2]
    assert np.array_equal(perm, num.symb.perm())
    Z = _rhs(name, 5, seed=13)
    for op in L_OPS:
        _check_rel(f"{name} {OP_NAME[op]}", num.apply(Z, op), _reference(name, op, Z, ordering), 1e-10)
    assert np.array_equal(num.apply_P(Z), Z[perm])
    back = np.empty_like(Z)
    back[perm] = Z
    assert np.array_equal(num.apply_Pt(Z), back)
    assert np.array_equal(num.apply_P(Z[:, 0].copy()), Z[perm, 0])
    assert np.array_equal(num.apply_Pt(Z[:, 0].copy()), back[:, 0])


# ---- 2. the product against A ----
@pytest.mark.parametrize("name,kw", INPUTS + [("1138_bus", dict(ordering=1)), ("1138_bus", dict(ordering=2)),
                                              ("lap16nat", dict(ordering=1))],
                         ids=INPUT_IDS + ["1138_bus_nd", "1138_bus_amd", "lap16nat_nd"])
def test_product_equals_A(gpu, name, kw):
    # A = P^T L L^T P from the factor alone
    num = _numeric(name, **kw)
    A = _matrix(name)
    Af = _sym_full(A)
    anorm = abs(Af).sum(axis=1).max()
    Z = _rhs(name, 16, seed=14)
    X = num.apply_Pt(num.mul_L(num.mul_Lt(num.apply_P(Z))))
    R = X - Af @ Z
    for j in range(Z.shape[1]):
        err = np.abs(R[:, j]).max() / (anorm * np.abs(Z[:, j]).max())
        print(f"{name} column {j}: |P^T L L^T P z - A z|_inf / (|A|_inf |z|_inf) = {err:.3e}")
        assert err < 1e-14, (name, j, err)


# ---- 3. composition, bitwise ----
@pytest.mark.parametrize("ordering", [0, 1, 2], ids=["natural", "nd", "amd"])
@pytest.mark.parametrize("name", ["1138_bus", "lap16nat"])
def test_half_solves_compose_to_the_solve_bitwise(gpu, name, ordering):
    num = _numeric(name, ordering=ordering)
    B = _rhs(name, 16, seed=15)
    for b in (B[:, 0].copy(), B, B[:, :5]):  # the single-vector family, a full and a partial panel
        x = num.apply_Pt(num.solve_Lt(num.solve_L(num.apply_P(b))))
        assert np.array_equal(x, num.solve(b))
        assert np.array_equal(num.apply(b, sc.SC_OP_SOLVE_A), num.solve(b))


# ---- 4. round trips ----
@pytest.mark.parametrize("name", ["lap20", "random"])
def test_round_trips(gpu, name):
    num = _numeric(name)
    Z = _rhs(name, 16, seed=16)
    _check_rel(f"{name} solve_L(mul_L)", num.solve_L(num.mul_L(Z)), Z, 1e-10)
    _check_rel(f"{name} solve_Lt(mul_Lt)", num.solve_Lt(num.mul_Lt(Z)), Z, 1e-10)


def test_quadratic_form_lap20(gpu):
    # b^T A^-1 b = |L^-1 P b|^2
    num = _numeric("lap20")
    b = _rhs("lap20", 1, seed=17)[:, 0].copy()
    y = num.solve_L(num.apply_P(b))
    q, ref = float(y @ y), float(b @ num.solve(b))
    print(f"quadratic form: {q!r} against {ref!r}, rel {abs(q - ref) / abs(ref):.3e}")
    assert abs(q - ref) / abs(ref) < 1e-12


# ---- 5. the stored inverses ----
@pytest.mark.parametrize("name,kw", [("lap20", {}), ("lap12", dict(small_front_max=0)), ("1138_bus", {})],
                         ids=["lap20", "lap12_allfronts", "1138_bus"])
def test_products_do_not_see_the_stored_inverses(gpu, name, kw):
    A = _matrix(name)
    num = sc.Numeric(sc.Symbolic(A, **kw))  # fresh: no solve has stored an inverse yet
    assert num.factor(A.x) == 0
    Z = _rhs(name, 16, seed=18)
    z = Z[:, 0].copy()
    first = [num.mul_L(Z), num.mul_Lt(Z), num.mul_L(z), num.mul_Lt(z)]
    _check_rel(f"{name} mul_L before any solve", first[0], _reference(name, sc.SC_OP_MUL_L, Z), 1e-10)
    _check_rel(f"{name} mul_Lt before any solve", first[1], _reference(name, sc.SC_OP_MUL_LT, Z), 1e-10)
    for solve_arg in (z, Z):  # a single solve, then a multi solve: the inverses are in place
        num.solve(solve_arg)
        again = [num.mul_L(Z), num.mul_Lt(Z), num.mul_L(z), num.mul_Lt(z)]
        for a, f in zip(again, first):
            assert np.array_equal(a, f)


# ---- 6. determinism and column independence ----
def test_ops_bitwise_repeatable_lap20(gpu):
    A = _matrix("lap20")
    Z = _rhs("lap20", 16, seed=19)
    # the plain solves run between the operators on the same handle: every op and family
    # replays a captured sweep of its own
    calls = {OP_NAME[op]: (lambda num, op=op: num.apply(Z, op)) for op in L_OPS}
    calls["solve(b)"] = lambda num: num.solve(Z[:, 0].copy())
    calls["solve(B)"] = lambda num: num.solve(Z)
    runs = {name: [] for name in calls}
    for rep in range(2):
        num = sc.Numeric(sc.Symbolic(A))
        assert num.factor(A.x) == 0
        for name, call in calls.items():
            runs[name].append(call(num))
            runs[name].append(call(num))
        assert num.factor(A.x) == 0
        for name, call in calls.items():
            runs[name].append(call(num))
        if rep == 1:
            assert sc.lib().sc_debug_solve_eager(num.h, 1) == 0
            for name, call in calls.items():
                runs[name].append(call(num))
    for name in calls:
        assert len(runs[name]) == 7
        for x in runs[name][1:]:
            assert np.array_equal(runs[name][0], x), name


@pytest.mark.parametrize("name", ["lap20", "1138_bus"])
def test_ops_column_independence_bitwise(gpu, name):
    num = _numeric(name)
    Z = _rhs(name, 16, seed=20)
    perm = np.random.default_rng(21).permutation(16)
    sel = [2, 9, 11]
    rep = np.arange(40) % 16
    for op in L_OPS:
        X = num.apply(Z, op)
        assert np.array_equal(num.apply(Z[:, perm], op), X[:, perm]), OP_NAME[op]
        assert np.array_equal(num.apply(Z[:, sel], op), X[:, sel]), OP_NAME[op]
        assert np.array_equal(num.apply(Z[:, rep], op), X[:, rep]), OP_NAME[op]
        assert np.array_equal(num.apply(Z[:, [7]], op), X[:, [7]]), OP_NAME[op]
    # the products have panel kernels only: a vector is a panel of one column
    z = Z[:, 4].copy()
    assert np.array_equal(num.mul_L(z), num.mul_L(z[:, None])[:, 0])
    assert np.array_equal(num.mul_Lt(z), num.mul_Lt(z[:, None])[:, 0])


# ---- 7. leading dimensions and aliasing (device entry points, torch tensors) ----
def _dev(torch, a):
    """(n, k) host array -> column-major device buffer (a (k, ld) torch tensor)."""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda:0")


@pytest.mark.parametrize("op", [sc.SC_OP_MUL_L, sc.SC_OP_SOLVE_LT], ids=["mul_L", "solve_Lt"])
def test_device_leading_dimensions_and_aliasing(gpu, op):
    torch = pytest.importorskip("torch")
    name, k = "lap20", 16
    num = _numeric(name)
    n = _matrix(name).size()
    B = _rhs(name, k, seed=22)
    ref = num.apply(B, op)
    _check_rel(f"{name} {OP_NAME[op]}", ref, _reference(name, op, B), 1e-10)
    ld = n + 7
    SENT = -7.25
    Bp = np.full((ld, k), SENT)
    Bp[:n] = B
    # ldb = ldx = n + 7, out of place: the 7 trailing rows of every X column stay the sentinel
    dB, dX = _dev(torch, Bp), _dev(torch, np.full((ld, k), SENT))
    torch.cuda.synchronize()
    assert num.apply_device_multi(op, dB.data_ptr(), k, ld, dX.data_ptr(), ld) == 0
    Xh = dX.cpu().numpy().T
    assert np.array_equal(Xh[n:], np.full((7, k), SENT))
    assert np.array_equal(Xh[:n], ref)
    assert np.array_equal(dB.cpu().numpy().T, Bp)  # B is read only
    # in place
    assert num.apply_device_multi(op, dB.data_ptr(), k, ld, dB.data_ptr(), ld) == 0
    Xh = dB.cpu().numpy().T
    assert np.array_equal(Xh[n:], np.full((7, k), SENT))
    assert np.array_equal(Xh[:n], ref)
    # ldb != ldx, out of place
    dB, dX = _dev(torch, Bp), _dev(torch, np.full((n, k), SENT))
    torch.cuda.synchronize()
    assert num.apply_device_multi(op, dB.data_ptr(), k, ld, dX.data_ptr(), n) == 0
    assert np.array_equal(dX.cpu().numpy().T, ref)
    # the single-vector device entry point, out of place and in place
    db, dx = _dev(torch, B[:, :1]), _dev(torch, np.full((n, 1), SENT))
    torch.cuda.synchronize()
    assert num.apply_device(op, db.data_ptr(), dx.data_ptr()) == 0
    x1 = dx.cpu().numpy()[0]
    assert np.array_equal(x1, num.apply(B[:, 0].copy(), op))
    assert np.array_equal(db.cpu().numpy()[0], B[:, 0])
    assert num.apply_device(op, db.data_ptr(), db.data_ptr()) == 0
    assert np.array_equal(db.cpu().numpy()[0], x1)
    # argument errors: nothing is computed
    dB = _dev(torch, Bp)
    torch.cuda.synchronize()
    with pytest.raises(sc.LibraryError, match="sc_factor_op"):
        num.apply_device_multi(7, dB.data_ptr(), k, ld, dX.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="sc_factor_op"):
        num.apply_device(-1, db.data_ptr(), dx.data_ptr())
    with pytest.raises(sc.LibraryError, match="leading dimension"):
        num.apply_device_multi(op, dB.data_ptr(), k, n - 1, dX.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="alias"):
        num.apply_device_multi(op, dB.data_ptr(), k, ld, dB.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="null"):
        num.apply_device_multi(op, 0, k, ld, dX.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="null"):
        num.apply_device(op, db.data_ptr(), 0)
    assert np.array_equal(dX.cpu().numpy().T, ref)
    assert np.array_equal(dB.cpu().numpy().T, Bp)


# ---- 8. the log-determinant ----
def _logdet_ref(name, ordering=0):
    d = _oracle(name, ordering)[5]
    return 2.0 * math.fsum(np.log(d)), 2.0 * math.fsum(np.abs(np.log(d)))


@pytest.mark.parametrize("name,kw", INPUTS + [("1138_bus", dict(ordering=2))], ids=INPUT_IDS + ["1138_bus_amd"])
def test_logdet_vs_oracle(gpu, name, kw):
    A = _matrix(name)
    num = _numeric(name, **kw)
    ref, scale = _logdet_ref(name, kw.get("ordering", 0))
    ld = num.logdet()
    print(f"{name}: logdet {ld!r} against {ref!r}, error / (2 sum |log L_jj|) = {abs(ld - ref) / scale:.3e}")
    assert abs(ld - ref) / scale < 1e-12
    assert num.logdet() == ld
    other = sc.Numeric(sc.Symbolic(A, **kw))
    assert other.factor(A.x) == 0
    assert other.logdet() == ld  # before any solve on this handle, too


@pytest.mark.parametrize("name", ["lap20", "bcsstk01"])
def test_logdet_and_solve_L_after_refactoring_with_2A(gpu, name):
    A = _matrix(name)
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    Z = _rhs(name, 16, seed=23)
    ld1, Y1 = num.logdet(), num.solve_L(Z)
    assert num.factor(2.0 * A.x) == 0
    ld2, Y2 = num.logdet(), num.solve_L(Z)
    _, scale = _logdet_ref(name)
    grow = n * math.log(2.0)
    print(f"{name}: logdet grew by {ld2 - ld1!r}, n log 2 = {grow!r}")
    assert abs((ld2 - ld1) - grow) / scale < 1e-12
    _check_rel(f"{name} solve_L of 2 A", Y2, Y1 / math.sqrt(2.0), 1e-12)


# ---- 9. state ----
def _vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_ops_after_failed_factor(gpu):
    A = sc.laplacian3d(6)
    A.x[A.p[5]:A.p[6]][-1] = -10.0  # diagonal of column 5
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(A.x)
    assert st > 0
    n = A.size()
    L = sc.lib()
    for op in ALL_OPS:
        B = np.ones((n, 3), order="F")
        X = np.full((n, 3), 4.5, order="F")
        assert L.sc_apply_host_multi(num.h, op, 3, _vp(B), n, _vp(X), n) == st, OP_NAME[op]
        assert np.array_equal(X, np.full((n, 3), 4.5))
        b, x = np.ones(n), np.full(n, 4.5)
        assert L.sc_apply_host(num.h, op, _vp(b), _vp(x)) == st, OP_NAME[op]
        assert np.array_equal(x, np.full(n, 4.5))
        with pytest.raises(sc.LibraryError, match="not positive definite"):
            num.apply(np.ones((n, 3)), op)
    v = ctypes.c_double(4.5)
    assert L.sc_logdet(num.h, ctypes.byref(v)) == st
    assert v.value == 4.5
    with pytest.raises(sc.LibraryError, match="not positive definite"):
        num.logdet()


def test_ops_nothing_to_do_and_call_order(gpu):
    num = _numeric("bcsstk01", tiny_dense=1)
    n = _matrix("bcsstk01").size()
    L = sc.lib()
    E = sc.csc_matrix(0, 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    ne = sc.Numeric(sc.Symbolic(E))
    assert ne.factor(E.x) == 0
    fresh = sc.Numeric(sc.Symbolic(_matrix("bcsstk01")))  # not factored
    buf = np.zeros(4)
    b = np.zeros((n, 1), order="F")
    for op in ALL_OPS:
        assert L.sc_apply_host_multi(num.h, op, 0, None, n, None, n) == 0
        assert L.sc_apply_device_multi(num.h, op, 0, None, n, None, n) == 0
        assert num.apply(np.zeros((n, 0)), op).shape == (n, 0)
        assert L.sc_apply_host_multi(ne.h, op, 3, _vp(buf), 0, _vp(buf), 0) == 0
        assert L.sc_apply_host(ne.h, op, _vp(buf), _vp(buf)) == 0
        assert ne.apply(np.zeros((0, 3)), op).shape == (0, 3)
        assert L.sc_apply_host_multi(fresh.h, op, 1, _vp(b), n, _vp(b), n) == -5, OP_NAME[op]
        assert L.sc_apply_host(fresh.h, op, _vp(b), _vp(b)) == -5, OP_NAME[op]
    assert ne.logdet() == 0.0
    v = ctypes.c_double(4.5)
    assert L.sc_logdet(fresh.h, ctypes.byref(v)) == -5 and v.value == 4.5


# ---- 10. emulated multi-rank ----
def test_ops_emulated_two_ranks(gpu):
    A = _matrix("lap20")
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    ref, scale = _logdet_ref("lap20")
    ld = num.logdet()
    print(f"two ranks: logdet error {abs(ld - ref) / scale:.3e}")
    assert abs(ld - ref) / scale < 1e-12
    Z = _rhs("lap20", 16, seed=24)
    for op in (sc.SC_OP_SOLVE_L, sc.SC_OP_MUL_L):
        _check_rel(f"two ranks {OP_NAME[op]}", num.apply(Z, op), _reference("lap20", op, Z), 1e-10)


# ---- 11. memory ----
@pytest.mark.parametrize("ordering", [0, 2], ids=["natural", "amd"])
def test_ops_need_no_new_buffers(gpu, ordering):
    name = "lap16nat"
    A = _matrix(name)
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A, ordering=ordering))
    assert num.factor(A.x) == 0
    Z = _rhs(name, 16, seed=25)
    num.solve(Z[:, 0].copy())
    num.solve(Z)
    mem0 = num.memory()["total"]
    for op in ALL_OPS:
        num.apply(Z, op)
        num.apply(Z[:, 0].copy(), op)
    num.logdet()
    grew = num.memory()["total"] - mem0
    print(f"{name} ordering {ordering}: memory grew by {grew} bytes, 8 n = {8 * n}")
    assert grew < 8 * n
