"""Panel solves on the GPU: nrhs right-hand sides through sc_solve_host_multi /
sc_solve_device_multi (16-column fp64 MFMA panels), against triangular solves with the
oracle's L, per column, with the single-vector solve's tolerances."""
import ctypes
import functools
import os

import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def random_spd(n, density, seed):
    """Random sparse SPD (diagonally dominant) upper CSC, as tests/test_gpu_parity.py builds it."""
    rng = np.random.default_rng(seed)
    nnz = max(1, int(density * n * n / 2))
    i = rng.integers(0, n, nnz)
    j = rng.integers(0, n, nnz)
    v = rng.uniform(-1, 1, nnz)
    ti = np.concatenate([i, np.arange(n)])
    tj = np.concatenate([j, np.arange(n)])
    deg = np.zeros(n)
    np.add.at(deg, i, np.abs(v))
    np.add.at(deg, j, np.abs(v))
    tx = np.concatenate([v, deg + 1.0 + rng.uniform(0, 1, n)])
    return sc.triplet_to_csc_matrix(ti, tj, tx, n)


def _sym_full(A):
    import scipy.sparse as sp

    U = sp.csc_matrix((A.x, A.i, A.p), shape=(A.size(), A.size()))
    U = sp.triu(U)
    return (U + sp.triu(U, 1).T).tocsr()


@functools.lru_cache(maxsize=None)
def _matrix(name):
    if name.startswith("lap") and name.endswith("nat"):
        return sc.laplacian3d(int(name[3:-3]), nd=False)
    if name.startswith("lap"):
        return sc.laplacian3d(int(name[3:]))
    if name == "random":
        return random_spd(500, 0.02, 5)
    return sc.load_matrix_market_to_csc(os.path.join(GOLDEN, name + ".mtx"))


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(full symmetric A, |A|_inf, L, L^T) of the oracle, computed once per input."""
    import scipy.sparse as sp
    from scipy.sparse.linalg import norm as spnorm

    A = _matrix(name)
    st, Lp, Li, Lx = oracle.chol(A)
    assert st == 0
    L = sp.csc_matrix((Lx, Li, Lp), shape=(A.size(), A.size())).tocsr()
    Af = _sym_full(A)
    return Af, spnorm(Af, np.inf), L, L.T.tocsr()


def _oracle_solve(name, B):
    from scipy.sparse.linalg import spsolve_triangular

    _, _, L, Lt = _oracle(name)
    Y = spsolve_triangular(L, B, lower=True)
    return spsolve_triangular(Lt, Y, lower=False)


def _check_columns(name, X, B):
    """Per column: relative 2-norm error against the oracle < 1e-10, normwise backward
    error |Ax - b|_inf / (|A|_inf |x|_inf + |b|_inf) < 1e-14."""
    assert X.shape == B.shape
    Af, anorm, _, _ = _oracle(name)
    Xo = _oracle_solve(name, B)
    R = Af @ X - B
    for j in range(B.shape[1]):
        err = np.linalg.norm(X[:, j] - Xo[:, j]) / np.linalg.norm(Xo[:, j])
        be = np.abs(R[:, j]).max() / (anorm * np.abs(X[:, j]).max() + np.abs(B[:, j]).max())
        print(f"{name} column {j}: rel err {err:.3e} backward err {be:.3e}")
        assert err < 1e-10, (name, j, err)
        assert be < 1e-14, (name, j, be)


_handles = {}


def _numeric(name, **kw):
    """One factored handle per (input, options), shared by the tests that only solve."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _handles:
        A = _matrix(name)
        num = sc.Numeric(sc.Symbolic(A, **kw))
        assert num.factor(A.x) == 0
        _handles[key] = num
    return _handles[key]


def _rhs(name, k, seed=1):
    return np.random.default_rng(seed).standard_normal((_matrix(name).size(), k))


# ---- 1. oracle parity ----
@pytest.mark.parametrize("name,kw", [("lap20", {}), ("lap24", {}), ("lap12", dict(small_front_max=0)),
                                     ("bcsstk01", dict(tiny_dense=0)), ("bcsstk01", dict(tiny_dense=1)),
                                     ("1138_bus", {}), ("random", {})],
                         ids=["lap20", "lap24", "lap12_allfronts", "bcsstk01_td0", "bcsstk01_td1", "1138_bus",
                              "random"])
def test_multi_vs_oracle_16(gpu, name, kw):
    B = _rhs(name, 16)
    X = _numeric(name, **kw).solve(B)
    _check_columns(name, X, B)


@pytest.mark.parametrize("k", [1, 3, 17, 40])
def test_multi_vs_oracle_panels_lap20(gpu, k):
    # a partial panel, full + partial, several panels
    B = _rhs("lap20", k, seed=2)
    X = _numeric("lap20").solve(B)
    assert X.shape == (B.shape[0], k)
    _check_columns("lap20", X, B)


def test_multi_accepts_any_memory_order(gpu):
    B = _rhs("random", 5, seed=3)
    num = _numeric("random")
    Xc = num.solve(np.ascontiguousarray(B))
    Xf = num.solve(np.asfortranarray(B))
    wide = np.zeros((B.shape[0], 10))
    wide[:, ::2] = B
    Xs = num.solve(wide[:, ::2])  # a strided view
    assert Xc.shape == B.shape
    assert np.array_equal(Xc, Xf) and np.array_equal(Xc, Xs)


# ---- 2. leading dimensions and aliasing (device entry point, torch tensors) ----
def _dev(torch, a):
    """(n, k) host array -> column-major device buffer (a (k, ld) torch tensor)."""
    return torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda:0")


def test_device_multi_leading_dimensions_and_aliasing(gpu):
    torch = pytest.importorskip("torch")
    name, k = "lap20", 16
    num = _numeric(name)
    n = _matrix(name).size()
    B = _rhs(name, k, seed=4)
    ref = num.solve(B)
    ld = n + 7
    SENT = -7.25
    Bp = np.full((ld, k), SENT)
    Bp[:n] = B
    # ldb = ldx = n + 7, out of place: the 7 trailing rows of every X column stay the sentinel
    dB, dX = _dev(torch, Bp), _dev(torch, np.full((ld, k), SENT))
    torch.cuda.synchronize()
    assert num.solve_device_multi(dB.data_ptr(), k, ld, dX.data_ptr(), ld) == 0
    Xh = dX.cpu().numpy().T
    assert np.array_equal(Xh[n:], np.full((7, k), SENT))
    assert np.array_equal(Xh[:n], ref)
    assert np.array_equal(dB.cpu().numpy().T, Bp)  # B is read only
    # in place
    assert num.solve_device_multi(dB.data_ptr(), k, ld, dB.data_ptr(), ld) == 0
    Xh = dB.cpu().numpy().T
    assert np.array_equal(Xh[n:], np.full((7, k), SENT))
    assert np.array_equal(Xh[:n], ref)
    # ldb != ldx, out of place
    dB, dX = _dev(torch, Bp), _dev(torch, np.full((n, k), SENT))
    torch.cuda.synchronize()
    assert num.solve_device_multi(dB.data_ptr(), k, ld, dX.data_ptr(), n) == 0
    assert np.array_equal(dX.cpu().numpy().T, ref)
    _check_columns(name, ref, B)
    # aliasing with ldx != ldb, and short leading dimensions, are argument errors
    with pytest.raises(sc.LibraryError, match="alias"):
        num.solve_device_multi(dB.data_ptr(), k, ld, dB.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="leading dimension"):
        num.solve_device_multi(dB.data_ptr(), k, n - 1, dX.data_ptr(), n)
    with pytest.raises(sc.LibraryError):
        num.solve_device_multi(dB.data_ptr(), -1, ld, dX.data_ptr(), n)
    with pytest.raises(sc.LibraryError, match="null"):
        num.solve_device_multi(0, k, ld, dX.data_ptr(), n)


# ---- 3. column independence, bitwise ----
@pytest.mark.parametrize("name", ["lap20", "1138_bus"])
def test_column_independence_bitwise(gpu, name):
    num = _numeric(name)
    B = _rhs(name, 16, seed=5)
    X = num.solve(B)
    perm = np.random.default_rng(6).permutation(16)
    assert np.array_equal(num.solve(B[:, perm]), X[:, perm])
    sel = [2, 9, 11]
    assert np.array_equal(num.solve(B[:, sel]), X[:, sel])
    rep = np.arange(40) % 16
    assert np.array_equal(num.solve(B[:, rep]), X[:, rep])
    assert np.array_equal(num.solve(B[:, [7]]), X[:, [7]])


# ---- 4. repeatability, bitwise ----
def test_multi_bitwise_repeatable_lap24(gpu):
    A = _matrix("lap24")
    B = _rhs("lap24", 16, seed=7)
    xs = []
    for rep in range(2):
        num = sc.Numeric(sc.Symbolic(A))
        assert num.factor(A.x) == 0
        xs.append(num.solve(B))
        xs.append(num.solve(B))
        assert num.factor(A.x) == 0
        xs.append(num.solve(B))
        if rep == 1:
            assert sc.lib().sc_debug_solve_eager(num.h, 1) == 0
            xs.append(num.solve(B))
    for x in xs[1:]:
        assert np.array_equal(xs[0], x)


# ---- 5. against the single-vector path ----
def test_multi_vs_single_vector_lap20(gpu):
    A = _matrix("lap20")
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    B = _rhs("lap20", 16, seed=8)
    before = [num.solve(B[:, j].copy()) for j in (0, 5)]
    mem0 = num.memory()["total"]
    X = num.solve(B)
    n = A.size()
    # the panel buffers are counted: at least 3 n 16 doubles more than before
    assert num.memory()["total"] - mem0 >= 3 * n * 16 * 8
    for j in range(16):
        xj = num.solve(B[:, j].copy())
        assert np.linalg.norm(X[:, j] - xj) / np.linalg.norm(xj) < 1e-10
    # the single solve's bits are those from before the first multi solve
    assert np.array_equal(num.solve(B[:, 0].copy()), before[0])
    assert np.array_equal(num.solve(B[:, 5].copy()), before[1])
    assert np.array_equal(num.solve(B), X)


# ---- 6. orderings ----
@pytest.mark.parametrize("ordering", [1, 2], ids=["nd", "amd"])
@pytest.mark.parametrize("name", ["1138_bus", "lap16nat"])
def test_multi_with_fill_reducing_ordering(gpu, name, ordering):
    # the factor is of P A P^T; solves take and return A's order
    B = _rhs(name, 5, seed=9)
    X = _numeric(name, ordering=ordering).solve(B)
    _check_columns(name, X, B)


# ---- 7. emulated multi-rank ----
def test_multi_emulated_two_ranks(gpu):
    A = _matrix("lap20")
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    B = _rhs("lap20", 16, seed=10)
    _check_columns("lap20", num.solve(B), B)


# ---- 8. not positive definite ----
def test_multi_after_failed_factor(gpu):
    A = sc.laplacian3d(6)
    A.x[A.p[5]:A.p[6]][-1] = -10.0  # diagonal of column 5
    num = sc.Numeric(sc.Symbolic(A))
    st = num.factor(A.x)
    assert st > 0
    n = A.size()
    with pytest.raises(sc.LibraryError, match="not positive definite"):
        num.solve(np.ones((n, 3)))
    B = np.ones((n, 3), order="F")
    X = np.full((n, 3), 4.5, order="F")
    rc = sc.lib().sc_solve_host_multi(num.h, 3, B.ctypes.data_as(ctypes.c_void_p), n,
                                      X.ctypes.data_as(ctypes.c_void_p), n)
    assert rc == st
    assert np.array_equal(X, np.full((n, 3), 4.5))


# ---- 9. nothing to do ----
def test_multi_nrhs_zero_and_empty_matrix(gpu):
    num = _numeric("bcsstk01", tiny_dense=1)
    n = _matrix("bcsstk01").size()
    L = sc.lib()
    assert L.sc_solve_host_multi(num.h, 0, None, n, None, n) == 0
    assert L.sc_solve_device_multi(num.h, 0, None, n, None, n) == 0
    X = num.solve(np.zeros((n, 0)))
    assert X.shape == (n, 0)
    E = sc.csc_matrix(0, 0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    ne = sc.Numeric(sc.Symbolic(E))
    assert ne.factor(E.x) == 0
    buf = np.zeros(4)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert L.sc_solve_host_multi(ne.h, 3, p, 0, p, 0) == 0
    assert ne.solve(np.zeros((0, 3))).shape == (0, 3)
    # before a factorization: call out of order
    fresh = sc.Numeric(sc.Symbolic(_matrix("bcsstk01")))
    b = np.zeros((n, 1), order="F")
    assert L.sc_solve_host_multi(fresh.h, 1, b.ctypes.data_as(ctypes.c_void_p), n,
                                 b.ctypes.data_as(ctypes.c_void_p), n) == -5
