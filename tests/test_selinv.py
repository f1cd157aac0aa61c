"""Selected inversion on the GPU (sc_selinv*): the entries of Z = (P A P^T)^-1 on the pattern
of L, against dense inverses on the CPU.

Reference: np.linalg.inv of the full symmetric P A P^T.  Tolerance per input: a second CPU
inverse (dense Cholesky, a triangular solve of the identity, X^T X) is compared with the
first in the same metric, and the bar is max(1e-12, 100 x that disagreement): the factor 100
covers a third backward-stable algorithm with another summation order and stays far below an
indexing error, which shows as O(1).  Metrics: normwise max |Z - Z_ref| over the exported
entries / max |Z_ref| over them; for the diagonal also entrywise relative."""
import ctypes
import functools

import numpy as np
import pytest

import sparsecholesky_amd as sc
from test_solve_multi import _matrix, _sym_full  # the inputs and their caches, shared

pytestmark = pytest.mark.gpu

SC_ERR_STATE, SC_ERR_NOTIMPL = -5, -7


def _dense_spd(n, seed):
    """The dense SPD generator of tests/test_gpu_parity.py."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    D = M @ M.T + n * np.eye(n)
    iu = np.triu_indices(n)
    return sc.triplet_to_csc_matrix(iu[0], iu[1], D[iu], n)


@functools.lru_cache(maxsize=None)
def _input(name):
    if name.startswith("dense"):
        return _dense_spd(int(name[5:]), 3)
    return _matrix(name)


# case id -> (input, analysis options)
CASES = {
    "bcsstk01_td0": ("bcsstk01", dict(tiny_dense=0)),  # n = 48, every w < 64; both tiny paths feed the same panels
    "bcsstk01_td1": ("bcsstk01", dict(tiny_dense=1)),
    "1138_bus": ("1138_bus", {}),                      # many small fronts and chains
    "1138_bus_nd": ("1138_bus", dict(ordering=1)),     # the permutation in diag and in the export numbering
    "1138_bus_amd": ("1138_bus", dict(ordering=2)),
    "random": ("random", {}),
    "lap16": ("lap16", {}),                            # root w = 256 = two full blocks, mb = 0; children w = 128
    "lap12_allfronts": ("lap12", dict(small_front_max=0)),  # root w = 144 = 128 + a 16-column partial block
    "dense700": ("dense700", {}),                      # one front, 5 full blocks + 60 columns; R never a tile multiple
    "dense100": ("dense100", {}),                      # 64 < w < 128: the off-diagonal inverse quadrant
}


def _key(kw):
    return tuple(sorted(kw.items()))


_handles = {}


def _numeric(case):
    """One factored handle per case, shared by the tests that only read."""
    if case not in _handles:
        name, kw = CASES[case]
        A = _input(name)
        num = sc.Numeric(sc.Symbolic(A, **kw))
        assert num.factor(A.x) == 0
        _handles[case] = num
    return _handles[case]


def _fresh(case, scale=1.0):
    name, kw = CASES[case]
    A = _input(name)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x * scale) == 0
    return num


@functools.lru_cache(maxsize=None)
def _refs(name, ordering):
    """(perm, Z_ref, Z_ref2) of P A P^T, computed once per input and ordering and left unchanged."""
    import scipy.linalg as sla

    A = _input(name)
    n = A.size()
    perm = sc.Symbolic(A, ordering=ordering).perm().astype(np.int64) if ordering else np.arange(n)
    D = sc.csc_to_dense(sc.permute_symmetric(A, perm) if ordering else A)
    D = np.triu(D) + np.triu(D, 1).T
    Z1 = np.linalg.inv(D)
    X = sla.solve_triangular(np.linalg.cholesky(D), np.eye(n), lower=True)
    Z2 = X.T @ X
    Z1.setflags(write=False)
    Z2.setflags(write=False)
    return perm, Z1, Z2


def _pattern_cols(Lp):
    return np.repeat(np.arange(len(Lp) - 1), np.diff(Lp))


def _bars(case, Lp, Li):
    name, kw = CASES[case]
    perm, Z1, Z2 = _refs(name, kw.get("ordering", 0))
    rows, cols = Li.astype(np.int64), _pattern_cols(Lp)
    zr, zr2 = Z1[rows, cols], Z2[rows, cols]
    d_nw = np.abs(zr - zr2).max() / np.abs(zr).max()
    d_dg = (np.abs(np.diag(Z1) - np.diag(Z2)) / np.abs(np.diag(Z1))).max()
    return perm, Z1, zr, max(1e-12, 100 * d_nw), max(1e-12, 100 * d_dg), d_nw, d_dg


# ---- 1. parity with the dense inverse ----
@pytest.mark.parametrize("case", list(CASES))
def test_selected_inverse_vs_dense(gpu, case):
    num = _numeric(case)
    assert num.selinv() == 0
    Lp, Li, Zx = num.selected_inverse()
    d = num.inverse_diagonal()
    n = num.symb.n
    # the export's pattern and numbering are those of the factor's export
    st, L = num.export()
    assert st == 0 and np.array_equal(Lp, L.p) and np.array_equal(Li, L.i)
    perm, Z1, zr, bar_nw, bar_dg, d_nw, d_dg = _bars(case, Lp, Li)
    assert np.array_equal(perm, num.symb.perm())
    # Z[i, j] taken from column j against e_i^T Z_ref e_j: every exported entry
    err_nw = np.abs(Zx - zr).max() / np.abs(zr).max()
    # diag is in A's own order: d[perm[k]] = Z[k, k], the first entry of column k, bitwise
    assert np.array_equal(Li[Lp[:-1]], np.arange(n))
    assert np.array_equal(d[perm], Zx[Lp[:-1]])
    dref = np.diag(Z1)
    err_dg = (np.abs(d[perm] - dref) / np.abs(dref)).max()
    print(f"{case}: normwise {err_nw:.3e} (bar {bar_nw:.3e}, references differ {d_nw:.3e}); "
          f"diagonal entrywise {err_dg:.3e} (bar {bar_dg:.3e}, references differ {d_dg:.3e})")
    assert err_nw < bar_nw, (case, err_nw, bar_nw)
    assert err_dg < bar_dg, (case, err_dg, bar_dg)


@pytest.mark.parametrize("case", list(CASES))
def test_trace_of_A_times_Z(gpu, case):
    # tr(A Z) = n needs only the entries of Z on the pattern of A, all of which lie on L's
    import scipy.sparse as sp

    num = _numeric(case)
    name, kw = CASES[case]
    A = _input(name)
    n = A.size()
    perm = num.symb.perm().astype(np.int64)
    B = _sym_full(sc.permute_symmetric(A, perm) if kw.get("ordering", 0) else A)
    Lp, Li, Zx = num.selected_inverse()
    Zl = sp.csc_matrix((Zx, Li, Lp), shape=(n, n))
    Zs = (Zl + sp.tril(Zl, -1).T).tocsr()
    Pl = sp.csc_matrix((np.ones(len(Li)), Li, Lp), shape=(n, n))
    Bl = sp.tril(B).tocsc()
    assert Bl.multiply(Pl).nnz == Bl.nnz  # every entry of A lies on the pattern
    tr = B.multiply(Zs).sum()
    print(f"{case}: tr(A Z) - n = {tr - n:.3e}")
    assert abs(tr - n) <= 1e-10 * n


# ---- 2. a factor too large for a dense inverse ----
def test_lap24_columns_vs_splu(gpu):
    # second-level separators with w = 288 (three blocks) and mb > 0: Z_RR spans the Z
    # panel and Z_II.  Reference: sparse LU columns A^-1 e_j, compared on the pattern of
    # column j; bar 1e-10, the bar of the other operator tests on Laplacians.
    from scipy.sparse.linalg import splu

    A = _matrix("lap24")
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    Lp, Li, Zx = num.selected_inverse()
    sn = num.symb.supernodes()
    _, post = num.symb.etree()
    root = int(np.flatnonzero(sn["parent"] < 0)[-1])
    seps = [s for s in range(len(sn["m"])) if sn["w"][s] == 288 and sn["m"][s] > sn["w"][s]]
    assert seps, "no separator with w = 288 and a contribution block"
    cols = []
    for s in (root, seps[0]):
        c0, w = int(sn["start"][s]), int(sn["w"][s])
        cols += [int(post[c0 + min(k0 + 5, w - 1)]) for k0 in range(0, w, 128)]
    cols += np.random.default_rng(24).integers(0, n, 32).tolist()
    lu = splu(_sym_full(A).tocsc())
    worst = 0.0
    for j in cols:
        e = np.zeros(n)
        e[j] = 1.0
        x = lu.solve(e)
        rows = Li[Lp[j]:Lp[j + 1]]
        err = np.abs(Zx[Lp[j]:Lp[j + 1]] - x[rows]).max() / np.abs(x[rows]).max()
        worst = max(worst, err)
        assert err < 1e-10, (j, err)
    d = num.inverse_diagonal()
    assert np.array_equal(d, Zx[Lp[:-1]])  # no fill-reducing permutation: A's order is the export's
    print(f"lap24: {len(cols)} columns, worst normwise error on a column's pattern {worst:.3e}")


# ---- 3. bitwise repeatability ----
@pytest.mark.parametrize("case", ["1138_bus_nd", "lap12_allfronts", "dense700"])
def test_bitwise_repeatable(gpu, case):
    name, kw = CASES[case]
    A = _input(name)
    num = _fresh(case)
    Z1 = num.selected_inverse()[2]
    d1 = num.inverse_diagonal()
    assert num.selinv() == 0  # a second call
    assert np.array_equal(num.selected_inverse()[2], Z1)
    other = _fresh(case)  # a second handle
    assert np.array_equal(other.selected_inverse()[2], Z1)
    assert np.array_equal(other.inverse_diagonal(), d1)
    assert num.factor(A.x) == 0  # the same values again
    assert np.array_equal(num.selected_inverse()[2], Z1)
    # 2 A: an accessor before any explicit recomputation is not served the stale result
    assert num.factor(2.0 * A.x) == 0
    d2 = num.inverse_diagonal()
    Lp, Li, Z2 = num.selected_inverse()
    _, _, zr, bar_nw, bar_dg, _, _ = _bars(case, Lp, Li)
    err = np.abs(Z2 - 0.5 * zr).max() / np.abs(0.5 * zr).max()
    print(f"{case}: Z(2A) against Z_ref / 2: normwise {err:.3e} (bar {bar_nw:.3e})")
    assert err < bar_nw
    assert (np.abs(d2 - 0.5 * d1) / np.abs(0.5 * d1)).max() < max(bar_dg, 1e-12)


# ---- 4. non-interference ----
ALL_OPS = [sc.SC_OP_SOLVE_A, sc.SC_OP_SOLVE_L, sc.SC_OP_SOLVE_LT, sc.SC_OP_MUL_L, sc.SC_OP_MUL_LT, sc.SC_OP_PERM,
           sc.SC_OP_PERM_T]


@pytest.mark.parametrize("case", ["1138_bus_nd", "lap12_allfronts"])
def test_solves_and_operators_keep_their_bits(gpu, case):
    num = _fresh(case)
    n = num.symb.n
    rng = np.random.default_rng(7)
    b, B = rng.standard_normal(n), rng.standard_normal((n, 5))

    def snapshot():
        out = [num.solve(b), num.solve(B), np.float64(num.logdet())]
        for op in ALL_OPS:
            out += [num.apply(b, op), num.apply(B, op)]
        return out

    before = snapshot()
    Z = num.selected_inverse()[2]
    after = snapshot()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    # a fresh handle (no stored inverses yet) gives the bits of one that has already solved
    fresh = _fresh(case)
    assert np.array_equal(fresh.selected_inverse()[2], Z)


@pytest.mark.parametrize("case", ["lap12_allfronts", "lap16", "1138_bus"])
def test_factorization_after_selinv_reuses_the_work_arena(gpu, case):
    name, kw = CASES[case]
    A = _input(name)
    st, L0 = _fresh(case).export()
    num = _fresh(case)
    assert num.selinv() == 0
    assert num.factor(A.x) == 0
    st, L1 = num.export()
    assert st == 0 and np.array_equal(L1.x, L0.x)


# ---- 5. state, status and memory ----
def test_before_factorization_is_a_state_error(gpu):
    A = _input("bcsstk01")
    num = sc.Numeric(sc.Symbolic(A))
    L = sc.lib()
    d = np.full(A.size(), -7.0)
    assert L.sc_selinv(num.h) == SC_ERR_STATE
    assert L.sc_selinv_diag_host(num.h, d.ctypes.data_as(ctypes.c_void_p)) == SC_ERR_STATE
    assert L.sc_selinv_export(num.h, None, None, None) == SC_ERR_STATE
    assert np.all(d == -7.0)


@pytest.mark.parametrize("tiny", [0, 1])
def test_not_positive_definite_returns_the_status(gpu, tiny):
    A = _input("bcsstk01")
    n = A.size()
    x = A.x.copy()
    j = 20
    x[A.p[j + 1] - 1] = -1.0  # the diagonal of column j (upper CSC: last entry of the column)
    assert A.i[A.p[j + 1] - 1] == j
    num = sc.Numeric(sc.Symbolic(A, tiny_dense=tiny))
    st = num.factor(x)
    assert st > 0
    L = sc.lib()
    d = np.full(n, -7.0)
    Zx = np.full(num.symb.nnz_L, -7.0)
    assert L.sc_selinv(num.h) == st
    assert L.sc_selinv_diag_host(num.h, d.ctypes.data_as(ctypes.c_void_p)) == st
    assert L.sc_selinv_export(num.h, None, None, Zx.ctypes.data_as(ctypes.c_void_p)) == st
    assert np.all(d == -7.0) and np.all(Zx == -7.0)
    # the handle recovers with a positive definite matrix
    assert num.factor(A.x) == 0
    assert num.selinv() == 0


def test_emulated_two_rank_handle_is_not_implemented(gpu):
    A = _matrix("lap12")
    num = sc.Numeric(sc.Symbolic(A), nranks=2, virtual=True)
    assert num.factor(A.x) == 0
    L = sc.lib()
    assert L.sc_selinv(num.h) == SC_ERR_NOTIMPL
    assert b"single-device" in L.sc_last_error()
    d = np.full(A.size(), -7.0)
    assert L.sc_selinv_diag_host(num.h, d.ctypes.data_as(ctypes.c_void_p)) == SC_ERR_NOTIMPL
    assert np.all(d == -7.0)
    with pytest.raises(sc.LibraryError):
        num.selinv()


def _documented_scratch_bytes(symb):
    """The header's account of what the first call allocates besides the Z panel: the W
    scratch (8 bytes x the largest sum of nr nb over the blocks of one step), the partials of
    the Z_KK products deeper than 512 (32 KiB per 256-deep chunk and 64 x 64 tile, the largest
    sum over one step) and the task lists (16 bytes per block, 8 per 64-row tile of a block's
    rows below, 16 per Z_KK tile and chunk plus 16 per tile that is cut, 16 per 64 x 64 tile
    of a contribution block)."""
    sn = symb.supernodes()
    w, m, par, lev = (sn[k].astype(np.int64) for k in ("w", "m", "parent", "level"))
    lists, wmax, smax = 0, 1, 1
    for L in range(int(lev.max()) + 1):
        fr = np.flatnonzero(lev == L)
        for k0 in range(0, int(w[fr].max()), 128):
            act = fr[w[fr] > k0]
            nb = np.minimum(128, w[act] - k0)
            nr = m[act] - k0 - nb
            tiles = np.where(nb > 64, 3, 1)
            nch = np.where(nb + nr <= 512, 1, (nb + nr + 255) // 256)
            cut = nch > 1
            wmax = max(wmax, int((nr * nb).sum()))
            smax = max(smax, int((tiles * nch * cut).sum()))
            lists += int(16 * len(act) + 8 * ((nr + 63) // 64).sum() + 16 * (tiles * nch).sum() + 16 * (tiles * cut).sum())
    mb = (m - w)[par >= 0]
    lists += int(16 * (((mb + 63) // 64) ** 2).sum())
    return 8 * wmax + 32768 * smax + lists + 5 * 16  # an empty list still takes one element


@pytest.mark.parametrize("case", ["lap16", "1138_bus_nd"])
def test_memory_growth(gpu, case):
    num = _fresh(case)
    num.solve(np.ones(num.symb.n))  # the solves' plan is not the selected inversion's
    m0 = num.memory()
    assert num.selinv() == 0
    m1 = num.memory()
    grow = m1["total"] - m0["total"]
    bound = m0["panel"] + _documented_scratch_bytes(num.symb)
    print(f"{case}: first call +{grow} bytes (Z panel {m0['panel']}, bound {bound})")
    assert m0["panel"] <= grow <= bound
    assert num.selinv() == 0
    num.inverse_diagonal()
    num.selected_inverse()
    assert num.memory()["total"] == m1["total"]
