"""Every operation of the library on the prescribed-tree catalogue (tests/zoo.py) against
long-double references, front by front: factor, solves, the factor operators, logdet, the
selected inversion, bitwise repeatability, exact scaling by powers of four, the status of
not positive definite inputs (one and two failing pivots) and emulated ranks.

The per-front bar.  For every front of the spec (its column range, whatever the amalgamation
did) the relative Frobenius error of the GPU's L against the long-double factor must be at
most 16 E, where E is the oracle's worst per-front error on the same case and value mode,
measured on the CPU in the same run (2e-16 to 1e-15 here).  The bar follows the reference,
not the code under test; 16 = four bits for another summation order (MFMA blocks and tree
reductions against the oracle's sequential sums: both are bounded by K eps sum |terms| and sit
near sqrt(K) eps; the argument does not depend on K, and E is measured at the same K: the
catalogue's fronts go up to K = 530 columns and 713 rows, the big_ cases of tests/zoo.py).

The big_ cases bring the large-front kernel instances under this bar: the 128-tile and lean
CB SYRK with the fused extend-add gather on irregular child maps, the 128-tile panel update,
the lookahead-stream instances, the tiled assembly and the 256-row TRSM workgroups
(tests/test_zoo_cpu.py asserts on the host schedule which case and tag reaches which)."""
import functools
import math

import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc
import zoo

pytestmark = pytest.mark.gpu

MARGIN = 16.0
L_OPS = [sc.SC_OP_SOLVE_A, sc.SC_OP_SOLVE_L, sc.SC_OP_SOLVE_LT, sc.SC_OP_MUL_L, sc.SC_OP_MUL_LT]
OP_NAME = {sc.SC_OP_SOLVE_A: "solve_A", sc.SC_OP_SOLVE_L: "solve_L", sc.SC_OP_SOLVE_LT: "solve_Lt",
           sc.SC_OP_MUL_L: "mul_L", sc.SC_OP_MUL_LT: "mul_Lt"}

# analysis options by tag, and the tags each case runs under: tests/zoo.py (shared with the host tests)
OPTS = zoo.OPTS
_tags = zoo.tags


CONFIGS = [(n, t) for n in zoo.NAMES for t in _tags(n)]
BASIC = [(n, t) for n in zoo.NAMES for t in ("relax0", "default")]
_ids = lambda cfgs: [f"{n}-{t}" for n, t in cfgs]  # noqa: E731

_handles = {}


def _numeric(name, tag, mode="llt"):
    """One factored handle per (case, options, value mode), shared by the tests that only read.
    The big_ cases run under eight tags and hold a few MB each: their handles are kept for one
    case at a time (pytest runs a parametrized test case by case), the small cases' for good."""
    key = (name, tag, mode)
    if key not in _handles:
        if name in zoo.BIG_FRONTS:
            for k in [k for k in _handles if k[0] in zoo.BIG_FRONTS and k[0] != name]:
                del _handles[k]
        A = zoo.case(name, mode).A
        num = sc.Numeric(sc.Symbolic(A, **OPTS[tag]))
        assert num.factor(A.x) == 0
        _handles[key] = num
    return _handles[key]


def _fresh(name, tag, mode="llt", scale=1.0, **kw):
    A = zoo.case(name, mode).A
    num = sc.Numeric(sc.Symbolic(A, **dict(OPTS[tag], **kw)))
    assert num.factor(A.x * scale) == 0
    return num


@functools.lru_cache(maxsize=None)
def _oracle(name, mode):
    """(Lx, E): the oracle's factor and its worst per-front error against long double."""
    c = zoo.case(name, mode)
    st, Lp, Li, Lx = oracle.chol(c.A)
    assert st == 0 and np.array_equal(Lp, c.ref.Lp) and np.array_equal(Li, c.ref.Li)
    Lx.setflags(write=False)
    return Lx, float(c.ref.front_errors(Lx).max())


def _check_factor(what, name, mode, L):
    """Pattern, the project's whole-factor bar against the oracle, the per-front bar against
    long double.  Prints the worst ratio err / E and where it sits."""
    c = zoo.case(name, mode)
    ref = c.ref
    Lx, E = _oracle(name, mode)
    assert np.array_equal(L.p, ref.Lp) and np.array_equal(L.i, ref.Li)
    whole = np.linalg.norm(L.x - Lx) / np.linalg.norm(Lx)
    e = ref.front_errors(L.x)
    f = int(e.argmax())
    print(f"ZOO {what} {name} {mode}: n={c.n} fronts={len(e)} E={E:.3e} worst front err={e[f]:.3e} "
          f"ratio={e[f] / E:.2f} (front {f}: w={c.st.w[f]} m={c.st.m[f]}) whole-factor vs oracle={whole:.3e}")
    assert whole < 1e-12
    assert e[f] <= MARGIN * E, (what, name, mode, f, e[f], E)


def _rhs(name, k, seed):
    return np.random.default_rng(seed).standard_normal((zoo.case(name).n, k))


def _check_rel(what, X, Xo, bar):
    """Per column: relative 2-norm error against the long-double result below bar."""
    X, Xo = np.atleast_2d(X.T).T, np.atleast_2d(Xo.T).T
    assert X.shape == Xo.shape
    worst = 0.0
    for j in range(Xo.shape[1]):
        err = float(np.linalg.norm(X[:, j] - Xo[:, j]) / np.linalg.norm(Xo[:, j]))
        worst = max(worst, err)
        assert err < bar, (what, j, err)
    print(f"{what}: worst column rel err {worst:.3e}")


def _backward_error(D, X, B):
    X, B = np.atleast_2d(X.T).T, np.atleast_2d(B.T).T
    anorm = np.abs(D).sum(axis=1).max()
    R = D @ X - B
    return max(np.abs(R[:, j]).max() / (anorm * np.abs(X[:, j]).max() + np.abs(B[:, j]).max())
               for j in range(B.shape[1]))


# ---- 1. the factor ----
@pytest.mark.parametrize("mode", zoo.MODES)
@pytest.mark.parametrize("name,tag", CONFIGS, ids=_ids(CONFIGS))
def test_factor_per_front(gpu, name, tag, mode):
    st, L = _numeric(name, tag, mode).export()
    assert st == 0
    _check_factor(tag, name, mode, L)


# ---- 2. solves and operators ----
@pytest.mark.parametrize("name,tag", BASIC, ids=_ids(BASIC))
def test_solves(gpu, name, tag):
    # one vector; 17 columns = a full 16-column panel and a partial one.  Bars of
    # tests/test_solve_multi.py (_check_columns): 1e-10 against the reference solve, 1e-14 backward
    num = _numeric(name, tag)
    c = zoo.case(name, "llt")
    D = c.dense()
    for B in (_rhs(name, 1, 31)[:, 0].copy(), _rhs(name, 17, 32)):
        X = num.solve(B)
        assert X.shape == B.shape
        _check_rel(f"{name} {tag} solve {B.shape}", X, c.ref.solve(B).astype(np.float64), 1e-10)
        be = _backward_error(D, X, B)
        print(f"{name} {tag} solve {B.shape}: backward error {be:.3e}")
        assert be < 1e-14


@pytest.mark.parametrize("name,tag", BASIC, ids=_ids(BASIC))
def test_operators(gpu, name, tag):
    num = _numeric(name, tag)
    ref = zoo.case(name, "llt").ref
    fn = {sc.SC_OP_SOLVE_A: ref.solve, sc.SC_OP_SOLVE_L: ref.solve_L, sc.SC_OP_SOLVE_LT: ref.solve_Lt,
          sc.SC_OP_MUL_L: ref.mul_L, sc.SC_OP_MUL_LT: ref.mul_Lt}
    for Z in (_rhs(name, 1, 33)[:, 0].copy(), _rhs(name, 17, 34)):
        for op in L_OPS:  # bar of tests/test_factor_apply.py
            _check_rel(f"{name} {tag} {OP_NAME[op]} {Z.shape}", num.apply(Z, op), fn[op](Z).astype(np.float64), 1e-10)
        # no fill-reducing ordering: P and P^T are copies
        assert np.array_equal(num.apply_P(Z), Z) and np.array_equal(num.apply_Pt(Z), Z)
        # half solves composed are the solve, bitwise (one vector: the single-vector kernels)
        x = num.apply_Pt(num.solve_Lt(num.solve_L(num.apply_P(Z))))
        assert np.array_equal(x, num.solve(Z))
        assert np.array_equal(num.apply(Z, sc.SC_OP_SOLVE_A), num.solve(Z))


@pytest.mark.parametrize("name,tag", BASIC, ids=_ids(BASIC))
def test_product_equals_A_and_logdet(gpu, name, tag):
    num = _numeric(name, tag)
    c = zoo.case(name, "llt")
    D = c.dense()
    anorm = np.abs(D).sum(axis=1).max()
    Z = _rhs(name, 17, 35)
    X = num.apply_Pt(num.mul_L(num.mul_Lt(num.apply_P(Z))))
    R = X - D @ Z
    err = max(np.abs(R[:, j]).max() / (anorm * np.abs(Z[:, j]).max()) for j in range(Z.shape[1]))
    print(f"{name} {tag}: |L L^T z - A z|_inf / (|A|_inf |z|_inf) = {err:.3e}")
    assert err < 1e-14
    d = np.diag(c.ref.L)
    ref, scale = float(2 * np.log(d).sum()), float(2 * np.abs(np.log(d)).sum())
    ld = num.logdet()
    print(f"{name} {tag}: logdet {ld!r} against {ref!r}, error / (2 sum |log L_jj|) = {abs(ld - ref) / scale:.3e}")
    assert abs(ld - ref) / scale < 1e-12
    assert num.logdet() == ld


# ---- 3. the selected inversion ----
@functools.lru_cache(maxsize=None)
def _inverses(name):
    """Two dense double inverses of A (llt values), as tests/test_selinv.py compares them."""
    import scipy.linalg as sla

    D = zoo.case(name, "llt").dense()
    Z1 = np.linalg.inv(D)
    X = sla.solve_triangular(np.linalg.cholesky(D), np.eye(len(D)), lower=True)
    Z2 = X.T @ X
    Z1.setflags(write=False)
    Z2.setflags(write=False)
    return Z1, Z2


SMALL_ENOUGH = [(n, t) for n, t in BASIC if n not in zoo.BIG]


@pytest.mark.parametrize("name,tag", SMALL_ENOUGH, ids=_ids(SMALL_ENOUGH))
def test_selected_inverse_vs_dense(gpu, name, tag):
    # the rule of tests/test_selinv.py (_bars): bar = max(1e-12, 100 x the disagreement of two
    # dense inverses).  On `forest` this covers every root: A^-1 is block diagonal over the
    # trees, so a root's Z_KK is the inverse of that component's Schur block, and the dense
    # inverse holds exactly that on the root's columns.
    num = _numeric(name, tag)
    assert num.selinv() == 0
    Lp, Li, Zx = num.selected_inverse()
    d = num.inverse_diagonal()
    ref = zoo.case(name, "llt").ref
    assert np.array_equal(Lp, ref.Lp) and np.array_equal(Li, ref.Li)
    Z1, Z2 = _inverses(name)
    rows, cols = Li.astype(np.int64), ref.cols
    zr, zr2 = Z1[rows, cols], Z2[rows, cols]
    d_nw = np.abs(zr - zr2).max() / np.abs(zr).max()
    d_dg = (np.abs(np.diag(Z1) - np.diag(Z2)) / np.abs(np.diag(Z1))).max()
    bar_nw, bar_dg = max(1e-12, 100 * d_nw), max(1e-12, 100 * d_dg)
    err_nw = np.abs(Zx - zr).max() / np.abs(zr).max()
    assert np.array_equal(d, Zx[Lp[:-1]])  # no ordering: the diagonal is each column's first entry
    err_dg = (np.abs(d - np.diag(Z1)) / np.abs(np.diag(Z1))).max()
    print(f"{name} {tag}: normwise {err_nw:.3e} (bar {bar_nw:.3e}); diagonal entrywise {err_dg:.3e} (bar {bar_dg:.3e})")
    assert err_nw < bar_nw and err_dg < bar_dg


BIG = [(n, t) for n, t in BASIC if n in zoo.BIG]


@pytest.mark.parametrize("name,tag", BIG, ids=_ids(BIG))
def test_selected_inverse_columns_vs_splu(gpu, name, tag):
    # as test_lap24_columns_vs_splu: sparse LU columns A^-1 e_j on the pattern of column j, bar
    # 1e-10; columns of the root, of the fan-in parent, of the first and last leaves and random ones
    import scipy.sparse as sp
    from scipy.sparse.linalg import splu

    num = _numeric(name, tag)
    c = zoo.case(name, "llt")
    st, n = c.st, c.n
    Lp, Li, Zx = num.selected_inverse()
    fronts = [0, 299 if len(st.w) > 299 else len(st.w) - 2, len(st.w) - 2, len(st.w) - 1]
    cols = sorted({int(st.start[f] + k) for f in fronts for k in (0, st.w[f] // 2, st.w[f] - 1)}
                  | set(np.random.default_rng(9).integers(0, n, 24).tolist()))
    lu = splu(sp.csc_matrix(c.dense()))
    worst = 0.0
    for j in cols:
        e = np.zeros(n)
        e[j] = 1.0
        x = lu.solve(e)
        rows = Li[Lp[j]:Lp[j + 1]]
        err = np.abs(Zx[Lp[j]:Lp[j + 1]] - x[rows]).max() / np.abs(x[rows]).max()
        worst = max(worst, err)
        assert err < 1e-10, (j, err)
    assert np.array_equal(num.inverse_diagonal(), Zx[Lp[:-1]])
    print(f"{name} {tag}: {len(cols)} columns, worst normwise error on a column's pattern {worst:.3e}")


@pytest.mark.parametrize("name,tag", BASIC, ids=_ids(BASIC))
def test_trace_of_A_times_Z(gpu, name, tag):
    # tr(A Z) = n needs Z on the pattern of A only, which here is the pattern of L
    num = _numeric(name, tag)
    c = zoo.case(name, "llt")
    Lp, Li, Zx = num.selected_inverse()
    D = c.dense()
    a = D[Li.astype(np.int64), c.ref.cols]
    off = Li != c.ref.cols
    tr = math.fsum(a[~off] * Zx[~off]) + 2.0 * math.fsum(a[off] * Zx[off])
    print(f"{name} {tag}: tr(A Z) - n = {tr - c.n:.3e}")
    assert abs(tr - c.n) <= 1e-10 * c.n


# ---- 4. bitwise ----
BITWISE = [n for n in zoo.NAMES if n in zoo.TINY or n in ("chain300_edges", "fanin300_mid_cb", "forest",
                                                          "big_nested_gather", "big_gather_k200")]


@pytest.mark.parametrize("tag", ["relax0", "default"])
@pytest.mark.parametrize("name", BITWISE)
def test_bitwise(gpu, name, tag):
    A = zoo.case(name, "llt").A
    eager = _fresh(name, tag, use_graph=0)
    graph = _fresh(name, tag, use_graph=1)
    L0 = eager.export()[1].x
    assert np.array_equal(graph.export()[1].x, L0)  # eager and graph replay
    for num in (eager, graph):
        assert num.factor(A.x) == 0  # again through the same handle
        assert np.array_equal(num.export()[1].x, L0)
    assert np.array_equal(_numeric(name, tag).export()[1].x, L0)  # another handle
    b, B = _rhs(name, 1, 41)[:, 0].copy(), _rhs(name, 17, 42)
    x, X = eager.solve(b), eager.solve(B)
    assert np.array_equal(eager.solve(b), x) and np.array_equal(eager.solve(B), X)
    assert np.array_equal(graph.solve(b), x) and np.array_equal(graph.solve(B), X)


# ---- 5. scaling by powers of four ----
@pytest.mark.parametrize("k", [150, -150])
@pytest.mark.parametrize("name,tag", [("tiny_hbm_pairs", "relax0"), ("chain300_edges", "relax0"), ("edges_b", "relax0"),
                                      ("edges_b", "allfronts")],
                         ids=["tiny_hbm_pairs", "chain300_edges", "edges_b", "edges_b_allfronts"])
def test_scaling_by_powers_of_four_is_exact(gpu, name, tag, k):
    # A 4^k has entries near 2^(+-300).  rsqrt_f64 is covariant under powers of four (the
    # v_rsq seed, then two Newton steps whose products are scale-free), everything else in the
    # factorization, the solves and the selected inversion is multiply-add, reciprocals of
    # pivots or divisions by them (exact in the exponent), and nothing leaves the normal range
    # at these exponents: the results are those of A scaled, bit for bit.  The logarithm is
    # not covariant: log(2^k l) = k log 2 + log l is rounded once more, so the log-determinant
    # is held to the project's logdet bar instead.
    base = _numeric(name, tag)
    c = zoo.case(name, "llt")
    n = c.n
    num = _fresh(name, tag, scale=4.0 ** k)
    L0, L1 = base.export()[1].x, num.export()[1].x
    assert np.array_equal(L1, L0 * 2.0 ** k)
    b, B = _rhs(name, 1, 51)[:, 0].copy(), _rhs(name, 17, 52)
    assert np.array_equal(num.solve(b), base.solve(b) * 4.0 ** -k)
    assert np.array_equal(num.solve(B), base.solve(B) * 4.0 ** -k)
    assert np.array_equal(num.selected_inverse()[2], base.selected_inverse()[2] * 4.0 ** -k)
    assert np.array_equal(num.inverse_diagonal(), base.inverse_diagonal() * 4.0 ** -k)
    want = base.logdet() + n * k * math.log(4.0)
    scale = float(2 * np.abs(np.log(np.diag(c.ref.L)) + k * math.log(2.0)).sum())
    got = num.logdet()
    print(f"{name} k={k}: logdet {got!r} against {want!r}, error / (2 sum |log L_jj|) = {abs(got - want) / scale:.3e}")
    assert abs(got - want) / scale < 1e-12


# ---- 6. not positive definite ----
def _expected_status(A, ordering=0):
    """The oracle's status; under an ordering, for P A P^T (the documented meaning: the column
    is counted in the order of the matrix that is factored)."""
    if ordering:
        A = sc.permute_symmetric(A, sc.Symbolic(A, ordering=ordering).perm().astype(np.int64))
    return oracle.chol(A)[0]


@pytest.mark.parametrize("tag", ["relax0", "default"])
@pytest.mark.parametrize("name", list(zoo.SINGLE_FAILURES))
def test_one_bad_pivot(gpu, name, tag):
    A, j = zoo.single_failure(name)
    bad = zoo.with_bad_pivots(A, (j,))
    num = sc.Numeric(sc.Symbolic(A, **OPTS[tag]))
    st = num.factor(bad.x)
    assert st == _expected_status(bad) == j + 1
    # the handle recovers: good values give status 0 and the factor of a handle that never failed
    assert num.factor(A.x) == 0
    st, L = num.export()
    other = sc.Numeric(sc.Symbolic(A, **OPTS[tag]))
    assert other.factor(A.x) == 0
    assert st == 0 and np.array_equal(L.x, other.export()[1].x)
    Lx = oracle.chol(A)[3]
    assert np.linalg.norm(L.x - Lx) / np.linalg.norm(Lx) < 1e-12


@pytest.mark.parametrize("handle", ["single", "two_ranks"])
@pytest.mark.parametrize("opts", [dict(relax=0), {}, dict(ordering=1)], ids=["relax0", "default", "nd"])
@pytest.mark.parametrize("name", list(zoo.DOUBLE_FAILURES))
def test_two_bad_pivots_report_the_first_natural_column(gpu, name, opts, handle):
    # two failing pivots in independent subtrees, the one with the smaller natural column
    # factored later (tests/test_zoo_cpu.py asserts that): the status is the reference's, the
    # smaller natural column
    A, (a, b) = zoo.double_failure(name)
    bad = zoo.with_bad_pivots(A, (a, b))
    want = _expected_status(bad, opts.get("ordering", 0))
    if not opts.get("ordering", 0):
        assert want == a + 1
    symb = sc.Symbolic(A, **opts)
    num = sc.Numeric(symb, nranks=2, virtual=True) if handle == "two_ranks" else sc.Numeric(symb)
    st = num.factor(bad.x)
    print(f"{name} {opts} {handle}: status {st}, the reference's {want}")
    assert st == want
    assert num.status() == want
    assert num.factor(A.x) == 0  # and the handle recovers


@pytest.mark.parametrize("tiny_dense", [0, 1])
def test_two_bad_pivots_tiny(gpu, tiny_dense):
    # n = 48: the tiny tree (status word in LDS) and the dense single-wave kernel, in which a
    # failed pivot's NaN spreads over every later column, independent ones included
    A, (a, b) = zoo.double_failure("bcsstk01_renumbered")
    symb = sc.Symbolic(A, tiny_dense=tiny_dense)
    assert symb.schedule_digest()["calls"]["tiny_dense" if tiny_dense else "tiny_tree"] == 1
    num = sc.Numeric(symb)
    for cols in ((a, b), (b,), (a,)):
        bad = zoo.with_bad_pivots(A, cols)
        want = oracle.chol(bad)[0]
        assert want == min(cols) + 1
        assert num.factor(bad.x) == want, cols
    assert num.factor(A.x) == 0
    Lx = oracle.chol(A)[3]
    assert np.linalg.norm(num.export()[1].x - Lx) / np.linalg.norm(Lx) < 1e-12


# ---- 7. emulated ranks ----
@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("name", ["forest", "fanin300_mid_cb", "big_gather_k200"])
def test_emulated_ranks(gpu, name, nranks):
    # as test_partitioned_split_fronts_emulated: every rank in one process with private memory
    c = zoo.case(name, "llt")
    symb = sc.Symbolic(c.A, relax=0)
    v = sc.Numeric(symb, nranks=nranks, virtual=True)
    for _ in range(2):  # the second time through reused arenas
        assert v.factor(c.A.x) == 0
    st, L = v.export()
    assert st == 0
    _check_factor(f"{nranks} ranks", name, "llt", L)
    b = _rhs(name, 1, 61)[:, 0].copy()
    assert _backward_error(c.dense(), v.solve(b), b) < 1e-14
