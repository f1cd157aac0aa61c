"""The gradient kernels on the GPU through the public entries: the sampled outer product and the
pattern dot against integer arithmetic, the Z gather against the exported selected inverse.

Outer product and dot.  The data are integers in [-1024, 1024] times 2^-10, so every product (an
integer times 2^-20) and every sum of up to 66 of them is exact in fp64, as are alpha, beta in {1,
-1, 0.5} and {0, 1, 0.5}: the result must equal integer arithmetic bit for bit whatever the order
of the sums.  The device form is the one under test (the kernels see the caller's leading
dimension there); the host form must return the same bits.

Z gather.  logdet_grad()[k] and the entry of selected_inverse() at the permuted (i, j) are two
copies of one number of the Z panel (times c_k, exact), so they are equal bit for bit."""
import ctypes

import numpy as np
import pytest

import grad_cases as gc
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

NRHS = (0, 1, 5, 16, 17, 33)
ALPHAS = (1.0, -1.0, 0.5)
BETAS = (0.0, 1.0, 0.5)


def _csc(n, cols):
    """Upper CSC from per-column row lists (values: a diagonally dominant filler, never read by
    the outer product or the dot)."""
    Ap = np.cumsum([0] + [len(c) for c in cols]).astype(np.int64)
    Ai = np.array([r for c in cols for r in c], dtype=np.int32)
    Ax = np.where(Ai == np.repeat(np.arange(n), np.diff(Ap)), float(n + 1), -0.5)
    return sc.csc_matrix(n, n, Ap, Ai, Ax.astype(np.float64))


def _banded(n, seed):
    rng = np.random.default_rng(seed)
    cols = []
    for j in range(n):
        r = {j} | ({j - 1} if j else set()) | {int(v) for v in rng.integers(0, j + 1, 2)}
        cols.append(sorted(r))
    return _csc(n, cols)


def _pattern(name):
    if name == "six":
        return gc.matrix("six")
    if name == "diag":
        return _csc(40, [[j] for j in range(40)])
    if name == "dense70":
        return _csc(70, [list(range(j + 1)) for j in range(70)])
    if name == "arrow":  # the last column holds 300 entries
        return _csc(300, [[j] for j in range(299)] + [list(range(300))])
    return _banded(int(name[1:]), 11)


PATTERNS = ("n1", "n2", "n63", "n64", "n65", "n257", "diag", "dense70", "arrow", "six")
_cache = {}


def _handle(name):
    if name not in _cache:
        A = _pattern(name)
        _cache[name] = (A, sc.Numeric(sc.Symbolic(A)))  # never factored: the outer product needs no factor
    return _cache[name]


def _ints(rng, shape):
    return rng.integers(-1024, 1025, size=shape)


def _expected(A, Ui, Vi, Gi, alpha, beta):
    """Integer arithmetic in units of 2^-21, then one exact scaling."""
    n = A.size()
    rows, cols, eff = gc.classify(n, A.p, A.i)
    s = (Ui[rows] * Vi[cols]).sum(axis=1)
    s = s + np.where(rows != cols, (Ui[cols] * Vi[rows]).sum(axis=1), 0)
    e = int(2 * alpha) * s + int(2 * beta) * Gi * 1024
    assert np.abs(e).max(initial=0) < 2 ** 52
    return np.where(eff, e.astype(np.float64) * 2.0 ** -21, 0.0), eff


def _device_panel(torch, M, ld):
    """n x k integers times 2^-10 as a column-major device panel of leading dimension ld, NaN in
    the padding: (tensor of shape (k, ld), pointer)."""
    n, k = M.shape
    T = np.full((max(k, 1), ld), np.nan)
    T[:k, :n] = M.T * 2.0 ** -10
    t = torch.from_numpy(T).cuda()
    return t, t.data_ptr()


@pytest.mark.parametrize("name", PATTERNS)
def test_outer_product_is_exact(gpu, name):
    import torch

    A, num = _handle(name)
    n, nnz = A.size(), len(A.x)
    rng = np.random.default_rng(5)
    combos = [(a, b) for a in ALPHAS for b in BETAS]
    q = 0
    for k in NRHS:
        for ld in (n, n + 3):
            Ui, Vi, Gi = _ints(rng, (n, k)), _ints(rng, (n, k)), _ints(rng, nnz)
            tU, pU = _device_panel(torch, Ui, ld)
            tV, pV = _device_panel(torch, Vi, ld)
            U0, V0 = tU.clone(), tV.clone()
            # every (alpha, beta) over the loop, three per shape
            for alpha, beta in (combos[(q + t) % 9] for t in range(3)):
                want, eff = _expected(A, Ui, Vi, Gi, alpha, beta)
                G = torch.from_numpy(Gi * 2.0 ** -10 if beta != 0.0 else np.full(nnz, np.nan)).cuda()
                num.pattern_outer_device(pU, pV, k, ld, ld, G.data_ptr(), alpha=alpha, beta=beta)
                got = G.cpu().numpy()
                assert np.array_equal(got, want), (name, k, ld, alpha, beta)
                assert not np.signbit(got[~eff]).any()  # ignored slots: +0.0
            q += 3
            # the inputs, padding included, are as they were
            assert torch.equal(torch.nan_to_num(tU, nan=7.0), torch.nan_to_num(U0, nan=7.0))
            assert torch.equal(torch.nan_to_num(tV, nan=7.0), torch.nan_to_num(V0, nan=7.0))


@pytest.mark.parametrize("name", ("n65", "arrow", "six"))
def test_host_form_repeat_and_second_handle_give_equal_bits(gpu, name):
    A, num = _handle(name)
    n, nnz = A.size(), len(A.x)
    rng = np.random.default_rng(9)
    other = sc.Numeric(sc.Symbolic(A))
    for k in (5, 33):
        # general data: nothing exact here, only the order of the sums makes the bits equal
        U, V, G0 = rng.standard_normal((n, k)), rng.standard_normal((n, k)), rng.standard_normal(nnz)
        g1 = num.pattern_outer(U, V, alpha=0.5, beta=0.5, G=G0)
        assert np.array_equal(num.pattern_outer(U, V, alpha=0.5, beta=0.5, G=G0), g1)
        assert np.array_equal(other.pattern_outer(U, V, alpha=0.5, beta=0.5, G=G0), g1)
        # against the model: 2 k + 2 roundings of terms whose sizes add up to `size`, two orders of summation
        ref = gc.outer(n, A.p, A.i, U, V, 0.5, 0.5, G0)
        size = gc.outer(n, A.p, A.i, np.abs(U), np.abs(V), 0.5, 0.5, np.abs(G0))
        assert np.abs(g1 - ref).max() <= 4 * (2 * k + 2) * gc.U * size.max()
        d1 = num.pattern_dot(g1, G0)
        assert num.pattern_dot(g1, G0) == d1 and other.pattern_dot(g1, G0) == d1
    # exact data through the host form
    Ui, Vi, Gi = _ints(rng, (n, 17)), _ints(rng, (n, 17)), _ints(rng, nnz)
    want, _ = _expected(A, Ui, Vi, Gi, -1.0, 0.5)
    got = num.pattern_outer(Ui * 2.0 ** -10, Vi * 2.0 ** -10, alpha=-1.0, beta=0.5, G=Gi * 2.0 ** -10)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", PATTERNS)
def test_pattern_dot_is_exact(gpu, name):
    import torch

    A, num = _handle(name)
    nnz = len(A.x)
    _, _, eff = gc.classify(A.size(), A.p, A.i)
    rng = np.random.default_rng(3)
    Gi, Hi = _ints(rng, nnz), _ints(rng, nnz)
    want = float(int((Gi[eff] * Hi[eff]).sum())) * 2.0 ** -20
    G, H = Gi * 2.0 ** -10, Hi * 2.0 ** -10
    G[~eff], H[~eff] = np.nan, np.nan  # ignored slots are not read
    assert num.pattern_dot(G, H) == want
    tG, tH = torch.from_numpy(G).cuda(), torch.from_numpy(H).cuda()
    assert num.pattern_dot_device(tG.data_ptr(), tH.data_ptr()) == want


def test_pattern_dot_over_several_workgroups(gpu):
    # 1138_bus has 2596 entries: three partials of 1024
    A = gc.matrix("1138_bus")
    num = sc.Numeric(sc.Symbolic(A))
    rng = np.random.default_rng(4)
    Gi, Hi = _ints(rng, len(A.x)), _ints(rng, len(A.x))
    assert len(A.x) > 2048
    assert num.pattern_dot(Gi * 2.0 ** -10, Hi * 2.0 ** -10) == float(int((Gi * Hi).sum())) * 2.0 ** -20


# ---- Z gather ----
def _lap(k, nd):
    return sc.laplacian3d(k, nd=nd)


ZCASES = {
    "lap4_nat": (lambda: _lap(4, False), {}),
    "lap4_nd": (lambda: _lap(4, True), {}),
    "bcsstk01": (lambda: gc.matrix("bcsstk01"), {}),
    "1138_bus_nd": (lambda: gc.matrix("1138_bus"), dict(ordering=1)),
    "1138_bus_amd": (lambda: gc.matrix("1138_bus"), dict(ordering=2)),
    "six": (lambda: gc.matrix("six"), {}),
    "six_amd": (lambda: gc.matrix("six"), dict(ordering=2)),
}


def _z_at_entries(num, A):
    """c_k Z[i_k, j_k] per value slot from the exported selected inverse (0 on ignored slots)."""
    n = A.size()
    rows, cols, eff = gc.classify(n, A.p, A.i)
    perm = num.symb.perm().astype(np.int64)
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    Lp, Li, Zx = num.selected_inverse()
    pos = {}
    for j in range(n):
        for p in range(int(Lp[j]), int(Lp[j + 1])):
            pos[(int(Li[p]), j)] = p
    out = np.zeros(len(rows))
    for k in np.flatnonzero(eff):
        a, b = iperm[rows[k]], iperm[cols[k]]
        out[k] = (1.0 if a == b else 2.0) * Zx[pos[(int(max(a, b)), int(min(a, b)))]]
    return out, eff


def _check_gather(num, A):
    want, eff = _z_at_entries(num, A)
    got = num.logdet_grad()
    assert np.array_equal(got, want)
    assert not np.signbit(got[~eff]).any()
    return got


@pytest.mark.parametrize("case", list(ZCASES))
def test_gather_equals_the_exported_inverse(gpu, case):
    make, kw = ZCASES[case]
    A = make()
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x) == 0
    assert num.selinv() == 0
    g = _check_gather(num, A)
    assert np.array_equal(num.logdet_grad(), g)  # a repeat
    other = sc.Numeric(sc.Symbolic(A, **kw))
    assert other.factor(A.x) == 0
    assert np.array_equal(other.logdet_grad(), g)  # a second handle, selinv run by the call itself


def test_gather_device_form(gpu):
    import torch

    A = gc.matrix("1138_bus")
    num = sc.Numeric(sc.Symbolic(A, ordering=1))
    assert num.factor(A.x) == 0
    G = torch.full((len(A.x),), float("nan"), dtype=torch.float64, device="cuda")
    assert num.logdet_grad_device(G.data_ptr()) == 0
    assert np.array_equal(G.cpu().numpy(), num.logdet_grad())


def test_gather_on_a_schur_handle(gpu):
    A = gc.matrix("1138_bus")
    num = sc.Numeric(sc.Symbolic(A, schur=[5, 700, 33, 1000]))
    assert num.factor(A.x) == 0
    _check_gather(num, A)


def test_gather_after_an_update_with_a_unit_vector(gpu):
    A = _lap(4, True)
    n = A.size()
    num = sc.Numeric(sc.Symbolic(A))
    assert num.factor(A.x) == 0
    g0 = num.logdet_grad()
    W = np.zeros((n, 1))
    W[n - 1, 0] = 1.5
    assert num.update(W) == 0
    g1 = _check_gather(num, A)  # the Z panel was recomputed: it belongs to A + w w^T
    D = gc.dense(n, A.p, A.i, A.x) + W @ W.T
    rows, cols, eff = gc.classify(n, A.p, A.i)
    ref = np.where(rows == cols, 1.0, 2.0) * np.linalg.inv(D)[rows, cols]
    assert np.abs(g1 - ref).max() <= 1e-12 * np.abs(ref).max()
    assert np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()
