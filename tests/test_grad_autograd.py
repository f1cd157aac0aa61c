"""The torch layer (sparsecholesky_amd.autograd): gradients equal to the Numeric methods bit for
bit, several functions through one factorization, torch's gradcheck, and the retired-view error."""
import numpy as np
import pytest

import grad_cases as gc
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    from sparsecholesky_amd.autograd import SparseCholesky

    return torch, SparseCholesky


def _values(torch, A):
    return torch.from_numpy(np.array(A.x)).cuda().requires_grad_(True)


def _reference(A, **kw):
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(A.x) == 0
    return num


@pytest.mark.parametrize("name,kw", [("bcsstk01", {}), ("1138_bus", dict(ordering=1)), ("six", {})])
def test_logdet_backward_is_logdet_grad(gpu, name, kw):
    torch, SparseCholesky = _torch()
    A = gc.matrix(name)
    v = _values(torch, A)
    F = SparseCholesky(sc.Symbolic(A, **kw))(v)
    ld = F.logdet()
    ref = _reference(A, **kw)
    assert ld.item() == ref.logdet()
    ld.backward()
    assert np.array_equal(v.grad.cpu().numpy(), ref.logdet_grad())


@pytest.mark.parametrize("name,kw,k", [("bcsstk01", {}, 3), ("1138_bus", dict(ordering=1), 20), ("six", {}, 1)])
def test_solve_backward_is_solve_grad(gpu, name, kw, k):
    torch, SparseCholesky = _torch()
    A = gc.matrix(name)
    n = A.size()
    rng = np.random.default_rng(k)
    Bn, Mn = rng.standard_normal((n, k)), rng.standard_normal((n, k))
    v = _values(torch, A)
    B = torch.from_numpy(Bn).cuda().requires_grad_(True)
    M = torch.from_numpy(Mn).cuda()
    F = SparseCholesky(sc.Symbolic(A, **kw))(v)
    X = F.solve(B)
    ref = _reference(A, **kw)
    Xn = X.detach().cpu().numpy()
    assert np.array_equal(Xn, ref.solve(Bn))
    (X * M).sum().backward()
    Bbar, G = ref.solve_grad(Mn, Xn)
    assert np.array_equal(B.grad.cpu().numpy(), Bbar)
    assert np.array_equal(v.grad.cpu().numpy(), G)


def test_one_dimensional_right_hand_side(gpu):
    torch, SparseCholesky = _torch()
    A = gc.matrix("bcsstk01")
    n = A.size()
    rng = np.random.default_rng(1)
    bn, mn = rng.standard_normal(n), rng.standard_normal(n)
    v = _values(torch, A)
    b = torch.from_numpy(bn).cuda().requires_grad_(True)
    x = SparseCholesky(sc.Symbolic(A))(v).solve(b)
    assert x.shape == (n,)
    (x * torch.from_numpy(mn).cuda()).sum().backward()
    ref = _reference(A)
    Bbar, G = ref.solve_grad(mn, x.detach().cpu().numpy())
    assert np.array_equal(b.grad.cpu().numpy(), Bbar) and np.array_equal(v.grad.cpu().numpy(), G)


def test_both_functions_through_one_factorization(gpu):
    torch, SparseCholesky = _torch()
    A = gc.matrix("six")
    n = A.size()
    rng = np.random.default_rng(2)
    Bn, Mn = rng.standard_normal((n, 2)), rng.standard_normal((n, 2))
    v = _values(torch, A)
    B = torch.from_numpy(Bn).cuda().requires_grad_(True)
    chol = SparseCholesky(sc.Symbolic(A))
    F = chol(v)
    X = F.solve(B)
    (F.logdet() + (X * torch.from_numpy(Mn).cuda()).sum()).backward()
    assert chol.generation == 1  # one factorization served both
    ref = _reference(A)
    Bbar, G = ref.solve_grad(Mn, X.detach().cpu().numpy())
    g = v.grad.cpu().numpy()
    assert np.array_equal(g, ref.logdet_grad() + G)
    assert np.array_equal(B.grad.cpu().numpy(), Bbar)
    # the slots the analysis ignores get zero gradient
    _, _, eff = gc.classify(n, A.p, A.i)
    assert (~eff).sum() == 5 and np.all(g[~eff] == 0.0)


@pytest.mark.parametrize("k", [2, 3])
def test_gradcheck(gpu, k):
    # torch's default fp64 settings (eps 1e-6, atol 1e-5, rtol 1e-3); cond_2 <= 5.8 here.  gradcheck
    # evaluates the function many times before it runs the backward of its first output, and a
    # handle holds one factor, so every evaluation gets a handle of its own.
    torch, SparseCholesky = _torch()
    A = sc.laplacian3d(k, nd=False)
    symb = sc.Symbolic(A)
    n = A.size()
    v = _values(torch, A)
    B = torch.from_numpy(np.random.default_rng(k).standard_normal((n, 2))).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: SparseCholesky(symb)(t).logdet(), (v,))
    assert torch.autograd.gradcheck(lambda t, b: SparseCholesky(symb)(t).solve(b), (v, B))


def test_backward_after_a_refactorization_raises(gpu):
    torch, SparseCholesky = _torch()
    A = gc.matrix("bcsstk01")
    v = _values(torch, A)
    chol = SparseCholesky(sc.Symbolic(A))
    F = chol(v)
    ld = F.logdet()
    X = F.solve(torch.ones(A.size(), 2, dtype=torch.float64, device="cuda"))
    F2 = chol((2.0 * v).detach())
    with pytest.raises(RuntimeError, match="refactored or the factor was updated"):
        ld.backward()
    with pytest.raises(RuntimeError, match="refactored or the factor was updated"):
        X.sum().backward()
    with pytest.raises(RuntimeError, match="refactored or the factor was updated"):
        F.logdet()
    assert v.grad is None
    assert F2.logdet().item() == pytest.approx(ld.item() + A.size() * np.log(2.0), rel=1e-12)
    # an update of the factor retires the view too
    W = np.zeros((A.size(), 1))
    W[-1, 0] = 1.0
    assert chol.update(W) == 0
    with pytest.raises(RuntimeError, match="refactored or the factor was updated"):
        F2.solve(torch.ones(A.size(), dtype=torch.float64, device="cuda"))


def test_not_positive_definite_raises_with_the_column(gpu):
    torch, SparseCholesky = _torch()
    A = gc.matrix("bcsstk01")
    x = np.array(A.x)
    x[A.p[21] - 1] = -1.0
    with pytest.raises(sc.LibraryError, match="not positive definite"):
        SparseCholesky(sc.Symbolic(A))(torch.from_numpy(x).cuda())
