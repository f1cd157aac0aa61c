"""The numpy model of the conjugate gradients (pcg_cases.emulate) is what the GPU tests measure
iteration counts against, so it is pinned here, without a GPU.

In exact arithmetic CG with k eigenvalues of inv(M) A' away from 1 (and the start x_0 = M b)
ends after at most k + 1 steps: the residual polynomial needs one root per distinct eigenvalue.
The tests allow one more step for rounding: k + 2 = 5 on the rank-3 cases, 2 on A' = 3 A (one
eigenvalue, 3, and none at 1).  A' = -A makes p.A'p negative for the first direction: a
breakdown before any step.  Two deliberately wrong methods must fail the same checks.
"""
import numpy as np
import pytest

import pcg_cases as pc

MATRICES = ("bcsstk01", "lap8", "bus_nd")
TOL = 1e-12


@pytest.fixture(scope="module")
def dense():
    out = {}
    for name in MATRICES:
        A, _ = pc.matrix(name)
        out[name] = (A, pc.dense(A), pc.rhs(A.size(), 2))
    return out


def _rank3_ok(Ad, Md, b, wrong=None):
    e = pc.emulate(Ad, Md, b, tol=TOL, max_iter=50, wrong=wrong)
    return e["state"] == pc.CONVERGED and 1 <= e["iters"] <= 5, e


@pytest.mark.parametrize("name", MATRICES)
def test_rank3_converges_in_k_plus_2_steps(dense, name):
    A, Md, B = dense[name]
    Ad = pc.dense(A, pc.values_rank3(A))
    # the refinement this replaces cannot work here: rho(I - inv(A) A') >= 2
    lam = np.linalg.eigvals(np.linalg.solve(Md, Ad)).real
    assert np.sum(np.abs(lam - 1.0) > 1e-6) == 3 and np.max(np.abs(1.0 - lam)) > 2.0
    for c in range(B.shape[1]):
        ok, e = _rank3_ok(Ad, Md, B[:, c])
        print(f"PCG model {name} rank 3 col {c}: iters {e['iters']} (<= 5), relres {e['relres']:.2e}, "
              f"true {e['relres_true']:.2e}")
        assert ok, e["hist"]
        assert e["relres"] <= TOL


@pytest.mark.parametrize("name", MATRICES)
def test_three_a_converges_in_two_steps(dense, name):
    A, Md, B = dense[name]
    for c in range(B.shape[1]):
        e = pc.emulate(3.0 * Md, Md, B[:, c], tol=TOL)
        print(f"PCG model {name} 3 A col {c}: iters {e['iters']} (<= 2), relres {e['relres']:.2e}")
        assert e["state"] == pc.CONVERGED and 1 <= e["iters"] <= 2, e["hist"]


@pytest.mark.parametrize("name", MATRICES)
def test_minus_a_breaks_down_before_a_step(dense, name):
    import scipy.linalg as sla

    A, Md, B = dense[name]
    e = pc.emulate(-Md, Md, B[:, 0], tol=TOL)
    assert e["state"] == pc.BREAKDOWN and e["iters"] == 0
    assert np.array_equal(e["x"], sla.cho_solve(sla.cho_factor(Md, lower=True), B[:, 0]))
    assert abs(e["relres"] - 2.0) < 1e-6  # r = b - (-A) inv(A) b = 2 b


def test_start_rules(dense):
    A, Md, B = dense["lap8"]
    b = B[:, 0]
    e = pc.emulate(Md, Md, b)  # the factored values: nothing to do
    assert (e["iters"], e["state"]) == (0, pc.CONVERGED) and e["relres"] < 1e-14
    e = pc.emulate(3.0 * Md, Md, np.zeros_like(b))
    assert (e["iters"], e["state"]) == (0, pc.CONVERGED) and not e["x"].any() and e["relres"] == 0.0
    e = pc.emulate(3.0 * Md, Md, b, max_iter=0)
    assert (e["iters"], e["state"]) == (0, pc.MAXITER)
    e = pc.emulate(pc.dense(A, pc.values_dad(A, 0.1)), Md, b, tol=0.0, max_iter=7)
    assert (e["iters"], e["state"]) == (7, pc.MAXITER)
    # a warm start at the solution stops at once, one from zero needs about a cold start's steps
    Ad = pc.dense(A, pc.values_rank3(A))
    x = np.linalg.solve(Ad, b)
    e = pc.emulate(Ad, Md, b, x0=x)
    assert (e["iters"], e["state"]) == (0, pc.CONVERGED) and np.array_equal(e["x"], x)
    cold, zero = pc.emulate(Ad, Md, b), pc.emulate(Ad, Md, b, x0=np.zeros_like(b))
    assert abs(cold["iters"] - zero["iters"]) <= 1


@pytest.mark.parametrize("wrong", ["beta_inverted", "alpha_old_rho"])
@pytest.mark.parametrize("name", MATRICES)
def test_wrong_methods_are_caught(dense, name, wrong):
    """The rank-3 check must tell a CG with a wrong coefficient from the right one."""
    A, Md, B = dense[name]
    Ad = pc.dense(A, pc.values_rank3(A))
    ok, e = _rank3_ok(Ad, Md, B[:, 0], wrong=wrong)
    print(f"PCG model {name} {wrong}: iters {e['iters']}, state {e['state']}, relres {e['relres']:.2e}")
    assert not ok
    # while the first step, where both mistakes are invisible, still solves 3 A
    e = pc.emulate(3.0 * Md, Md, B[:, 0], tol=1e-10, wrong=wrong)
    assert e["iters"] == 1
