"""Smallest eigenpairs by block shift-invert Lanczos (Numeric.eigsh) on the GPU.

References: eigs_cases.emulate, the numpy model of the documented algorithm (pinned by
test_eigs_cases_cpu.py), for block counts; scipy.linalg.eigh of the dense matrix for the
eigenvalues.  All at tol = 1e-10, X0 passed so that the model sees the same start block.

Bounds (u = 2^-53, n the order, |A| the infinity norm >= the 2-norm):
  (a) every pair CONVERGED, blocks <= the model's + 1 (an estimate within rounding of tol can
      fall on either side);
  (b) info.resid agrees with |F x - x / theta| recomputed in numpy with the dense F to
      gamma-level -- 4 (gamma_{w+3} |F| + u / theta) sqrt(n), w the longest row: both are
      computed sums of at most w + 1 products per entry plus one more fma, and norms of n
      entries -- and is <= tol |A|: |F x - x / theta| = |F r| / theta <= |F| est / theta;
  (c) |lambda_i - mu_i| <= resid_i + n u |A|, mu the i-th eigenvalue from eigh: the residual
      bound for a unit vector plus eigh's own error; it fails when an eigenvalue is missed;
  (d) max |X^T X - I| <= 64 n u.
"""
import functools

import numpy as np
import pytest

import sparsecholesky_amd as sc

import eigs_cases as ec
from refine_cases import bits

pytestmark = pytest.mark.gpu

TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _numeric(name):
    return _fresh(name)


def _fresh(name, shift=0.0):
    A, kw = ec.matrix(name)
    num = sc.Numeric(sc.Symbolic(A, **kw))
    assert num.factor(_shifted(A, shift)) == 0
    return num


def _shifted(A, shift):
    x = np.array(A.x, dtype=np.float64)
    if shift:
        for i in range(A.size()):
            x[A.find_index(i, i)] += shift
    return x


@functools.lru_cache(maxsize=None)
def _mu(name):
    import scipy.linalg as sla

    return sla.eigh(ec.dense(name), eigvals_only=True)


def _norm(name):
    return np.abs(ec.dense(name)).sum(axis=1).max()


def _nevs(name):
    n = ec.dense(name).shape[0]
    return sorted({1, min(6, n), min(16, n)})


def _checks_bcd(name, lam, X, info, tag, Fd=None, sigma=0.0):
    """(b), (c), (d) for a result of the library; prints every figure before it asserts."""
    Fd = ec.dense(name) if Fd is None else Fd
    n, nev = X.shape
    norm, mu = np.abs(Fd).sum(axis=1).max(), _mu(name)[:nev]  # |F| (= |A| without a shift)
    theta = 1.0 / (lam - sigma)
    resid = np.linalg.norm(Fd @ X - X / theta, axis=0)
    w = int((Fd != 0.0).sum(axis=1).max())
    slack = 4.0 * (ec.gamma(w + 3) * (norm + abs(sigma)) + ec.U / theta) * np.sqrt(n)
    orth = float(np.max(np.abs(X.T @ X - np.eye(nev))))
    print(f"eigs {tag}: blocks {info['blocks'][0]}, resid max {info['resid'].max():.2e} = "
          f"{info['resid'].max() / (TOL * norm):.3f} tol |A|, |resid - numpy| max {np.abs(info['resid'] - resid).max():.1e} "
          f"(slack {slack.min():.1e}), |lam - mu| max {np.abs(lam - mu).max():.2e}, "
          f"|X^T X - I| {orth:.2e} (bar {64 * n * ec.U:.2e})")
    assert np.all(np.diff(lam) >= 0.0)
    assert np.all(np.abs(info["resid"] - resid) <= slack)
    assert np.all(info["resid"] <= TOL * norm)
    assert np.all(np.abs(lam - mu) <= info["resid"] + n * ec.U * norm)
    assert orth <= 64 * n * ec.U


# ---- (a) - (d), with the triple eigenvalues of lap8 and nev = 16 = b ----
@pytest.mark.parametrize("name", ec.INPUTS)
def test_against_the_model_and_eigh(gpu, name):
    num, Fd = _numeric(name), ec.dense(name)
    n = Fd.shape[0]
    X0 = ec.start_uniform(n)
    for nev in _nevs(name):
        lam, X, info = num.eigsh(nev, tol=TOL, X0=X0, return_info=True)
        e = ec.emulate(Fd, nev, X0, tol=TOL)
        print(f"eigs {name} nev {nev}: blocks {info['blocks'][0]} (model {e['blocks']}), est / (tol theta) max "
              f"{np.max(info['est'] * (lam - 0.0)) / TOL:.3f}")
        assert X.shape == (n, nev) and np.all(info["blocks"] == info["blocks"][0])
        assert np.all(info["state"] == ec.CONVERGED), info["state"]
        assert info["blocks"][0] <= e["blocks"] + 1
        assert np.all(info["est"] <= TOL / lam * (1.0 + 4 * ec.U))
        _checks_bcd(name, lam, X, info, f"{name} nev {nev}")
    if name.startswith("lap8"):  # the second eigenvalue of the grid Laplacian is a triple one
        mu = _mu(name)
        assert abs(mu[1] - mu[3]) < 1e-12 and np.max(np.abs(lam[1:4] - mu[1])) <= info["resid"][1:4].max() + 1e-12


# ---- (e) the library's start block; bits repeat across calls and handles ----
@pytest.mark.parametrize("name", ("lap8_nd", "bus_nd"))
def test_default_start_and_bits(gpu, name):
    num = _numeric(name)
    lam, X, info = num.eigsh(6, tol=TOL, return_info=True)
    assert np.all(info["state"] == ec.CONVERGED)
    _checks_bcd(name, lam, X, info, f"{name} default start")
    e = ec.emulate(ec.dense(name), 6, ec.start_library(X.shape[0], 1), tol=TOL)
    assert info["blocks"][0] <= e["blocks"] + 1  # the start block is the documented one
    lam2, X2, info2 = num.eigsh(6, tol=TOL, seed=1, return_info=True)
    lam3, X3, info3 = _fresh(name).eigsh(6, tol=TOL, return_info=True)
    for l, x, i in ((lam2, X2, info2), (lam3, X3, info3)):
        assert np.array_equal(bits(l), bits(lam)) and np.array_equal(bits(x), bits(X))
        assert all(np.array_equal(bits(np.asarray(i[f], dtype=np.float64)), bits(np.asarray(info[f], dtype=np.float64)))
                   for f in info)
    lam4, X4 = num.eigsh(6, tol=TOL, seed=2)
    assert not np.array_equal(bits(X4), bits(X))
    assert np.all(np.abs(lam4 - lam) <= 2 * TOL * _norm(name))


def test_device_form(gpu):
    import torch

    name = "lap8_nd"
    num, A = _numeric(name), ec.matrix(name)[0]
    n = A.size()
    X0 = ec.start_uniform(n)
    lam, X, info = num.eigsh(6, tol=TOL, X0=X0, return_info=True)
    dl, dX, dinfo = num.eigsh_device(6, tol=TOL, X0=torch.tensor(np.array(X0), device="cuda"),
                                     values=torch.tensor(np.asarray(A.x, dtype=np.float64), device="cuda"),
                                     return_info=True)
    assert dX.is_cuda and tuple(dX.shape) == (n, 6)
    assert np.array_equal(bits(dl), bits(lam)) and np.array_equal(bits(dX.cpu().numpy()), bits(X))
    assert np.array_equal(dinfo["resid"], info["resid"])


# ---- (f) sigma ----
def test_sigma(gpu):
    name = "lap8"
    Fd, n = ec.dense(name), 512
    X0 = ec.start_uniform(n)
    lam0, _, i0 = _numeric(name).eigsh(6, tol=TOL, X0=X0, return_info=True)
    num = _fresh(name, shift=0.5)
    lam, X, info = num.eigsh(6, sigma=-0.5, tol=TOL, X0=X0, return_info=True)
    assert np.all(info["state"] == ec.CONVERGED)
    _checks_bcd(name, lam, X, info, "lap8 + 0.5 I, sigma -0.5", Fd=Fd + 0.5 * np.eye(n), sigma=-0.5)
    assert np.all(np.abs(lam - lam0) <= info["resid"] + i0["resid"] + 2 * n * ec.U * (_norm(name) + 0.5))


# ---- (g) the block cap ----
def test_max_blocks(gpu):
    num = _numeric("lap8")
    lam, X, info = num.eigsh(6, tol=TOL, X0=ec.start_uniform(512), max_blocks=2, return_info=True)
    assert np.all(info["blocks"] == 2) and np.all(info["state"] == ec.MAXBLOCKS)
    assert np.all(info["est"] > TOL / lam * (1.0 - 4 * ec.U)) and np.all(np.isfinite(X))
    # Ritz values of inv(F) on a subspace lie below its eigenvalues (Cauchy interlacing): lambda from above
    assert np.all(lam >= _mu("lap8")[:6] - 512 * ec.U * _norm("lap8"))


# ---- (h) a rank-deficient start ----
def test_dependent_start_columns(gpu):
    num = _numeric("lap8")
    X0 = np.array(ec.start_uniform(512))
    X0[:, 5] = X0[:, 2]
    lam, X, info = num.eigsh(4, tol=TOL, X0=X0, return_info=True)
    print(f"eigs dependent start: states {info['state']}, blocks {info['blocks'][0]}, lam {lam}")
    assert np.all(np.isin(info["state"], (ec.EXHAUSTED, ec.CONVERGED)))
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(X)) and np.all(np.isfinite(info["resid"]))


# ---- (i) n < 16 ----
def test_small_n(gpu):
    num, Fd = _numeric("lap2"), ec.dense("lap2")
    lam, X, info = num.eigsh(8, tol=TOL, X0=ec.start_uniform(8), return_info=True)
    assert np.all(info["blocks"] == 1) and np.all(info["state"] == ec.CONVERGED)
    _checks_bcd("lap2", lam, X, info, "lap2 nev 8")
    assert np.max(np.abs(Fd @ X - X * lam)) <= 64 * 8 * ec.U * _norm("lap2")


# ---- (j) after an update of the factor ----
def test_follows_an_update(gpu):
    name = "lap8_nd"
    num, Fd = _fresh(name), ec.dense(name)
    n = Fd.shape[0]
    Wu = np.zeros((n, 2))
    Wu[3, 0], Wu[100, 1] = 1.0, 2.0  # one entry per column: inside any pattern
    num.update(Wu)
    Fn = Fd + Wu @ Wu.T
    import scipy.linalg as sla

    mu = sla.eigh(Fn, eigvals_only=True)[:6]
    X0 = ec.start_uniform(n)
    lam, X, info = num.eigsh(6, tol=TOL, X0=X0, return_info=True)  # the values A.x are stale: resid shows it
    norm = np.abs(Fn).sum(axis=1).max()
    true = np.linalg.norm(Fn @ X - X * lam, axis=0)
    print(f"eigs after update: |lam - mu| max {np.abs(lam - mu).max():.2e}, true resid max {true.max():.2e}, "
          f"reported (stale values) {info['resid'].max():.2e}")
    assert np.all(info["state"] == ec.CONVERGED)
    assert np.all(true <= TOL * norm) and np.all(np.abs(lam - mu) <= true + n * ec.U * norm)
    assert np.max(np.abs(mu - _mu(name)[:6])) > 1e-6  # and they moved


# ---- (k) values other than the factored ones ----
def test_other_values_show_in_resid(gpu):
    name = "bcsstk01"
    num, A = _numeric(name), ec.matrix(name)[0]
    X0 = ec.start_uniform(A.size())
    lam, X, info = num.eigsh(6, tol=TOL, X0=X0, return_info=True)
    lam2, X2, info2 = num.eigsh(6, tol=TOL, X0=X0, values=1.01 * np.asarray(A.x), return_info=True)
    assert np.array_equal(bits(lam), bits(lam2)) and np.array_equal(bits(X), bits(X2))
    assert np.array_equal(info["est"], info2["est"])
    # F' x - x / theta = 0.01 F x + (F x - x / theta): about 0.01 lambda
    assert np.all(info2["resid"] >= 0.009 * lam) and np.all(info2["resid"] > 1e3 * info["resid"])
