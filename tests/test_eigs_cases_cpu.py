"""The numpy model of the block shift-invert Lanczos iteration (eigs_cases.emulate) is what the
GPU tests measure block counts against, so it is pinned here, without a GPU, against
scipy.linalg.eigh of the dense matrix -- with the checks the GPU tests apply (u = 2^-53):

  (a) every pair CONVERGED, in at most 16 blocks;
  (b) resid = |F x - x / theta| <= tol |F|_inf: with |x| = 1 and r = inv(F) x - theta x, |r| = est,
      F x - x / theta = -F r / theta, so resid <= |F|_2 est / theta <= tol |F|_2 <= tol |F|_inf;
  (c) |lambda_i - mu_i| <= resid_i + n u |A|_inf, mu ascending from eigh: a symmetric matrix has an
      eigenvalue within the residual of any unit vector's Ritz value, eigh's own error is of the
      order n u |A|, and the i-th of each list meet only when no eigenvalue was missed;
  (d) max |X^T X - I| <= 64 n u.

Three deliberately wrong methods must fail them.  The library's defaults, its start block and
its host dense algebra (which need no GPU) are pinned here too.
"""
import ctypes
import functools

import numpy as np
import pytest

import sparsecholesky_amd as sc

import eigs_cases as ec

TOL = 1e-10


@functools.lru_cache(maxsize=None)
def _eigh(name):
    import scipy.linalg as sla

    return sla.eigh(ec.dense(name), eigvals_only=True)


def verdict(name, e, nev, tol=TOL):
    """The checks (a) - (d) on a result dict (model's or library's); returns (ok, text)."""
    Fd = ec.dense(name)
    n = Fd.shape[0]
    norm = np.abs(Fd).sum(axis=1).max()
    mu = _eigh(name)[:nev]
    a = bool(np.all(e["state"] == ec.CONVERGED)) and e["blocks"] <= 16
    b = bool(np.all(e["resid"] <= tol * norm))
    c = bool(np.all(np.abs(e["lam"] - mu) <= e["resid"] + n * ec.U * norm))
    orth = float(np.max(np.abs(e["X"].T @ e["X"] - np.eye(nev))))
    d = orth <= 64 * n * ec.U
    text = (f"{name} nev {nev}: blocks {e['blocks']}, resid/(tol |A|) {np.max(e['resid']) / (tol * norm):.3f}, "
            f"|lam - mu| max {np.max(np.abs(e['lam'] - mu)):.2e}, |X^T X - I| {orth:.2e} (bar {64 * n * ec.U:.2e})")
    return a and b and c and d, text


def nevs(name):
    n = ec.dense(name).shape[0]
    return sorted({1, min(6, n), min(16, n)})


@pytest.mark.parametrize("name", ec.INPUTS)
def test_model_meets_the_checks(name):
    n = ec.dense(name).shape[0]
    for nev in nevs(name):
        e = ec.emulate(ec.dense(name), nev, ec.start_uniform(n), tol=TOL)
        ok, text = verdict(name, e, nev)
        print(f"eigs model {text}, smallest scaled pivot {e['min_pivot']:.1e} (threshold {2 * (n + 16) * ec.U:.1e})")
        assert ok, text
    if name == "lap2":
        assert e["blocks"] == 1
    if name == "bcsstk01":
        assert e["blocks"] == 3  # the whole space


def test_library_start_block_in_the_model():
    n = 512
    e = ec.emulate(ec.dense("lap8"), 6, ec.start_library(n), tol=TOL)
    ok, text = verdict("lap8", e, 6)
    assert ok, text


@pytest.mark.parametrize("wrong", ["one_pass", "est_first", "smallest"])
def test_wrong_methods_are_caught(wrong):
    """Each mistake fails the checks on at least one input, where the right method passes all."""
    failed = []
    for name in ("lap8", "bus_nd"):
        n = ec.dense(name).shape[0]
        # 17 blocks at most: check (a) fails whatever needs more than 16
        e = ec.emulate(ec.dense(name), 6, ec.start_uniform(n), tol=TOL, max_blocks=17, wrong=wrong)
        ok, text = verdict(name, e, 6)
        print(f"eigs model {wrong}: {text} -> {'passes' if ok else 'caught'}")
        if not ok:
            failed.append(name)
    assert failed


def test_stop_rules():
    Fd, n = ec.dense("lap8"), 512
    e = ec.emulate(Fd, 6, ec.start_uniform(n), tol=TOL, max_blocks=2)
    assert e["blocks"] == 2 and np.all(e["state"] == ec.MAXBLOCKS) and np.all(e["est"] > TOL * e["theta"])
    X0 = np.array(ec.start_uniform(n))
    X0[:, 5] = X0[:, 2]  # a dependent start column is dropped; the solve's block cannot grow the space
    e = ec.emulate(Fd, 4, X0, tol=TOL)
    assert e["blocks"] == 1 and np.all(np.isin(e["state"], (ec.EXHAUSTED, ec.CONVERGED)))
    assert np.all(np.isfinite(e["lam"])) and np.all(np.isfinite(e["X"]))
    # sigma: the factor of A + 0.5 I reports A's eigenvalues with sigma = -0.5
    e0 = ec.emulate(Fd, 6, ec.start_uniform(n), tol=TOL)
    e1 = ec.emulate(Fd + 0.5 * np.eye(n), 6, ec.start_uniform(n), tol=TOL, sigma=-0.5)
    norm = np.abs(Fd).sum(axis=1).max() + 0.5
    assert np.all(np.abs(e0["lam"] - e1["lam"]) <= e0["resid"] + e1["resid"] + 2 * n * ec.U * norm)


def test_default_options():
    o = sc.EigsOptions()
    sc.lib().sc_default_eigs_options(ctypes.byref(o))
    assert o.struct_size == ctypes.sizeof(sc.EigsOptions) == 40
    assert (o.max_blocks, o.use_x0, o.seed, o.tol, o.sigma) == (32, 0, 1, 1e-10, 0.0)
    assert ctypes.sizeof(sc.EigsInfo) == 24
    assert (sc.SC_EIGS_CONVERGED, sc.SC_EIGS_MAXBLOCKS, sc.SC_EIGS_EXHAUSTED) == (0, 1, 2)


def test_start_block_generator():
    """splitmix64 in Python integers, entry by entry, against the numpy form the tests pass on."""
    M = (1 << 64) - 1

    def entry(seed, i, c):
        z = (seed + (16 * i + c + 1) * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        return 2.0 * ((z >> 11) * 2.0 ** -53) - 1.0

    for n, seed in ((5, 1), (40, 2 ** 63 + 12345)):
        S = ec.start_library(n, seed)
        assert S.shape == (n, min(16, n)) and np.all((-1.0 <= S) & (S < 1.0))
        for i in (0, 1, n - 1):
            for c in (0, min(16, n) - 1):
                assert S[i, c] == entry(seed, i, c)
    assert abs(ec.start_library(4096).mean()) < 0.02


def _dense_hook(which, m, A, d):
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    return sc.lib().sc_debug_eigs_dense(which, m, P(A), P(d))


@pytest.mark.parametrize("m", [1, 2, 3, 16, 48, 208])
def test_host_eigensolver(m):
    """Householder + QL of the library against eigh: backward stable, so eigenvalues agree to a
    small multiple of m u |T|_2 and S^T T S is diagonal to the same; S orthogonal to m u."""
    rng = np.random.default_rng(m)
    Q, _ = np.linalg.qr(rng.standard_normal((m, m)))
    lam = np.sort(np.concatenate([rng.uniform(0.0, 1e-3, m - m // 2), rng.uniform(1.0, 40.0, m // 2)]))
    if m >= 3:
        lam[-3:] = lam[-1]  # a triple
    T = (Q * lam) @ Q.T
    T = 0.5 * (T + T.T)
    A, d = np.array(T, order="C"), np.zeros(m)
    assert _dense_hook(0, m, A, d) == 0
    nrm = np.linalg.norm(T, 2)
    bar = 20 * m * ec.U * nrm
    assert np.all(np.diff(d) >= 0.0)
    assert np.max(np.abs(d - np.linalg.eigvalsh(T))) <= bar
    assert np.max(np.abs(A.T @ A - np.eye(m))) <= 20 * m * ec.U
    assert np.max(np.abs(A.T @ T @ A - np.diag(d))) <= bar


def test_host_cholesky_inverse():
    rng = np.random.default_rng(3)
    for b in (1, 5, 16):
        W = rng.standard_normal((40, b))
        W /= np.linalg.norm(W, axis=0)
        if b > 2:
            W[:, 2] = W[:, 0]  # dependent: dropped
        G = np.zeros((16, 16), order="F")
        G[:b, :b] = W.T @ W
        out = np.zeros(256)
        out[0] = 2 * 56 * ec.U
        ndrop = _dense_hook(1, b, G, out)
        Ri = out.reshape(16, 16).T  # tile (a, c) at a + 16 c
        ref, nref, _ = ec.chol_inv(G[:b, :b], 2 * 56 * ec.U)
        assert ndrop == nref == (1 if b > 2 else 0)
        assert not Ri[b:].any() and not Ri[:, b:].any() and np.allclose(Ri[:b, :b], ref, rtol=1e-12, atol=0.0)
        Q = W @ Ri[:b, :b]
        keep = [c for c in range(b) if not (b > 2 and c == 2)]
        assert np.max(np.abs(Q[:, keep].T @ Q[:, keep] - np.eye(len(keep)))) < 1e-13
        if b > 2:
            assert not Q[:, 2].any()
