"""What the eigensolver tests share: the inputs, a dense numpy model of the block shift-invert
Lanczos iteration that include/sparsecholesky.h documents, the library's start block in numpy,
and exact integer arithmetic for the two panel kernels' bounds.

The model is the yardstick of the GPU tests, so test_eigs_cases_cpu.py pins it: the same steps,
estimates and stopping rules as the header, with a dense Cholesky of F for the solves and
numpy's eigh for the projected matrix.
"""
import functools
from fractions import Fraction

import numpy as np

import sparsecholesky_amd as sc

import pcg_cases as pc
import refine_cases as rc

U = rc.U
CONVERGED, MAXBLOCKS, EXHAUSTED = range(3)
INPUTS = ("lap2", "lap4", "lap8", "lap8_nd", "bcsstk01", "bus_nd", "lap4_schur")


def gamma(m):
    return m * U / (1.0 - m * U)


# ---- inputs ----
@functools.lru_cache(maxsize=None)
def matrix(name):
    """name -> (upper CSC matrix, Symbolic keywords)."""
    if name == "lap2":
        return sc.laplacian3d(2, nd=False), {}
    if name == "lap4":
        return sc.laplacian3d(4, nd=False), {}
    return pc.matrix(name)


@functools.lru_cache(maxsize=None)
def dense(name):
    M = pc.dense(matrix(name)[0])
    M.setflags(write=False)
    return M


def start_uniform(n, seed=7):
    """A start block for X0 =: uniform(-1, 1), n x min(16, n)."""
    X = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, min(16, n)))
    X.setflags(write=False)
    return X


def start_library(n, seed=1):
    """The library's own start block (use_x0 = 0), entry for entry: splitmix64 of seed and 16 i + c."""
    b = min(16, n)
    with np.errstate(over="ignore"):
        k = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(16) + np.arange(b, dtype=np.uint64)[None, :]
             + np.uint64(1))
        z = np.uint64(seed) + k * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return 2.0 * ((z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


# ---- the model ----
def chol_inv(G, thr):
    """inv(R) of G = R^T R with the header's dropping rule, and the smallest pivot met."""
    b = G.shape[0]
    R = np.zeros((b, b))
    drop = np.zeros(b, dtype=bool)
    piv_min = np.inf
    for k in range(b):
        piv = G[k, k] - R[:k, k] @ R[:k, k]
        piv_min = min(piv_min, piv) if np.isfinite(piv) else -np.inf
        if not (piv > thr) or not np.isfinite(piv):
            drop[k] = True
            continue
        R[k, k] = np.sqrt(piv)
        R[k, k + 1:] = (G[k, k + 1:] - R[:k, k] @ R[:k, k + 1:]) / R[k, k]
    Ri = np.zeros((b, b))
    keep = np.nonzero(~drop)[0]
    if len(keep):
        Ri[np.ix_(keep, keep)] = np.linalg.inv(R[np.ix_(keep, keep)])
    return Ri, int(drop.sum()), piv_min


def emulate(Fd, nev, X0, tol=1e-10, max_blocks=32, sigma=0.0, wrong=None):
    """The documented algorithm in dense numpy.  Fd: the dense factored matrix F; X0: the start
    block (n x b).  wrong: None, or a deliberate mistake -- "one_pass" (a single Gram-Schmidt
    pass), "est_first" (the estimate from the first b entries of s instead of the last),
    "smallest" (the nev smallest theta wanted).  Returns a dict: lam, X, theta, est, resid, state
    (per pair), blocks, and the diagnostics min_pivot (smallest scaled pivot of a rank test) and
    orth (max |X^T X - I|)."""
    import scipy.linalg as sla

    n = Fd.shape[0]
    b = min(16, n)
    thr = 2.0 * (n + 16) * U
    cf = sla.cho_factor(Fd, lower=True)

    def orth(W):
        for _ in range(2):
            g = np.einsum("ij,ij->j", W, W)
            W = W * np.where(g > 0.0, 1.0 / np.sqrt(np.where(g > 0.0, g, 1.0)), 0.0)
            Ri, _, _ = chol_inv(W.T @ W, thr)
            W = W @ Ri
        return W

    V = [orth(np.array(X0[:, :b], dtype=np.float64))]
    T = np.zeros((b * max_blocks, b * max_blocks))
    min_pivot = np.inf
    j, capped = 0, False
    while True:
        W = sla.cho_solve(cf, V[j])
        Vall = np.hstack(V)
        H = np.zeros((b * (j + 1), b))
        for _ in range(1 if wrong == "one_pass" else 2):
            h = Vall.T @ W
            W = W - Vall @ h
            H += h
        m = b * (j + 1)
        H[m - b:] = 0.5 * (H[m - b:] + H[m - b:].T)
        T[:m, m - b:m] = H
        T[m - b:m, :m] = H.T
        G = W.T @ W
        theta, S = np.linalg.eigh(T[:m, :m])
        kw = min(nev, m)
        cols = np.arange(kw) if wrong == "smallest" else m - 1 - np.arange(kw)
        s = S[:b, cols] if wrong == "est_first" else S[m - b:, cols]
        est = np.sqrt(np.maximum(np.einsum("ai,ab,bi->i", s, G, s), 0.0))
        conv = kw == nev and bool(np.all(est <= tol * theta[cols]))
        if conv:
            break
        if j + 1 == max_blocks:
            capped = True
            break
        if m + b > n:
            break
        d = np.diag(G)
        if not np.all(d > 0.0):
            break
        _, ndrop, piv = chol_inv(G / np.sqrt(np.outer(d, d)), thr)
        min_pivot = min(min_pivot, piv)
        if ndrop:
            break
        V.append(orth(W))
        j += 1
    Vall = np.hstack(V)
    X = np.zeros((n, nev))
    lam = np.full(nev, np.inf)
    th = np.zeros(nev)
    e = np.full(nev, np.inf)
    X[:, :kw] = Vall @ S[:, cols]
    th[:kw] = theta[cols]
    with np.errstate(divide="ignore"):
        lam[:kw] = sigma + 1.0 / th[:kw]
    e[:kw] = est
    resid = np.full(nev, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        resid[:kw] = np.linalg.norm(Fd @ X[:, :kw] - X[:, :kw] / th[:kw], axis=0)
        ok = e <= tol * th
    state = np.where(ok, CONVERGED, MAXBLOCKS if capped else EXHAUSTED)
    return dict(lam=lam, X=X, theta=th, est=e, resid=resid, state=state, blocks=j + 1, min_pivot=min_pivot,
                orth=float(np.max(np.abs(X.T @ X - np.eye(nev)))) if nev else 0.0)


# ---- exact arithmetic for the two panel kernels ----
SCALE = 40  # test panels hold multiples of 2^-SCALE below 2^22: exact integers after scaling


def quantised(rng, shape):
    """Magnitudes over 2^-20 .. 2^20 with random signs, as multiples of 2^-SCALE."""
    a = rng.standard_normal(shape) * 2.0 ** rng.integers(-20, 21, shape)
    return np.round(np.ldexp(a, SCALE)) / 2.0 ** SCALE


def as_int(a):
    """A float array of multiples of 2^-SCALE as an object array of Python ints (times 2^SCALE)."""
    s = np.ldexp(np.asarray(a, dtype=np.float64), SCALE)
    assert np.all(s == np.floor(s)) and np.all(np.abs(s) < 2.0 ** 63)
    return s.astype(np.int64).astype(object)


def exact_matmul(A, B):
    """(A B, |A| |B|) exactly, as object arrays of ints scaled by 2^(2 SCALE)."""
    Ai, Bi = as_int(A), as_int(B)
    if Ai.shape[1] == 0:  # an empty sum
        zero = np.zeros((Ai.shape[0], Bi.shape[1]), dtype=object)
        return zero, zero
    return Ai @ Bi, np.abs(Ai) @ np.abs(Bi)


def within(fl, exact, bound_int, g, extra=None):
    """Entrywise |fl - exact / 2^(2 SCALE)| <= g (bound_int / 2^(2 SCALE) + extra), in rationals."""
    den = 1 << (2 * SCALE)
    g = Fraction(g)
    fl, exact, bound_int = np.asarray(fl), np.asarray(exact), np.asarray(bound_int)
    worst = 0.0
    for idx in np.ndindex(fl.shape):
        ex = Fraction(int(exact[idx]), den) + (Fraction(0) if extra is None else extra[0][idx])
        bd = g * (Fraction(int(bound_int[idx]), den) + (Fraction(0) if extra is None else extra[1][idx]))
        err = abs(Fraction(float(fl[idx])) - ex)
        if err == 0:
            continue
        if bd == 0:
            return float("inf")
        worst = max(worst, float(err / bd))
    return worst
