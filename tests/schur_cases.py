"""Inputs and dense references shared by the Schur-complement tests."""
import os

import numpy as np

import sparsecholesky_amd as sc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return sc.load_matrix_market_to_csc(os.path.join(GOLDEN, name + ".mtx"))


def plane(k, x):
    """Indices of the grid points of lap k^3 (natural order) whose fastest coordinate is x."""
    return np.nonzero(np.arange(k ** 3) % k == x)[0].astype(np.int32)


def random_set(n, ns, seed):
    """ns distinct indices, unsorted."""
    return np.random.default_rng(seed).permutation(n)[:ns].astype(np.int32)


def dense_spd(n, seed=5):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    D = M @ M.T + n * np.eye(n)
    i, j = np.triu_indices(n)
    return sc.triplet_to_csc_matrix(i.astype(np.int32), j.astype(np.int32), D[i, j], n)


def split(A, idx):
    """(A_II, A_IS, A_SS, interior) of the dense matrix of A for the index list idx."""
    M = sc.csc_to_dense(A)
    idx = np.asarray(idx, dtype=np.int64)
    mask = np.ones(M.shape[0], dtype=bool)
    mask[idx] = False
    I = np.nonzero(mask)[0]
    return M[np.ix_(I, I)], M[np.ix_(I, idx)], M[np.ix_(idx, idx)], I


def schur_refs(A, idx):
    """R1 = A_SS - A_IS^T solve(A_II, A_IS) by LU and R2, the same by Cholesky."""
    import scipy.linalg as sla

    AII, AIS, ASS, _ = split(A, idx)
    if AII.shape[0] == 0:
        return ASS.copy(), ASS.copy()
    R1 = ASS - AIS.T @ np.linalg.solve(AII, AIS)
    R2 = ASS - AIS.T @ sla.cho_solve(sla.cho_factor(AII, lower=True), AIS)
    return R1, R2


def bar(R1, R2, floor=1e-12):
    """The project's bar: max(floor, 100 x the references' disagreement)."""
    return max(floor, 100.0 * np.linalg.norm(R2 - R1) / np.linalg.norm(R1))
