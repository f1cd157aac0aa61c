"""The two kernels of one block step of the rank-k update / downdate (sc_debug_updown_block)
on caller data, against long double.

With X = [L W] the rows [k0, m) of the block's columns and of the workspace as given, Y what
the kernels left (K = nb + 16 columns each) and J = diag(I_nb, sign I_16), the step must give
    Y J Y^T = X J X^T,   Y's first nb rows = [L11' 0] with L11' lower triangular, diagonal > 0,
which determines Y's L part (the Cholesky factor is unique) and, with T = the transform the
elimination order fixes, its W part.  The first is checked entry by entry in long double,
the second bitwise (zeros) and by sign.

The bound is derived, not measured.  u = 2^-53.  The block kernel pushes every row -- the
block's own and the rows of the identity that become T -- through the rotations one after
the other.  One application of a computed rotation to a pair commits at most 6 u times the
pair's norm (Higham, Accuracy and Stability of Numerical Algorithms, Lemma 19.8: gamma_6
covers the coefficients' own errors).  Row x meets, per pivot j, the pairs (L_j, W_c), c <
16, whose norms sum to at most 16 |L_j| + 4 |W|_2; over the nb pivots that is at most
(16 sqrt(nb) + 4 nb) |x|_2 <= 4.8 K |x|_2 for nb <= 64.  So a row of the computed T is a row
of an exactly J-orthogonal matrix plus an error of norm at most 6 * 4.8 K u = 29 K u (times
tau^2 for hyperbolic rotations, below), a row x T of the MFMA product differs from x times
that matrix by at most 29 K u tau^2 |x|_1 plus the product's own gamma_K tau |x|_2, and the
Gram entry (i, p) by
    K u tau^2 (29 (|x_i|_1 |x_p|_2 + |x_i|_2 |x_p|_1) + 2 |x_i|_2 |x_p|_2)
to first order: the multiple is 29 = 6 * 4.8 on the mixed 1-norm / 2-norm terms and 2 on the
product.  tau = |T|_2: 1 for an update; for a downdate sqrt((1 + t) / (1 - t)) with t^2 the
largest eigenvalue of W1^T (L11 L11^T)^-1 W1, which the data fixes at 1/2: tau = 1 + sqrt(2).
An indexing error, a dropped rotation or a wrong sign shows as O(1), fourteen orders above.

Operands start one double into their allocations and m is odd and even; everything the
kernels must not write -- rows above k0, other columns, the strict upper triangle of the
diagonal block, lead-in and canaries -- is compared bitwise."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc
import zoo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
CANARY = 8
KW = 16
ZERO_COLS = (3, 7, 12)  # columns of W with exact zeros on the block's pivot rows
SHAPES = [(64, 64, 0), (65, 64, 0), (200, 100, 64), (321, 130, 128), (1000, 64, 0)]


def _dev(host):
    return torch.tensor(host, device="cuda", dtype=torch.float64)


def _ptr(t, first):
    return ctypes.c_void_p(t.data_ptr() + 8 * first)


@functools.lru_cache(maxsize=None)
def _case(m, w, k0):
    """Host buffers of the panel (column-major, ld = m) and the workspace (row-major m x 16),
    each with a lead-in double and canaries, everything random; the block's triangle has its
    diagonal in [1, 2] and off-diagonals uniform / sqrt(m) like the rows below; W is scaled so
    that the largest eigenvalue of W1^T (L11 L11^T)^-1 W1 is 1/2 (a downdate stays positive
    definite, safely)."""
    zoo.require_long_double()
    nb = min(64, w - k0)
    rng = np.random.default_rng(1000 * m + 10 * w + k0)
    fbuf = rng.uniform(-1, 1, 1 + m * w + CANARY)
    F = fbuf[1:1 + m * w].reshape(w, m).T
    F[k0:, k0:k0 + nb] /= np.sqrt(m)
    F[k0 + np.arange(nb), k0 + np.arange(nb)] = rng.uniform(1, 2, nb)
    wbuf = rng.standard_normal(1 + m * KW + CANARY)
    W = wbuf[1:1 + m * KW].reshape(m, KW)
    W[k0:k0 + nb, ZERO_COLS] = 0.0
    L11 = np.tril(F[k0:k0 + nb, k0:k0 + nb])
    Kmat = np.linalg.solve(L11, W[k0:k0 + nb])
    W[k0:] *= np.sqrt(0.5) / np.linalg.norm(Kmat, 2)
    fbuf.setflags(write=False)
    wbuf.setflags(write=False)
    return fbuf, wbuf, nb


def _rows(fbuf, wbuf, m, w, k0, nb):
    """X = [L W] over rows [k0, m): the block's columns with the strict upper triangle of the
    diagonal block read as zero, and the workspace."""
    F = fbuf[1:1 + m * w].reshape(w, m).T
    W = wbuf[1:1 + m * KW].reshape(m, KW)
    Lb = F[k0:, k0:k0 + nb].copy()
    Lb[:nb][np.triu(np.ones((nb, nb), dtype=bool), 1)] = 0.0
    return np.hstack([Lb, W[k0:]])


def _eliminate_ld(X, nb, sign):
    """The same elimination in long double: pivot by pivot, column of W by column of W."""
    Y = X.astype(LD)
    for j in range(nb):
        for c in range(KW):
            a, b = Y[j, j], Y[j, nb + c]
            if b == 0:
                continue
            r = np.sqrt(a * a + sign * b * b)
            cs, sn = a / r, b / r
            l, v = Y[j:, j].copy(), Y[j:, nb + c].copy()
            Y[j:, j] = cs * l + sign * sn * v
            Y[j:, nb + c] = cs * v - sn * l
    return Y


@pytest.mark.parametrize("sign", [1, -1], ids=["update", "downdate"])
@pytest.mark.parametrize("m,w,k0", SHAPES, ids=[f"m{m}-w{w}-k{k}" for m, w, k in SHAPES])
def test_block_step(gpu, m, w, k0, sign):
    fbuf, wbuf, nb = _case(m, w, k0)
    K = nb + KW
    dF, dW = _dev(fbuf), _dev(wbuf)
    info = ctypes.c_int32(-1)
    rc = sc.lib().sc_debug_updown_block(_ptr(dF, 1), m, w, k0, _ptr(dW, 1), sign, ctypes.byref(info))
    assert rc == 0 and info.value == 0, (rc, info.value)
    fout, wout = dF.cpu().numpy(), dW.cpu().numpy()
    X = _rows(fbuf, wbuf, m, w, k0, nb)
    Y = _rows(fout, wout, m, w, k0, nb)
    # the structure: W1' exactly zero, the diagonal positive
    assert np.all(Y[:nb, nb:] == 0.0)
    assert np.all(np.diag(Y[:nb, :nb]) > 0)
    # the Gram identity, entry by entry, in long double
    J = np.concatenate([np.ones(nb), sign * np.ones(KW)]).astype(LD)
    Xl, Yl = X.astype(LD), Y.astype(LD)
    res = np.abs((Yl * J) @ Yl.T - (Xl * J) @ Xl.T)
    tau = LD(1.0) if sign > 0 else 1 + np.sqrt(LD(2.0))
    n1, n2 = np.abs(Xl).sum(axis=1), np.sqrt((Xl * Xl).sum(axis=1))
    bound = K * U * tau * tau * (29 * (np.outer(n1, n2) + np.outer(n2, n1)) + 2 * np.outer(n2, n2))
    ratio = float((res / bound).max())
    # for information: the distance to the same elimination in long double (it also carries
    # the conditioning of the update, so it is printed, not asserted)
    ref = _eliminate_ld(X, nb, sign)
    fwd = float(np.abs(Yl - ref).max() / np.abs(ref).max())
    print(f"KERNEL updown sign={sign:+d} m={m} w={w} k0={k0} nb={nb}: worst Gram residual / bound {ratio:.3f}; "
          f"max |Y - Y_ld| / max |Y_ld| = {fwd:.2e}")
    assert ratio <= 1.0, ratio
    # a column of W with exact zeros on the pivot rows is inactive: its part of the transform
    # is exactly the identity, and its entries in the rows below come back bit for bit
    Win = wbuf[1:1 + m * KW].reshape(m, KW)
    Wout = wout[1:1 + m * KW].reshape(m, KW)
    assert np.array_equal(Wout[k0 + nb:, ZERO_COLS].view(np.int64), Win[k0 + nb:, ZERO_COLS].view(np.int64))
    if m > k0 + nb:  # the active columns did change
        assert not np.array_equal(Wout[k0 + nb:, 0], Win[k0 + nb:, 0])
    # nothing else written: put the written region back and compare everything bitwise
    kept = fout.copy()
    Fk = kept[1:1 + m * w].reshape(w, m).T
    Fi = fbuf[1:1 + m * w].reshape(w, m).T
    low = np.tril(np.ones((m - k0, nb), dtype=bool))
    Fk[k0:, k0:k0 + nb][low] = Fi[k0:, k0:k0 + nb][low]
    assert np.array_equal(kept.view(np.int64), fbuf.view(np.int64))
    keptw = wout.copy()
    keptw[1:1 + m * KW].reshape(m, KW)[k0:] = Win[k0:]
    assert np.array_equal(keptw.view(np.int64), wbuf.view(np.int64))


def test_block_step_is_repeatable_bitwise(gpu):
    m, w, k0 = 321, 130, 64
    fbuf, wbuf, nb = _case(m, w, k0)
    outs = []
    for _ in range(2):
        dF, dW = _dev(fbuf), _dev(wbuf)
        info = ctypes.c_int32(-1)
        assert sc.lib().sc_debug_updown_block(_ptr(dF, 1), m, w, k0, _ptr(dW, 1), -1, ctypes.byref(info)) == 0
        outs.append((dF.cpu().numpy(), dW.cpu().numpy()))
    assert np.array_equal(outs[0][0].view(np.int64), outs[1][0].view(np.int64))
    assert np.array_equal(outs[0][1].view(np.int64), outs[1][1].view(np.int64))


@pytest.mark.parametrize("p", [0, 35])
def test_failing_downdate_reports_the_column(gpu, p):
    # W1 = alpha e_p on one column with alpha^2 = 2 L(p, p)^2: exactly that pivot fails; the
    # status word is the column of the panel + 1 and the block is not written
    m, w, k0 = 200, 100, 64
    fbuf, wbuf, nb = _case(m, w, k0)
    F = fbuf[1:1 + m * w].reshape(w, m).T
    wb = wbuf.copy()
    W = wb[1:1 + m * KW].reshape(m, KW)
    W[k0:] = 0.0
    W[k0 + p, 5] = np.sqrt(2.0) * F[k0 + p, k0 + p]
    dF, dW = _dev(fbuf), _dev(wb)
    info = ctypes.c_int32(-1)
    assert sc.lib().sc_debug_updown_block(_ptr(dF, 1), m, w, k0, _ptr(dW, 1), -1, ctypes.byref(info)) == 0
    assert info.value == k0 + p + 1
    assert np.array_equal(dF.cpu().numpy().view(np.int64), fbuf.view(np.int64))


def test_bad_arguments_are_refused_before_any_launch(gpu):
    L = sc.lib()
    fbuf, wbuf, _ = _case(64, 64, 0)
    dF, dW = _dev(fbuf), _dev(wbuf)
    info = ctypes.c_int32(-1)
    for m, w, k0, sign in ((64, 64, 0, 0), (64, 64, 32, 1), (64, 64, 64, 1), (64, 65, 0, 1), (0, 0, 0, 1)):
        assert L.sc_debug_updown_block(_ptr(dF, 1), m, w, k0, _ptr(dW, 1), sign, ctypes.byref(info)) == -1
    assert L.sc_debug_updown_block(None, 64, 64, 0, _ptr(dW, 1), 1, ctypes.byref(info)) == -1
