"""The three vector kernels of the conjugate gradients alone (sc_debug_pcg_vec), against
exact rational arithmetic.

Bounds (u = 2^-53), none taken from what the kernels give:
  * a sum of n products, in any order, fused or not: |fl - exact| <= gamma_n sum |u_i v_i|,
    gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability, section 3.1);
  * x + a p per entry: |fl - exact| <= u (|a p| + |x + a p|) (1 + u), which one rounding (fma)
    and two (product, then sum) both meet; the same for r - a q and z + b p.
The data cancels: magnitudes over 2^-20 .. 2^20 and v = +-u with alternating signs.
Shapes: n = 1, 5, 67; one below, at and above the 1024 rows of a workgroup; 2049, the smallest n
with three workgroup partials; nrhs 1, 15, 16; leading dimensions n and n + 3.  Padding rows
and the columns >= nrhs hold NaN and must come back untouched, masked columns bit for bit.
"""
import ctypes

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import pcg_cases as pc
from refine_cases import bits

pytestmark = pytest.mark.gpu

ROWS = 1024  # PCG_ROWS of kernels.hpp
SIZES = (1, 5, 67, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1)
DOT, UPDATE, DIR, DIR_FIRST = range(4)


def _dev(a, n, k, ld):
    """n x k host array as a 16 x ld device panel (column c at row c), NaN everywhere else."""
    h = np.full((16, ld), np.nan)
    h[:k, :n] = a.T
    return torch.tensor(h, device="cuda"), h


def _call(which, n, k, mask, coef, A, lda, B, ldb, C, ldc, D, ldd, T):
    out = np.full(32, np.nan)
    cf = None if coef is None else np.ascontiguousarray(coef, dtype=np.float64)
    ptr = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())  # noqa: E731
    rc = sc.lib().sc_debug_pcg_vec(which, n, k, mask, None if cf is None else cf.ctypes.data_as(ctypes.c_void_p),
                                   ptr(A), lda, ptr(B), ldb, ptr(C), ldc, ptr(D), ldd, ptr(T),
                                   out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, sc.lib().sc_last_error()
    return out


def _mask(k):
    """All columns but column 0 (when there are several) and one in the middle."""
    m = (1 << k) - 1
    if k > 1:
        m &= ~1
    if k > 4:
        m &= ~(1 << (k // 2))
    return m | (1 << 20)  # a bit past nrhs is ignored


def _untouched(t, h0, n, k, cols):
    """Padding, the columns >= k and the listed columns of t hold the bits of h0."""
    h = t.cpu().numpy()
    assert np.array_equal(bits(h[k:]), bits(h0[k:])) and np.array_equal(bits(h[:, n:]), bits(h0[:, n:]))
    for c in cols:
        assert np.array_equal(bits(h[c]), bits(h0[c])), c
    return h


@pytest.mark.parametrize("k", [1, 15, 16])
@pytest.mark.parametrize("n", SIZES)
def test_dot(gpu, n, k):
    u, v, w = pc.cancelling(n, k, seed=100 * n + k)
    mask = _mask(k)
    off = [c for c in range(k) if not (mask >> c) & 1]
    for ld in (n, n + 3):
        dU, hU = _dev(u, n, k, ld)
        dV, hV = _dev(v, n, k, ld + 1)
        dW, hW = _dev(w, n, k, ld)
        two = _call(DOT, n, k, mask, None, dU, ld, dV, ld + 1, dW, ld, None, 0, None)
        one = _call(DOT, n, k, mask, None, dU, ld, dV, ld + 1, None, 0, None, 0, None)
        assert np.array_equal(bits(two), bits(_call(DOT, n, k, mask, None, dU, ld, dV, ld + 1, dW, ld, None, 0, None)))
        assert np.array_equal(bits(one[:16]), bits(two[:16])) and not one[16:].any()
        for t, h in ((dU, hU), (dV, hV), (dW, hW)):
            _untouched(t, h, n, k, range(k))
        for c in range(16):
            if c >= k or c in off:
                assert two[c] == 0.0 and two[16 + c] == 0.0
            else:
                assert pc.dot_within(two[c], u[:, c], v[:, c]), (c, two[c])
                assert pc.dot_within(two[16 + c], u[:, c], w[:, c]), (c, two[16 + c])
    # every column alone gives the bits it has in company
    full = _call(DOT, n, k, (1 << k) - 1, None, dU, ld, dV, ld + 1, dW, ld, None, 0, None)
    c = k - 1
    alone = _call(DOT, n, k, 1 << c, None, dU, ld, dV, ld + 1, dW, ld, None, 0, None)
    assert bits(alone)[c] == bits(full)[c] and bits(alone)[16 + c] == bits(full)[16 + c]


@pytest.mark.parametrize("k", [1, 15, 16])
@pytest.mark.parametrize("n", SIZES)
def test_update(gpu, n, k):
    x, p, r = pc.cancelling(n, k, seed=7 * n + k)
    q = pc.cancelling(n, k, seed=11 * n + k)[2]
    alpha = np.random.default_rng(n + k).standard_normal(16) * 4.0
    mask = _mask(k)
    off = [c for c in range(k) if not (mask >> c) & 1]
    for ld in (n, n + 3):
        res = []
        for _ in range(2):
            dX, hX = _dev(x, n, k, ld)
            dR, hR = _dev(r, n, k, ld + 2)
            dP, hP = _dev(p, n, k, ld)
            dQ, hQ = _dev(q, n, k, ld + 1)
            out = _call(UPDATE, n, k, mask, alpha, dX, ld, dR, ld + 2, dP, ld, dQ, ld + 1, None)
            X = _untouched(dX, hX, n, k, off)
            R = _untouched(dR, hR, n, k, off)
            _untouched(dP, hP, n, k, range(k))
            _untouched(dQ, hQ, n, k, range(k))
            res.append((X, R, out))
        for a, b in zip(res[0], res[1]):
            assert np.array_equal(bits(a), bits(b))
        X, R, out = res[0]
        assert not out[16:].any()
        worst = 0.0
        for c in range(16):
            if c >= k or c in off:
                assert out[c] == 0.0
                continue
            worst = max(worst, pc.axpy_worst(X[c, :n], alpha[c], p[:, c], x[:, c]),
                        pc.axpy_worst(R[c, :n], -alpha[c], q[:, c], r[:, c]))
            assert pc.dot_within(out[c], R[c, :n], R[c, :n]), (c, out[c])
        print(f"PCG update n {n} nrhs {k} ld {ld}: worst error / bound {worst:.3f} (<= 1)")
        assert worst <= 1.0


@pytest.mark.parametrize("k", [1, 15, 16])
@pytest.mark.parametrize("n", SIZES)
def test_direction(gpu, n, k):
    p, _, z = pc.cancelling(n, k, seed=13 * n + k)
    beta = np.abs(np.random.default_rng(n + k).standard_normal(16)) + 0.1
    mask = _mask(k)
    off = [c for c in range(k) if not (mask >> c) & 1]
    for ld in (n, n + 3):
        for which in (DIR, DIR_FIRST):
            res = []
            for with_t in (True, True, False):
                # a first direction starts from garbage: NaN in p must not reach the result
                dP, hP = _dev(np.full_like(p, np.nan) if which == DIR_FIRST else p, n, k, ld)
                dZ, hZ = _dev(z, n, k, ld + 1)
                dT = torch.full((n, 16), float("nan"), dtype=torch.float64, device="cuda") if with_t else None
                _call(which, n, k, mask, None if which == DIR_FIRST else beta, dP, ld, None, 0, dZ, ld + 1, None, 0, dT)
                P = _untouched(dP, hP, n, k, off)
                _untouched(dZ, hZ, n, k, range(k))
                res.append(P)
                if with_t:
                    T = dT.cpu().numpy()
                    for c in range(16):
                        if c >= k or c in off:
                            assert not T[:, c].any(), c  # zeros: the product must not meet a NaN
                        else:  # the row-major copy is the column-major result, bit for bit
                            assert np.array_equal(bits(T[:, c]), bits(P[c, :n])), c
            assert np.array_equal(bits(res[0]), bits(res[1])) and np.array_equal(bits(res[0]), bits(res[2]))
            P = res[0]
            for c in range(k):
                if c in off:
                    continue
                if which == DIR_FIRST:
                    assert np.array_equal(bits(P[c, :n]), bits(z[:, c]))
                else:
                    assert pc.axpy_worst(P[c, :n], beta[c], p[:, c], z[:, c]) <= 1.0, c


def test_arguments_are_validated_before_a_launch(gpu):
    L = sc.lib()
    t = torch.zeros((16, 8), dtype=torch.float64, device="cuda")
    out, coef = np.zeros(32), np.zeros(16)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    d = ctypes.c_void_p(t.data_ptr())

    def call(which=0, n=8, k=2, cf=P(coef), a=d, lda=8, b=d, ldb=8, c=d, ldc=8, dd=d, ldd=8, o=P(out)):
        return L.sc_debug_pcg_vec(which, n, k, 3, cf, a, lda, b, ldb, c, ldc, dd, ldd, None, o)

    bad = [(lambda: call(which=4), b"unknown kernel"), (lambda: call(which=-1), b"unknown kernel"),
           (lambda: call(n=-1), b"n < 0 or nrhs outside [0, 16]"), (lambda: call(k=17), b"nrhs outside [0, 16]"),
           (lambda: call(a=None), b"null array"), (lambda: call(b=None), b"null array"),
           (lambda: call(o=None), b"null array"), (lambda: call(which=1, cf=None), b"null array"),
           (lambda: call(which=1, dd=None), b"null array"), (lambda: call(which=2, c=None), b"null array"),
           (lambda: call(which=2, cf=None), b"null array"),
           (lambda: call(lda=7), b"leading dimension below n"), (lambda: call(ldb=7), b"leading dimension below n"),
           (lambda: call(ldc=7), b"leading dimension below n"),
           (lambda: call(which=1, ldd=7), b"leading dimension below n")]
    for f, text in bad:
        assert f() == -1, text
        assert b"sc_debug_pcg_vec: " + text in L.sc_last_error() or text in L.sc_last_error(), L.sc_last_error()
    out[:] = 5.0
    assert call(n=0, a=None, b=None, c=None) == 0 and not out.any()
    out[:] = 5.0
    assert call(k=0, a=None, b=None, c=None) == 0 and not out.any()
    assert not t.cpu().numpy().any()
