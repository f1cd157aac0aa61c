"""The two panel kernels of the eigensolver alone (sc_debug_eigs_gram, sc_debug_eigs_update),
against exact integer arithmetic.

Bounds (u = 2^-53, gamma_k = k u / (1 - k u); Higham, Accuracy and Stability, section 3.1), none
taken from what the kernels give:
  * Gram: |G - exact| <= gamma_n sum |v| |w| entrywise -- a sum of n products in any order,
    fused or not;
  * update: |Out - exact| <= gamma_{16 nb + 2} (|beta w| + sum |v| |c|): 16 nb products summed
    onto the rounded beta w, in any order.
The data cancels: magnitudes over 2^-20 .. 2^20 with random signs, quantised to 2^-40 so that
integers hold every product exactly.
Shapes: n = 0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 257 (the 4 rows of an MFMA step, the 16 of a
tile, the 64 of a wave, the 256 of a staged chunk, each with its neighbours), 1023 and 1025 (the
1024 rows of a Gram workgroup -1 / +1) and 2053 (three workgroup partials, the last one short);
nb 1, 2, 5; b 1, 5, 16; leading dimensions n and n + 3 with NaN in the padding rows and in the
columns >= b, which must come back untouched (and a NaN read would poison the result).
"""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import eigs_cases as ec
from refine_cases import bits

pytestmark = pytest.mark.gpu

ROWS = 1024  # EIGS_ROWS of kernels.hpp
SIZES = (0, 1, 3, 4, 15, 16, 17, 63, 64, 65, 257, ROWS - 1, ROWS + 1, 2 * ROWS + 5)


def _basis(a, ld):
    """(n, b, nb) host array as an (nb, 16, ld) device basis, NaN everywhere else."""
    n, b, nb = a.shape
    h = np.full((nb, 16, max(ld, 1)), np.nan)
    h[:, :b, :n] = a.transpose(2, 1, 0)
    return torch.tensor(h, device="cuda"), h


def _panel(a, ld):
    t, h = _basis(a[:, :, None], ld)
    return t, h


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _gram(n, b, nb, dV, ldv, dW, ldw, vstride=None):
    out = np.full(256 * max(nb, 1), np.nan)
    rc = sc.lib().sc_debug_eigs_gram(n, b, nb, _ptr(dV), ldv, 16 * ldv if vstride is None else vstride, _ptr(dW), ldw,
                                     out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, sc.lib().sc_last_error()
    return out[:256 * nb].reshape(nb, 16, 16).transpose(0, 2, 1)  # [i][a][c]


def _update(n, b, bc, nb, beta, dOut, ldo, dW, ldw, dV, ldv, C):
    """C: (nb, 16, 16) host, [i][a][c]."""
    tiles = np.ascontiguousarray(np.asarray(C, dtype=np.float64).transpose(0, 2, 1)).reshape(-1)
    rc = sc.lib().sc_debug_eigs_update(n, b, bc, nb, beta, _ptr(dOut), ldo, _ptr(dW), ldw, _ptr(dV), ldv, 16 * ldv,
                                       tiles.ctypes.data_as(ctypes.c_void_p) if tiles.size else None)
    assert rc == 0, sc.lib().sc_last_error()


@pytest.mark.parametrize("n", SIZES)
def test_gram(gpu, n):
    rng = np.random.default_rng(1000 + n)
    for nb, b, pad in ((1, 16, 0), (2, 5, 3), (5, 1, 3), (5, 16, 3)):
        ld = max(n + pad, 1)
        V = ec.quantised(rng, (n, b, nb))
        W = ec.quantised(rng, (n, b))
        dV, hV = _basis(V, ld)
        dW, hW = _panel(W, ld + 1)
        G = _gram(n, b, nb, dV, ld, dW, ld + 1)
        assert np.array_equal(bits(G), bits(_gram(n, b, nb, dV, ld, dW, ld + 1)))
        assert np.array_equal(bits(dV.cpu().numpy()), bits(hV)) and np.array_equal(bits(dW.cpu().numpy()), bits(hW))
        assert not G[:, b:].any() and not G[:, :, b:].any() and np.all(np.isfinite(G))
        worst = 0.0
        for i in range(nb):
            ex, ab = ec.exact_matmul(V[:, :, i].T, W)
            worst = max(worst, ec.within(G[i, :b, :b], ex, ab, ec.gamma(max(n, 1))))
            # the block alone gives the bits it has in company
            one = _gram(n, b, 1, dV[i], ld, dW, ld + 1)
            assert np.array_equal(bits(one[0]), bits(G[i])), (nb, b, i)
        print(f"eigs gram n {n} nb {nb} b {b} ld {ld}: worst error / bound {worst:.3f} (<= 1)")
        assert worst <= 1.0
    # W^T W through the same kernel: V = W
    G = _gram(n, b, 1, dW, ld + 1, dW, ld + 1)
    ex, ab = ec.exact_matmul(W.T, W)
    assert ec.within(G[0, :b, :b], ex, ab, ec.gamma(max(n, 1))) <= 1.0


def _update_case(rng, n, nb, b, bc, beta, pad):
    ld = max(n + pad, 1)
    V = ec.quantised(rng, (n, b, nb))
    W = ec.quantised(rng, (n, bc))
    C = np.zeros((nb, 16, 16))
    C[:, :b, :bc] = ec.quantised(rng, (nb, b, bc))
    Cn = np.array(C)
    Cn[:, b:, :] = np.nan  # never read
    Cn[:, :, bc:] = np.nan
    ex, ab = ec.exact_matmul(V.transpose(0, 2, 1).reshape(n, nb * b), C[:, :b, :bc].reshape(nb * b, bc))
    fb = Fraction(beta)
    bw = np.array([[fb * Fraction(float(W[i, c])) for c in range(bc)] for i in range(n)], dtype=object).reshape(n, bc)
    return ld, V, W, Cn, ex, ab, (bw, np.abs(bw))


@pytest.mark.parametrize("n", SIZES)
def test_update(gpu, n):
    rng = np.random.default_rng(2000 + n)
    for nb, b, bc, beta, pad in ((1, 16, 16, 0.0, 0), (2, 5, 5, 1.0, 3), (5, 16, 6, -0.75, 3), (5, 1, 1, 1.0, 3),
                                 (2, 5, 16, 0.5, 0)):
        ld, V, W, C, ex, ab, extra = _update_case(rng, n, nb, b, bc, beta, pad)
        dV, hV = _basis(V, ld)
        res = []
        for inplace in (False, False, True):
            # beta == 0: W is not read, so it may hold anything
            dW, hW = _panel(np.full_like(W, np.nan) if beta == 0.0 else W, ld + 1)
            dO, hO = (dW, hW) if inplace else _panel(np.full((n, bc), np.nan), ld + 2)
            ldo = ld + 1 if inplace else ld + 2
            _update(n, b, bc, nb, beta, dO, ldo, dW, ld + 1, dV, ld, C)
            O = dO.cpu().numpy()[0]
            assert np.array_equal(bits(O[bc:]), bits(hO[0][bc:])) and np.array_equal(bits(O[:, n:]), bits(hO[0][:, n:]))
            assert np.array_equal(bits(dV.cpu().numpy()), bits(hV))
            if not inplace:
                assert np.array_equal(bits(dW.cpu().numpy()), bits(hW))
            res.append(O[:bc, :n].T)
        assert np.array_equal(bits(res[0]), bits(res[1])) and np.array_equal(bits(res[0]), bits(res[2]))
        assert np.all(np.isfinite(res[0]))
        worst = ec.within(res[0], ex, ab, ec.gamma(16 * nb + 2), extra=extra)
        print(f"eigs update n {n} nb {nb} b {b} bc {bc} beta {beta} ld {ld}: worst error / bound {worst:.3f} (<= 1)")
        assert worst <= 1.0


@pytest.mark.parametrize("n", (1, 17, 257, ROWS + 1))
def test_update_in_place_with_its_own_block(gpu, n):
    """W <- W C (the CholQR scaling): Out = V_0, and Out = a later block of a longer basis."""
    rng = np.random.default_rng(3000 + n)
    for nb, k in ((1, 0), (3, 1)):
        ld, V, _, C, ex, ab, _ = _update_case(rng, n, nb, 16, 16, 0.0, 3)
        dV, _ = _basis(V, ld)
        dO, _ = _panel(np.full((n, 16), np.nan), ld)
        _update(n, 16, 16, nb, 0.0, dO, ld, None, 0, dV, ld, C)
        _update(n, 16, 16, nb, 0.0, dV[k], ld, None, 0, dV, ld, C)
        assert np.array_equal(bits(dV[k].cpu().numpy()[:, :n]), bits(dO.cpu().numpy()[0][:, :n]))
        assert ec.within(dO.cpu().numpy()[0][:, :n].T, ex, ab, ec.gamma(16 * nb + 2)) <= 1.0


def test_empty_sums_and_sizes(gpu):
    W = ec.quantised(np.random.default_rng(5), (9, 4))
    dW, hW = _panel(W, 12)
    dO, hO = _panel(np.full((9, 4), np.nan), 12)
    _update(9, 0, 4, 3, 2.0, dO, 12, dW, 12, None, 0, np.zeros((0, 16, 16)))  # blocks of no column: Out = beta W
    assert np.array_equal(dO.cpu().numpy()[0][:4, :9].T, 2.0 * W)
    _update(9, 5, 4, 0, 0.0, dO, 12, None, 0, None, 0, np.zeros((0, 16, 16)))  # no block, beta 0: zeros
    O = dO.cpu().numpy()[0]
    assert not O[:4, :9].any() and np.array_equal(bits(O[4:]), bits(hO[0][4:]))
    _update(0, 5, 4, 2, 1.0, None, 0, None, 0, None, 0, np.zeros((2, 16, 16)))
    assert not _gram(0, 5, 2, None, 0, None, 0).any() and not _gram(9, 0, 2, None, 0, None, 0).any()


def test_arguments_are_validated_before_a_launch(gpu):
    L = sc.lib()
    t = torch.zeros((3, 16, 8), dtype=torch.float64, device="cuda")
    d = ctypes.c_void_p(t.data_ptr())
    out, C = np.zeros(3 * 256), np.zeros(3 * 256)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def gram(n=8, b=4, nb=2, v=d, ldv=8, vs=128, w=d, ldw=8, o=P(out)):
        return L.sc_debug_eigs_gram(n, b, nb, v, ldv, vs, w, ldw, o)

    def upd(n=8, b=4, bc=4, nb=2, beta=1.0, o=d, ldo=8, w=d, ldw=8, v=d, ldv=8, vs=128, c=P(C)):
        return L.sc_debug_eigs_update(n, b, bc, nb, beta, o, ldo, w, ldw, v, ldv, vs, c)

    bad = [(lambda: gram(n=-1), b"n < 0 or b outside [0, 16]"), (lambda: gram(b=17), b"b outside [0, 16]"),
           (lambda: gram(nb=-1), b"nb outside [0, 64]"), (lambda: gram(nb=65), b"nb outside [0, 64]"),
           (lambda: gram(v=None), b"null array"), (lambda: gram(w=None), b"null array"),
           (lambda: gram(o=None), b"null array"), (lambda: gram(ldv=7), b"leading dimension below n"),
           (lambda: gram(ldw=7), b"leading dimension below n"), (lambda: gram(vs=31), b"blocks of V closer"),
           (lambda: upd(n=-1), b"n < 0 or b outside [0, 16]"), (lambda: upd(bc=17), b"bc outside [0, 16]"),
           (lambda: upd(nb=65), b"nb outside [0, 64]"), (lambda: upd(o=None), b"null array"),
           (lambda: upd(w=None), b"null array"), (lambda: upd(v=None), b"null array"),
           (lambda: upd(c=None), b"null array"), (lambda: upd(ldo=7), b"leading dimension below n"),
           (lambda: upd(ldw=7), b"leading dimension below n"), (lambda: upd(ldv=7), b"leading dimension below n"),
           (lambda: upd(vs=31), b"blocks of V closer")]
    for f, text in bad:
        assert f() == -1, text
        assert text in L.sc_last_error(), L.sc_last_error()
    assert b"sc_debug_eigs_update: " in L.sc_last_error()
    assert upd(beta=0.0, w=None, ldw=0) == 0  # beta 0: W is not needed
    assert not t.cpu().numpy().any()
