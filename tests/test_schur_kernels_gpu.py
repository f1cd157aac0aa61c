"""The Schur complement's product kernel alone (sc_debug_schur_llt): S = D D^T for a lower
triangular D, on caller data.

D is random in its lower triangle and NaN above the diagonal, so a clean result proves that
nothing above the diagonal is used: neither in the diagonal K tile of a tile column nor for
the rows of a diagonal tile, and that K stops where the triangle does.  Sizes cover one
partial tile, the MFMA edge 16, the tile edge 64, several tiles and tails of both.

Bound, entry by entry: S(i, j) is a dot product of length min(i, j) + 1, so for any order
of summation, with or without fused multiply-adds (Higham, Accuracy and Stability, section 3.1),
    |S - ref| <= gamma_{min(i,j)+1} (|D| |D|^T)_ij,   gamma_k = k u / (1 - k u),   u = 2^-53,
with the reference in long double.  Both leading dimensions exceed ns and both buffers sit
between canaries; the padding rows of S must come back untouched."""
import ctypes

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc
import zoo

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = LD(2.0) ** -53
CANARY = 8
SIZES = [1, 15, 16, 17, 63, 64, 65, 129, 200, 515]


def _run(dbuf, ns, ldd, lds, sfill):
    dD = torch.tensor(dbuf, device="cuda", dtype=torch.float64)
    dS = torch.tensor(sfill, device="cuda", dtype=torch.float64)
    rc = sc.lib().sc_debug_schur_llt(ctypes.c_void_p(dD.data_ptr() + 8 * CANARY), ns, ldd,
                                     ctypes.c_void_p(dS.data_ptr() + 8 * CANARY), lds)
    assert rc == 0, rc
    return dD.cpu().numpy(), dS.cpu().numpy()


@pytest.mark.parametrize("ns", SIZES)
def test_product_against_long_double(gpu, ns):
    zoo.require_long_double()
    ldd, lds = ns + 5, ns + 3
    rng = np.random.default_rng(ns)
    dbuf = rng.standard_normal(2 * CANARY + ldd * ns)
    Dv = dbuf[CANARY:CANARY + ldd * ns].reshape(ns, ldd).T  # Dv[i, j], i < ldd
    Dv[:ns][np.triu(np.ones((ns, ns), dtype=bool), 1)] = np.nan
    D = np.tril(np.nan_to_num(Dv[:ns], nan=0.0))
    sfill = rng.standard_normal(2 * CANARY + lds * ns)
    dout, sout = _run(dbuf, ns, ldd, lds, sfill)
    # the input and everything around the window of S come back bit for bit
    assert np.array_equal(dout.view(np.int64), dbuf.view(np.int64))
    Sv = sout[CANARY:CANARY + lds * ns].reshape(ns, lds).T
    Fv = sfill[CANARY:CANARY + lds * ns].reshape(ns, lds).T
    assert np.array_equal(Sv[ns:].view(np.int64), Fv[ns:].view(np.int64))
    assert np.array_equal(sout[:CANARY].view(np.int64), sfill[:CANARY].view(np.int64))
    assert np.array_equal(sout[-CANARY:].view(np.int64), sfill[-CANARY:].view(np.int64))
    S = Sv[:ns]
    assert np.all(np.isfinite(S))
    assert np.array_equal(S, S.T)
    ref = D.astype(LD) @ D.astype(LD).T
    mag = np.abs(D).astype(LD) @ np.abs(D).astype(LD).T
    k = (np.minimum.outer(np.arange(ns), np.arange(ns)) + 1).astype(LD)
    bound = k * U / (1 - k * U) * mag
    err = np.abs(S.astype(LD) - ref)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print(f"KERNEL schur_llt ns={ns} ldd={ldd} lds={lds}: worst |S - ref| / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio
    # a second run gives the same bits
    _, sout2 = _run(dbuf, ns, ldd, lds, sfill)
    assert np.array_equal(sout2.view(np.int64), sout.view(np.int64))


def test_argument_checks(gpu):
    d = torch.zeros(64, device="cuda", dtype=torch.float64)
    p = ctypes.c_void_p(d.data_ptr())
    L = sc.lib()
    assert L.sc_debug_schur_llt(p, 4, 3, p, 4) == -1
    assert L.sc_debug_schur_llt(p, 4, 4, p, 3) == -1
    assert L.sc_debug_schur_llt(p, -1, 4, p, 4) == -1
    assert L.sc_debug_schur_llt(None, 4, 4, p, 4) == -1
    assert L.sc_debug_schur_llt(None, 0, 0, None, 0) == 0
