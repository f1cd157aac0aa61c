"""The product / residual kernels alone, through sc_debug_spmv, against exact arithmetic.

Bounds (derived, not measured).  Per row, k its length, s = |b| + sum |a| |x| exactly,
gamma_m = m u / (1 - m u), u = 2^-53:
  * product, fp64 residual:  |R - r| <= gamma_{k+2} s      (k fmas in one fixed order, the
    chunk partials of a long row add at most two more roundings per term)
  * compensated residual:    |R - r| <= u |r| + gamma_{2k+4}^2 s   (Ogita, Rump, Oishi, Dot2,
    with room for the TwoSum combination of the chunk partials)
  * W = |b| + |A| |x|:       |W - s| <= gamma_{k+2} s
The data is cancellation-heavy, b = fl(A x), so |r| ~ u s: a plain fp64 accumulation misses
the compensated bound by about ten orders of magnitude, which is how a compiler contraction
of the error-free transforms (a * x fused into the following subtraction) would show.

omega = max_i |r_i| / w_i counts 0 / 0 as 0 (tested with empty rows and zero data); nonzero /
0 cannot be produced with finite data, because w >= |b| and w >= |a x| term by term and any
product that underflows in w underflows in r as well, so that branch is covered by reading.
"""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

import sparsecholesky_amd as sc

import refine_cases as rc

pytestmark = pytest.mark.gpu

SPMV_CH = 256  # kernels.hpp
MUL, FP64, DD = 0, 1, 2


def _upper(n, entries):
    """Upper CSC of the given (i <= k) -> value dictionary."""
    cols = [[] for _ in range(n)]
    for (i, k), v in sorted(entries.items()):
        cols[k].append((i, v))
    p = np.zeros(n + 1, dtype=np.int64)
    ii, xx = [], []
    for k in range(n):
        for i, v in sorted(cols[k]):
            ii.append(i), xx.append(v)
        p[k + 1] = len(ii)
    return sc.csc_matrix(n, n, p, np.array(ii, dtype=np.int32), np.array(xx, dtype=np.float64))


def _random(n, density, seed, scaled=False):
    rng = np.random.default_rng(seed)
    d = 10.0 ** rng.uniform(-8, 8, n) if scaled else np.ones(n)
    e = {}
    for k in range(n):
        for i in range(k + 1):
            if i == k or rng.random() < density:
                e[(i, k)] = rng.standard_normal() * d[i] * d[k]
    return _upper(n, e)


def _arrow():
    """Order 2 SPMV_CH + 3: row 0 is full (three chunks: 2 SPMV_CH + 3 entries), row 1 has
    exactly SPMV_CH entries (one task), row 2 SPMV_CH + 1 (two chunks, the second of one entry)."""
    n = 2 * SPMV_CH + 3
    rng = np.random.default_rng(11)
    e = {(k, k): rng.standard_normal() for k in range(n)}
    for k in range(1, n):
        e[(0, k)] = rng.standard_normal()
    for k in range(2, SPMV_CH):
        e[(1, k)] = rng.standard_normal()
    for k in range(3, SPMV_CH + 1):
        e[(2, k)] = rng.standard_normal()
    return _upper(n, e)


MATRICES = {
    "n1": lambda: _random(1, 1.0, 1),
    "n5": lambda: _random(5, 0.6, 2),
    "n67": lambda: _random(67, 0.15, 3),
    "n67_scaled": lambda: _random(67, 0.15, 4, scaled=True),
    "arrow": _arrow,
}


@functools.lru_cache(maxsize=None)
def _matrix(name):
    A = MATRICES[name]()
    rp, ci, sp = rc.expected_structure(A)
    if name == "arrow":
        assert sorted(np.diff(rp)[:3].tolist()) == [SPMV_CH, SPMV_CH + 1, 2 * SPMV_CH + 3]
    return A, rp, ci, sp, rc.Exact.of(A)


@functools.lru_cache(maxsize=None)
def _data(name, nrhs):
    """X, B = fl(A X) and the exact residual, denominator and product per column."""
    A, rp, ci, sp, E = _matrix(name)
    n = A.size()
    rng = np.random.default_rng(5 + nrhs)
    X = rng.standard_normal((n, nrhs))
    if name == "n67_scaled":
        X *= 10.0 ** rng.uniform(-8, 8, (n, 1))
    B = np.zeros((n, nrhs))
    ex = []
    for c in range(nrhs):
        y = E.mul(X[:, c])
        B[:, c] = [float(v) for v in y]
        ex.append((y, E.residual(B[:, c], X[:, c]), E.denom(B[:, c], X[:, c]), E.mul(X[:, c], absolute=True)))
    return X, B, ex


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _padded(M, ld, extra_cols=0):
    """n x k host array as a NaN-padded column-major device buffer with leading dimension ld."""
    n, k = M.shape
    buf = np.full((k + extra_cols, ld), np.nan)
    buf[:k, :n] = M.T
    return _dev(buf)


def _run(name, mode, X, B, ld, want_w=True):
    A, rp, ci, sp, _ = _matrix(name)
    n, nrhs = X.shape
    dX, dB = _padded(X, ld), _padded(B, ld)
    dR, dW = _padded(np.full((n, nrhs), np.nan), ld, 1), _padded(np.full((n, nrhs), np.nan), ld, 1)
    dN = _dev(np.full(80, np.nan))
    dAx = _dev(A.x)
    vp = ctypes.c_void_p
    st = sc.lib().sc_debug_spmv(mode, n, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp), sp.ctypes.data_as(vp), len(A.x),
                                vp(dAx.data_ptr()), nrhs, vp(dX.data_ptr()), ld, vp(dB.data_ptr()), ld,
                                vp(dR.data_ptr()), ld, vp(dW.data_ptr()) if want_w else None, ld, vp(dN.data_ptr()))
    assert st == 0, (st, sc.lib().sc_last_error())
    R, W = dR.cpu().numpy(), dW.cpu().numpy()
    # neither written outside the n x nrhs window: the padding rows and the extra column stay NaN
    for out in (R, W):
        assert np.all(np.isnan(out[:, n:])) and np.all(np.isnan(out[nrhs:]))
    return R[:nrhs, :n].T.copy(), W[:nrhs, :n].T.copy(), dN.cpu().numpy().reshape(5, 16)


def _worst(err, bound):
    """max over the entries of err / bound (Fractions), 0 / 0 = 0."""
    w = 0.0
    for e, b in zip(err, bound):
        if e == 0:
            continue
        assert b > 0, (e, b)
        w = max(w, float(e / b))
    return w


@pytest.mark.parametrize("nrhs", [1, 15, 16])
@pytest.mark.parametrize("name", list(MATRICES))
def test_residual_and_product_bounds(gpu, name, nrhs):
    A, rp, ci, sp, E = _matrix(name)
    n = A.size()
    X, B, ex = _data(name, nrhs)
    ld = n + 3
    klen = np.diff(rp)
    out = {m: _run(name, m, X, B, ld) for m in (MUL, FP64, DD)}
    worst = {"mul": 0.0, "fp64": 0.0, "dd": 0.0, "w": 0.0, "fp64_vs_dd_bound": 0.0}
    for c in range(nrhs):
        y, r, s, ax = ex[c]
        g1 = [Fraction(rc.gamma(int(k) + 2)) for k in klen]
        g2 = [Fraction(rc.gamma(2 * int(k) + 4)) ** 2 for k in klen]
        Y, Rf, Rd = out[MUL][0][:, c], out[FP64][0][:, c], out[DD][0][:, c]
        assert np.all(np.isfinite(Y)) and np.all(np.isfinite(Rf)) and np.all(np.isfinite(Rd))
        worst["mul"] = max(worst["mul"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(Y, y)],
                                                [g * a for g, a in zip(g1, ax)]))
        worst["fp64"] = max(worst["fp64"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(Rf, r)],
                                                  [g * a for g, a in zip(g1, s)]))
        ddb = [Fraction(rc.U) * abs(e) + g * a for e, g, a in zip(r, g2, s)]
        worst["dd"] = max(worst["dd"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(Rd, r)], ddb))
        worst["fp64_vs_dd_bound"] = max(worst["fp64_vs_dd_bound"],
                                        _worst([abs(Fraction(float(v)) - e) for v, e in zip(Rf, r)], ddb))
        for m in (FP64, DD):
            worst["w"] = max(worst["w"], _worst([abs(Fraction(float(v)) - e) for v, e in zip(out[m][1][:, c], s)],
                                                [g * a for g, a in zip(g1, s)]))
    print(f"SPMV-KERNEL {name} nrhs={nrhs}: worst error / bound: product {worst['mul']:.3f}, fp64 residual "
          f"{worst['fp64']:.3f}, compensated {worst['dd']:.3f}, W {worst['w']:.3f} (each must be <= 1); the fp64 "
          f"residual against the compensated bound: {worst['fp64_vs_dd_bound']:.3e}")
    assert worst["mul"] <= 1 and worst["fp64"] <= 1 and worst["dd"] <= 1 and worst["w"] <= 1
    # the norms: maxima of what the kernel itself wrote, bit for bit; the row sums of |A| to rounding
    for m in (FP64, DD):
        R, W, N = out[m]
        with np.errstate(invalid="ignore", divide="ignore"):
            om = np.where(W == 0, np.where(R == 0, 0.0, np.inf), np.abs(R) / W)
        assert np.array_equal(rc.bits(N[0, :nrhs]), rc.bits(np.abs(R).max(axis=0)))
        assert np.array_equal(rc.bits(N[1, :nrhs]), rc.bits(np.abs(X).max(axis=0)))
        assert np.array_equal(rc.bits(N[2, :nrhs]), rc.bits(np.abs(B).max(axis=0)))
        assert np.array_equal(rc.bits(N[3, :nrhs]), rc.bits(om.max(axis=0)))
        anorm = float(E.norm_inf())
        assert np.all(np.abs(N[4, :nrhs] - anorm) <= rc.gamma(int(klen.max())) * anorm)
        assert np.all(N[:, nrhs:] == 0.0)
    # without W and from other leading dimensions: the same bits
    again = _run(name, DD, X, B, n, want_w=False)
    assert np.array_equal(rc.bits(again[0]), rc.bits(out[DD][0])) and np.all(np.isnan(again[1]))
    assert np.array_equal(rc.bits(again[2]), rc.bits(out[DD][2]))


def test_plain_accumulation_cannot_meet_the_compensated_bound(gpu):
    """The margin that makes the test above sensitive to a broken transform."""
    X, B, ex = _data("n67", 16)
    klen = np.diff(_matrix("n67")[1])
    Rf = _run("n67", FP64, X, B, 70)[0]
    ratio = 0.0
    for c in range(16):
        _, r, s, _ = ex[c]
        ddb = [Fraction(rc.U) * abs(e) + Fraction(rc.gamma(2 * int(k) + 4)) ** 2 * a for e, k, a in zip(r, klen, s)]
        ratio = max(ratio, _worst([abs(Fraction(float(v)) - e) for v, e in zip(Rf[:, c], r)], ddb))
    print(f"SPMV-KERNEL n67: fp64 residual error / compensated bound = {ratio:.3e} (must exceed 1e6)")
    assert ratio > 1e6


def test_omega_zero_over_zero(gpu):
    """Rows without entries and zero data: 0 / 0 counts as 0, in omega and in the norms."""
    n = 5
    A = _upper(n, {(0, 0): 2.0, (0, 3): 1.0, (3, 3): 3.0})  # rows 1, 2, 4 are empty
    rp, ci, sp = rc.expected_structure(A)
    X = np.array([[1.0, 0.0], [5.0, 0.0], [0.0, 0.0], [2.0, 0.0], [0.0, 0.0]])
    B = np.array([[4.0, 0.0], [0.0, 0.0], [0.0, 0.0], [7.0, 0.0], [0.0, 0.0]])
    MATRICES["_empty_rows"] = lambda: A
    try:
        for mode in (FP64, DD):
            R, W, N = _run("_empty_rows", mode, X, B, n + 1)
            assert np.array_equal(R[:, 0], [0.0, 0.0, 0.0, 0.0, 0.0]) and np.array_equal(W[:, 0], [8.0, 0, 0, 14.0, 0])
            assert np.array_equal(R[:, 1], np.zeros(n)) and np.array_equal(W[:, 1], np.zeros(n))
            print(f"SPMV-KERNEL empty rows mode {mode}: omega = {N[3, :2]} (expected 0 0)")
            assert np.array_equal(N[3, :2], [0.0, 0.0]) and np.array_equal(N[0, :2], [0.0, 0.0])
            B2 = B.copy()
            B2[1, 0] = 3.0  # an empty row with b != 0: r = b, w = |b|, omega = 1
            R, W, N = _run("_empty_rows", mode, X, B2, n)
            assert R[1, 0] == 3.0 and W[1, 0] == 3.0 and N[3, 0] == 1.0
    finally:
        del MATRICES["_empty_rows"]
        _matrix.cache_clear()


def test_two_launches_equal_bits(gpu):
    X, B, _ = _data("arrow", 15)
    for mode in (MUL, FP64, DD):
        a, b = _run("arrow", mode, X, B, 520), _run("arrow", mode, X, B, 520)
        assert all(np.array_equal(rc.bits(np.nan_to_num(p)), rc.bits(np.nan_to_num(q))) for p, q in zip(a, b))


def test_hook_rejects_a_bad_structure(gpu):
    """Validated on the host before anything is launched."""
    vp = ctypes.c_void_p
    rp, ci, sp = np.array([0, 1, 2], dtype=np.int64), np.array([0, 2], dtype=np.int32), np.array([0, 1], dtype=np.int64)
    d = _dev(np.zeros(8))
    args = (vp(d.data_ptr()), 1, vp(d.data_ptr()), 2, vp(d.data_ptr()), 2, vp(d.data_ptr()), 2, None, 0, None)
    assert sc.lib().sc_debug_spmv(1, 2, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp), sp.ctypes.data_as(vp), 2, *args) == -1
    assert b"out of range" in sc.lib().sc_last_error()
    ci[1] = 1
    assert sc.lib().sc_debug_spmv(1, 2, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp), sp.ctypes.data_as(vp), 1, *args) == -1
    assert sc.lib().sc_debug_spmv(7, 2, rp.ctypes.data_as(vp), ci.ctypes.data_as(vp), sp.ctypes.data_as(vp), 2, *args) == -1
