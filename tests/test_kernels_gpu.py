"""The large-front kernels on their own, on caller data, against long double: every instance
of the MFMA SYRK (sc_debug_syrk_ex) and the panel kernels -- the diagonal-block POTRF, the
fused and the prefactored TRSM, the partial-block TRSM (sc_debug_panel).

The bounds are derived, not measured.  u = 2^-53, gamma_k = k u / (1 - k u).

SYRK: |got - ref| <= gamma_{K+1} (|C| + |A| |A[:N]|^T) entry by entry, the bound of a length
K inner product plus one subtraction in any summation order, with or without FMA (Higham,
Accuracy and Stability of Numerical Algorithms, 3.1 / 3.5).

Panel: with P the block's rows and L11 its top triangle as the kernels left them,
|A_blk - P L11^T| <= gamma_{nb+17} |P| |L11|^T.  nb + 1 is the constant of Cholesky and of
substitution in any order (Higham 10.3, 8.5); the other 16 allow 8 u for the reciprocal
square root the kernels multiply by (rsqrt_f64, about 1 ulp), whose error enters each
product twice.  A term dropped from an update is 1 / nb of the right-hand side in this data,
twelve orders above the bound.

Operands start one double into their allocations, the SYRK's leading dimensions are M + 3
and M + 5 and the panels' m is odd and even: the library hands these kernels 8-byte-aligned
operands with odd leading dimensions (odd m, panel_off + k0 m + r0), and the kernels' global
accesses are 64-bit buffer loads and stores and scalar double loads, which ask for no more
(mfma_kloop, syrk_rmw_epilogue, potrf_tiles_kernel, trsm_panel_g_kernel, trsm_partial).  Everything
the kernels must not write is filled with values and compared bitwise; the SYRK's operand
padding, which must not be read, holds 1e30."""
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
CANARY = 8  # doubles after each operand
POISON = 1e30


def gamma(k):
    return k * U / (1 - k * U)


def _dev(host):
    return torch.tensor(host, device="cuda", dtype=torch.float64)


def _ptr(t, first):
    return ctypes.c_void_p(t.data_ptr() + 8 * first)


# --------------------------------------------------------------------------
# SYRK
# --------------------------------------------------------------------------
SYRK_SHAPES = [(1, 1, 1), (17, 5, 3), (63, 63, 4), (64, 64, 5), (65, 64, 7), (65, 65, 8), (127, 100, 9), (128, 128, 16),
               (129, 129, 17), (130, 70, 33), (193, 129, 64), (257, 257, 65), (300, 40, 129), (260, 260, 200)]
SYRK_INSTANCES = [(64, 0), (64, 1), (128, 0)]  # (bt, lean); each with tag x epi
_worst = {}


@functools.lru_cache(maxsize=None)
def _syrk_case(M, N, K):
    """Host buffers (lead-in double, operand, canaries), the long-double reference and bound."""
    zoo.require_long_double()
    lda, ldc = M + 3, M + 5
    rng = np.random.default_rng(7919 * M + 31 * N + K)
    abuf = np.full(1 + lda * K + CANARY, POISON)
    A = rng.standard_normal((M, K))
    abuf[1:1 + lda * K].reshape(K, lda)[:, :M] = A.T
    cbuf = rng.standard_normal(1 + ldc * N + CANARY)
    C = cbuf[1:1 + ldc * N].reshape(N, ldc)[:, :M].T.copy()
    Al = A.astype(LD)
    ref = C.astype(LD) - Al @ Al[:N].T
    bound = gamma(K + 1) * (np.abs(C).astype(LD) + np.abs(Al) @ np.abs(Al[:N]).T)
    low = np.tril(np.ones((M, N), dtype=bool))
    for a in (abuf, cbuf, ref, bound, low):
        a.setflags(write=False)
    return abuf, cbuf, ref, bound, low


@pytest.mark.parametrize("bt,lean", SYRK_INSTANCES, ids=["bt64", "bt64lean", "bt128"])
@pytest.mark.parametrize("M,N,K", SYRK_SHAPES, ids=[f"{m}x{n}x{k}" for m, n, k in SYRK_SHAPES])
def test_syrk_instances(gpu, M, N, K, bt, lean):
    abuf, cbuf, ref, bound, low = _syrk_case(M, N, K)
    lda, ldc = M + 3, M + 5
    dA = _dev(abuf)
    outs = []
    for tag in (0, 1):
        for epi in (0, 1):
            dC = _dev(cbuf)
            rc = sc.lib().sc_debug_syrk_ex(_ptr(dC, 1), ldc, _ptr(dA, 1), lda, M, N, K, bt, lean, tag, epi)
            assert rc == 0, (tag, epi, rc)
            out = dC.cpu().numpy()
            assert np.array_equal(dA.cpu().numpy(), abuf)
            got = out[1:1 + ldc * N].reshape(N, ldc)[:, :M].T
            ratio = np.abs(got.astype(LD) - ref)[low] / bound[low]
            key = (bt, lean)
            _worst[key] = max(_worst.get(key, 0.0), float(ratio.max()))
            print(f"KERNEL syrk bt={bt} lean={lean} tag={tag} epi={epi} {M}x{N}x{K}: worst error / bound "
                  f"{float(ratio.max()):.3f} (worst of this instance so far {_worst[key]:.3f})")
            assert ratio.max() <= 1.0, (tag, epi, float(ratio.max()))
            # nothing else written: the strict upper part, rows M .. ldc - 1 of every column,
            # the lead-in double and the canaries, bit for bit
            kept = out.copy()
            kept[1:1 + ldc * N].reshape(N, ldc)[:, :M][low.T] = cbuf[1:1 + ldc * N].reshape(N, ldc)[:, :M][low.T]
            assert np.array_equal(kept.view(np.int64), cbuf.view(np.int64)), (tag, epi)
            outs.append(out)
    # TAG and EPI only separate the launches in profiles (kernels.hip, launch_syrk_t): a task
    # that does not gather runs the same code under all four, so the results agree bitwise
    for out in outs[1:]:
        assert np.array_equal(out.view(np.int64), outs[0].view(np.int64))


def test_old_syrk_hook_is_the_new_one(gpu):
    # sc_debug_syrk = bt 64, lean for K <= 128, tag 0, epi 0
    for (M, N, K), lean in (((130, 70, 33), 1), ((300, 40, 129), 0)):
        abuf, cbuf, _, _, _ = _syrk_case(M, N, K)
        lda, ldc = M + 3, M + 5
        dA, d0, d1 = _dev(abuf), _dev(cbuf), _dev(cbuf)
        assert sc.lib().sc_debug_syrk(_ptr(d0, 1), ldc, _ptr(dA, 1), lda, M, N, K) == 0
        assert sc.lib().sc_debug_syrk_ex(_ptr(d1, 1), ldc, _ptr(dA, 1), lda, M, N, K, 64, lean, 0, 0) == 0
        assert np.array_equal(d0.cpu().numpy().view(np.int64), d1.cpu().numpy().view(np.int64))


# --------------------------------------------------------------------------
# panel
# --------------------------------------------------------------------------
def _panel_case(m, w, k0, nb, seed, bad=None):
    """A front panel (m x w, column-major, ld = m) whose block k0 awaits its step: columns
    before k0 hold factor values, the block's rows >= k0 the product T T[:nb]^T of a random
    trapezoid T (diagonal in [1, 2], off-diagonals uniform / sqrt(m)) multiplied out in
    double, everything else -- the rows above the block, the strict upper triangle of its
    diagonal block, later columns, lead-in and canaries -- values that must come back as
    they are.  bad: the block's diagonal at that position set to -1."""
    rng = np.random.default_rng(seed)
    buf = rng.uniform(-1, 1, 1 + m * w + CANARY)
    F = buf[1:1 + m * w].reshape(w, m).T  # view: F[i, j]
    T = np.tril(rng.uniform(-1, 1, (m - k0, nb)) / np.sqrt(m))
    T[np.arange(nb), np.arange(nb)] = rng.uniform(1, 2, nb)
    Ablk = T @ T[:nb].T
    if bad is not None:
        Ablk[bad, bad] = -1.0
    low = np.tril(np.ones((m - k0, nb), dtype=bool))
    F[k0:, k0:k0 + nb][low] = Ablk[low]
    return buf, Ablk, low


def _run_panel(buf, m, w, k0, mode):
    d = _dev(buf)
    info = ctypes.c_int32(-1)
    rc = sc.lib().sc_debug_panel(_ptr(d, 1), m, w, k0, mode, ctypes.byref(info))
    assert rc == 0, (mode, rc)
    return d.cpu().numpy(), info.value


def _block(out, m, w, k0, nb):
    return out[1:1 + m * w].reshape(w, m).T[k0:, k0:k0 + nb]


def _check_panel(what, buf, out, Ablk, low, m, w, k0, nb, rows):
    """The first `rows` rows of the block hold factor rows within the bound, everything but
    the block's lower trapezoid is untouched (and below `rows` the block too)."""
    P = np.where(low, _block(out, m, w, k0, nb), 0.0).astype(LD)
    L11 = P[:nb]
    res = np.abs(Ablk.astype(LD) - P @ L11.T)
    bound = gamma(nb + 17) * (np.abs(P) @ np.abs(L11).T)
    sel = low.copy()
    sel[rows:] = False
    ratio = float((res[sel] / bound[sel]).max())
    _worst[what] = max(_worst.get(what, 0.0), ratio)
    print(f"KERNEL panel {what} m={m} w={w} k0={k0} nb={nb}: worst error / bound {ratio:.3f} "
          f"(worst of this mode so far {_worst[what]:.3f})")
    assert ratio <= 1.0, (what, ratio)
    # written: rows >= k0 of columns [k0, k0 + nb), on or below the diagonal.  The kernels
    # neither read nor write the strict upper triangle of the diagonal block (they load and
    # store i >= j only: potrf_tiles_kernel, trsm_panel_g_kernel, trsm_partial), so it comes
    # back bitwise like the rest
    kept = out.copy()
    _block(kept, m, w, k0, nb)[sel] = _block(buf, m, w, k0, nb)[sel]
    assert np.array_equal(kept.view(np.int64), buf.view(np.int64)), what


FULL = [(r, k0) for r in (64, 65, 319, 320, 321, 577) for k0 in (0, 64)]


@pytest.mark.parametrize("rows,k0", FULL, ids=[f"rows{r}-k{k}" for r, k in FULL])
def test_panel_full_blocks(gpu, rows, k0):
    nb, m = 64, k0 + rows                # m odd and even both occur
    w = k0 + nb + (7 if rows % 2 else 0)  # with and without columns after the block
    w = min(w, m)
    buf, Ablk, low = _panel_case(m, w, k0, nb, 100 * rows + k0)
    outs = {}
    for mode in (0, 1, 2):
        out, info = _run_panel(buf, m, w, k0, mode)
        assert info == 0
        _check_panel(f"mode{mode}", buf, out, Ablk, low, m, w, k0, nb, nb if mode == 0 else rows)
        outs[mode] = _block(out, m, w, k0, nb)
    # the fused TRSM and the POTRF launch + prefactored TRSM agree bitwise, the POTRF alone
    # with both on the diagonal block (tests/test_gpu_parity.py claims it for whole factors)
    assert np.array_equal(outs[1].view(np.int64), outs[2].view(np.int64))
    assert np.array_equal(outs[0][:nb].view(np.int64), outs[1][:nb].view(np.int64))


PARTIAL = [(nb, extra, k0) for nb in (1, 2, 31, 33, 63) for extra in (0, 1, 256, 257) for k0 in (0, 64)]


@pytest.mark.parametrize("nb,extra,k0", PARTIAL, ids=[f"nb{n}-rows+{e}-k{k}" for n, e, k in PARTIAL])
def test_panel_partial_blocks(gpu, nb, extra, k0):
    m, w = k0 + nb + extra, k0 + nb
    buf, Ablk, low = _panel_case(m, w, k0, nb, 7000 + 100 * nb + extra + k0)
    out0, info = _run_panel(buf, m, w, k0, 0)
    assert info == 0
    _check_panel("mode0 partial", buf, out0, Ablk, low, m, w, k0, nb, nb)
    out3, info = _run_panel(buf, m, w, k0, 3)
    assert info == 0
    _check_panel("mode3", buf, out3, Ablk, low, m, w, k0, nb, nb + extra)
    assert np.array_equal(_block(out0, m, w, k0, nb)[:nb].view(np.int64), _block(out3, m, w, k0, nb)[:nb].view(np.int64))


STATUS = [(64, mode, p) for mode in (0, 1, 2) for p in (0, 31, 63)] + \
         [(nb, mode, p) for nb in (33, 1) for mode in (0, 3) for p in sorted({0, nb - 1})]


@pytest.mark.parametrize("nb,mode,p", STATUS, ids=[f"nb{n}-mode{m}-p{p}" for n, m, p in STATUS])
def test_panel_status(gpu, nb, mode, p):
    # one not positive definite block per mode: the status word is the failing column of the
    # panel + 1 (the status path of the factorization, through an identity post table)
    k0 = 64
    m, w = k0 + nb + 70, k0 + nb
    buf, _, _ = _panel_case(m, w, k0, nb, 9000 + 10 * nb + p, bad=p)
    _, info = _run_panel(buf, m, w, k0, mode)
    assert info == k0 + p + 1
