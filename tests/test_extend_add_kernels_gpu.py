"""The four extend-add implementations alone (sc_debug_extend_add), bit for bit:
assemble_cols_kernel, assemble_tile_kernel (with the column limits of the distributed
assembly), small_assemble inside front_small_kernel<1|2|3>, and the gather epilogue of the CB
SYRK on its three instances.

extend_add_cases.py has the cases, the reference assemble() and the derivation of the small
fronts' bound gamma_{w+17} (|L| |L|^T + |S|).  Every child sum is a fixed sequence of fp64
additions (children in child-list order, no atomics), so cols and tile equal assemble() bit for
bit, and the gathering SYRK equals sc_debug_syrk_ex on a C holding assemble()'s CB part: both
epilogues subtract the same MFMA sums from the same bits.  The strict upper triangles of the
children's CBs hold NaN; the gather's target holds NaN (it is written, never read) and so do
the panel rows above its A operand.  Everything outside a written window -- the strict upper
triangles of the panel's diagonal block and of the CB, columns outside [0, ncol) and outside
the limits, the children, the values, lead-ins and canaries -- is compared bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import extend_add_cases as K
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

COLS, TILE, SMALL, GATHER = 0, 1, 2, 3


def _dev(host):
    return torch.tensor(host, device="cuda", dtype=torch.float64)


def _ptr(t, first=1):
    return ctypes.c_void_p(t.data_ptr() + 8 * first)


def _run(case, op, bufs, p0, p1=0, p2=0):
    """One hook call on fresh device copies of bufs; (host copies after the call, status word)."""
    d = [_dev(b) for b in bufs]
    info = ctypes.c_int32(-1)
    rc = sc.lib().sc_debug_extend_add(op, case.m, case.w, *K.host_args(case), _ptr(d[0]), _ptr(d[1]), _ptr(d[2]),
                                      _ptr(d[3]), p0, p1, p2, ctypes.byref(info))
    assert rc == 0, (rc, sc.lib().sc_last_error())
    return [t.cpu().numpy() for t in d], info.value


@functools.lru_cache(maxsize=None)
def _front(case):
    F = K.assemble(case)
    assert np.isfinite(F).all()
    F.setflags(write=False)
    return F


def _check_assembly(what, case, bufs, outs, ncol, lo=None, hi=None):
    """Inside the window: assemble() bit for bit.  Outside: the inputs bit for bit."""
    m, w, mb = case.m, case.w, case.mb
    F = _front(case)
    pm, cm = K.window(case, ncol, lo, hi)
    P, C = K.pview(outs[2], m, w), K.cview(outs[3], mb)
    okp, okc = K.same_bits(P[pm], F[:, :w][pm]), K.same_bits(C[cm], F[w:, w:][cm])
    finite = bool(np.isfinite(P[pm]).all() and np.isfinite(C[cm]).all())
    clean = (K.same_bits(outs[0], bufs[0]) and K.same_bits(outs[1], bufs[1]) and
             K.untouched(outs[2], bufs[2], lambda b: K.pview(b, m, w), pm) and
             K.untouched(outs[3], bufs[3], lambda b: K.cview(b, mb), cm))
    lim = "" if lo is None else f" lim [{lo}, {hi})"
    print(f"KERNEL {what} {case.name} ncol={ncol}{lim}: entries {int(pm.sum() + cm.sum())}, panel bitwise {okp}, "
          f"CB bitwise {okc}, finite {finite}, rest untouched {clean}")
    assert okp and okc and finite, (what, case, ncol, lo, hi)
    assert clean, (what, case, ncol, lo, hi)


ASM_CASES = K.cols_cases() + K.tile_cases()


@pytest.mark.parametrize("case", ASM_CASES, ids=repr)
def test_cols_and_tile_equal_the_reference_bit_for_bit(gpu, case):
    bufs = K.buffers(case)
    for ncol in sorted({case.w, case.m}):
        both = []
        for op, what in ((COLS, "assemble_cols"), (TILE, "assemble_tile")):
            outs, _ = _run(case, op, bufs, ncol, *((0, 0) if op == COLS else (-1, -1)))
            _check_assembly(what, case, bufs, outs, ncol)
            both.append(outs)
        assert all(K.same_bits(a, b) for a, b in zip(*both))


@pytest.mark.parametrize("case", K.tile_cases(), ids=repr)
def test_tile_column_limits(gpu, case):
    bufs = K.buffers(case)
    for ncol in sorted({case.w, case.m}):
        for lo, hi in K.tile_limits(case):
            outs, _ = _run(case, TILE, bufs, ncol, lo, hi)
            _check_assembly("assemble_tile", case, bufs, outs, ncol, lo, hi)


@pytest.mark.parametrize("case", K.small_cases(), ids=repr)
def test_small_front_factors_the_assembled_front(gpu, case):
    K.require_long_double()
    m, w, mb = case.m, case.w, case.mb
    F = _front(case)
    bufs = K.buffers(case)
    pm, cm = K.window(case)
    for maxm in sorted({K.bucket_of(m), 128}):
        outs, info = _run(case, SMALL, bufs, maxm)
        P, C = K.pview(outs[2], m, w), K.cview(outs[3], mb)
        finite = bool(np.isfinite(P[pm]).all() and np.isfinite(C[cm]).all())
        ratio, _ = K.small_ratio(F, np.where(pm, P, 0.0), np.where(cm, C, 0.0), w)
        clean = (K.same_bits(outs[0], bufs[0]) and K.same_bits(outs[1], bufs[1]) and
                 K.untouched(outs[2], bufs[2], lambda b: K.pview(b, m, w), pm) and
                 K.untouched(outs[3], bufs[3], lambda b: K.cview(b, mb), cm))
        print(f"KERNEL front_small {case.name} bucket {maxm}: status {info}, worst error / bound {ratio:.3f}, "
              f"finite {finite}, rest untouched {clean}")
        assert info == 0 and finite
        assert ratio <= 1.0, (case, maxm, ratio)
        assert clean, (case, maxm)


@pytest.mark.parametrize("bucket", K.BUCKETS)
def test_small_front_reports_the_failing_pivot(gpu, bucket):
    case = K.small_fail_cases()[bucket]
    bufs = K.buffers(case)
    _, info = _run(case, SMALL, bufs, bucket)
    good = next(c for c in K.small_cases() if (c.m, c.w) == (case.m, case.w))
    _, info2 = _run(good, SMALL, K.buffers(good), bucket)
    print(f"KERNEL front_small {case.name} bucket {bucket}: status {info}, good rerun {info2}")
    assert info == case.fail + 1 and info2 == 0


GATHER_IDS = [f"mb{mb}" for mb in K.GATHER_MB]


@pytest.mark.parametrize("bt,lean", K.GATHER_INSTANCES, ids=["bt64", "bt64lean", "bt128"])
@pytest.mark.parametrize("mb", K.GATHER_MB, ids=GATHER_IDS)
def test_gather_equals_the_syrk_on_the_assembled_block(gpu, mb, bt, lean):
    for case in K.gather_cases():
        if case.mb != mb or (lean and case.w == K.GATHER_W_DEEP):
            continue
        m, w = case.m, case.w
        F = _front(case)
        bufs = K.buffers(case, cb_nan=True, rows_nan=True)
        _, cm = K.window(case)
        # the same buffer with assemble()'s CB part in the lower triangle: what the plain SYRK updates
        cref = bufs[3].copy()
        K.cview(cref, mb)[cm] = F[w:, w:][cm]
        for epi in (0, 1):
            outs, _ = _run(case, GATHER, bufs, bt, lean, epi)
            dC, dA = _dev(cref), _dev(bufs[2])
            rc = sc.lib().sc_debug_syrk_ex(_ptr(dC), mb, _ptr(dA, 1 + w), m, mb, mb, w, bt, lean, 1, epi)
            assert rc == 0, rc
            want = dC.cpu().numpy()
            C = K.cview(outs[3], mb)
            same, finite = K.same_bits(outs[3], want), bool(np.isfinite(C[cm]).all())
            clean = all(K.same_bits(outs[i], bufs[i]) for i in (0, 1, 2))
            print(f"KERNEL syrk_gather bt={bt} lean={lean} epi={epi} {case.name} children {case.nchild}: "
                  f"bitwise {same}, finite {finite}, rest untouched {clean}")
            assert same and finite, (case, bt, lean, epi)
            assert clean, (case, bt, lean, epi)


def test_bad_arguments_leave_every_buffer_untouched(gpu):
    case = K.cols_cases()[-1]
    bufs = K.buffers(case)
    d = [_dev(b) for b in bufs]
    L = sc.lib()
    info = ctypes.c_int32(-1)
    bad_rel = case.relind.copy()
    bad_rel[0] = case.m
    for op, rel, p0, p1 in ((COLS, bad_rel, case.m, 0), (SMALL, case.relind, 100, 0), (GATHER, case.relind, 128, 1),
                            (COLS, case.relind, case.w + 1, 0)):
        rc = L.sc_debug_extend_add(op, case.m, case.w, case.nchild, case.rel_ptr.ctypes.data, rel.ctypes.data,
                                   case.a_ptr.ctypes.data, case.a_pos.ctypes.data, case.a_src.ctypes.data, case.nval,
                                   _ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), p0, p1, 0, ctypes.byref(info))
        assert rc == -1 and L.sc_last_error().decode().startswith("sc_debug_extend_add: ")
    assert all(K.same_bits(t.cpu().numpy(), b) for t, b in zip(d, bufs))
