"""The solve-kernel cases without a GPU (solve_kernel_cases.py has the bounds): (a) numpy double
emulations of every op pass the checks the kernels face, so the derived bounds are attainable;
(b) deliberately wrong emulations each miss a check on a named shape, so the shapes and bounds
would notice such a kernel; (c) the two hooks refuse bad arguments before any device call."""
import ctypes
import functools

import numpy as np
import pytest

import solve_kernel_cases as K
import sparsecholesky_amd as sc

IDS = [K.shape_id(s) for s in K.SHAPES]


def _emu0(m, w, k0):
    return lambda ins: K.emulate(0, 1, m, w, k0, ins)


@functools.lru_cache(maxsize=None)
def _ins(op, width, shape, family):
    return K.inputs(op, width, *shape, family, _emu0(*shape))


def _cases():
    for family in K.FAMILIES:
        yield 0, 1, family
        for op in (1, 2):
            for width in (1, K.RHS):
                yield op, width, family
    yield 3, K.RHS, "W"
    yield 4, K.RHS, "W"


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_emulations_meet_the_bounds(shape):
    worst = {}
    for op, width, family in _cases():
        ins = _ins(op, width, shape, family)
        res = K.check(op, width, *shape, ins, K.emulate(op, width, *shape, ins))
        print(f"EMULATED op {op} width {width} family {family} {K.shape_id(shape)}: {K.fmt(res)}")
        assert K.asserted(res) <= 1.0, (op, width, family, res)
        worst[op] = max(worst.get(op, 0.0), K.asserted(res))
    print(f"EMULATED {K.shape_id(shape)}: worst error / bound per op {worst}")


@pytest.mark.parametrize("name", sorted(K.MUTANTS))
def test_mutants_miss_a_bound(name):
    op, width, family, shape = K.MUTANTS[name]
    assert shape in K.SHAPES
    ins = _ins(op, width, shape, family)
    good = K.check(op, width, *shape, ins, K.emulate(op, width, *shape, ins))
    bad = K.check(op, width, *shape, ins, K.emulate(op, width, *shape, ins, mutant=name))
    print(f"MUTANT {name} op {op} {K.shape_id(shape)}: {K.fmt(bad)} (unmutated: {K.fmt(good)})")
    assert K.asserted(good) <= 1.0
    assert K.asserted(bad) > 1.0, bad


def test_poisoned_panel_fails_when_read():
    # an emulation that reads a column before k0 returns NaN: the checks call that a miss
    shape = (300, 200, 128)
    ins = _ins(3, K.RHS, shape, "W")
    outs = K.emulate(3, K.RHS, *shape, ins)
    K.vview(outs[1], shape[0], K.RHS)[130, 3] += K.fview(ins[0], *shape[:2])[130, 5]
    assert K.asserted(K.check(3, K.RHS, *shape, ins, outs)) == float("inf")


def test_a_stray_write_is_noticed():
    shape = (129, 128, 0)
    ins = _ins(1, 1, shape, "W")
    for bi, at in ((0, 0), (0, -1), (1, 1), (2, -K.CANARY), (3, 0), (3, -1)):
        outs = K.emulate(1, 1, *shape, ins)
        outs[bi][at] = 0.5
        assert not K.untouched(*shape, 1, 1, ins, outs), (bi, at)


def test_family_k_inverse_grows_and_stays_finite():
    K.require_long_double()
    L = K.factor(128, 128, 0, "K").astype(K.LD)
    X = np.abs(K._tri_inv_ld(L))
    far, near = float(X[127, 0]), float(X[1, 0])
    print(f"family K, nb = 128: max |X| = {float(X.max()):.3e}, |X(127, 0)| = {far:.3e}, |X(1, 0)| = {near:.3e}")
    assert np.isfinite(X.astype(np.float64)).all()
    assert 1e3 < float(X.max()) < 1e5 and far > 100 * near
    Lw = K.factor(128, 128, 0, "W").astype(K.LD)
    assert float(np.abs(K._tri_inv_ld(Lw)).max()) <= 1.0 + 1e-9


@pytest.mark.parametrize("width", [1, K.RHS])
def test_gather_case_depends_on_the_order(width):
    rel_ptr, relind, _, cbuf, ubuf = K.gather_case(width)
    n = K.GATHER_W + K.GATHER_MB
    assert rel_ptr[0] == 0 and (np.diff(rel_ptr) == K.GATHER_SIZES).all()
    hit = np.zeros(n, dtype=int)
    for q in range(len(K.GATHER_SIZES)):
        t = relind[rel_ptr[q]:rel_ptr[q + 1]]
        assert len(np.unique(t)) == len(t) and t.min(initial=0) >= 0 and t.max(initial=0) < n
        hit[t] += 1
    assert (hit[:K.GATHER_W] > 1).any() and (hit[K.GATHER_W:] > 1).any()  # overlapping targets, both sides of w
    c0, u0 = K.gather_reference(width)
    c1, u1 = K.gather_reference(width, order=range(len(K.GATHER_SIZES) - 1, -1, -1))
    assert not np.array_equal(c0.view(np.int64), c1.view(np.int64))
    assert not np.array_equal(u0.view(np.int64), u1.view(np.int64))
    assert not np.array_equal(c0, cbuf) and not np.array_equal(u0, ubuf)


def test_hooks_refuse_bad_arguments_before_any_device_call():
    # no device pointer is ever followed: every call returns before the first HIP call
    L = sc.lib()
    p = ctypes.c_void_p(4096)
    step = L.sc_debug_solve_step
    assert all(step(p, 300, 200, 128, op, 16, p, p, p) == -1 for op in (-1, 5))
    for m, w, k0, op, width, u in (
            (300, 200, 200, 1, 1, p), (300, 200, 256, 1, 1, p),   # k0 >= w
            (300, 200, 64, 1, 1, p), (300, 200, 1, 0, 1, p), (300, 200, -128, 1, 1, p),  # k0 % 128
            (300, 200, 0, 1, 2, p), (300, 200, 0, 1, 0, p), (300, 200, 0, 2, 64, p),  # the width
            (300, 200, 0, 3, 1, p), (300, 200, 0, 4, 1, p),  # products with width 1
            (0, 0, 0, 1, 1, p), (200, 300, 0, 1, 1, p), (300, 0, 0, 1, 1, p), (1 << 20, 64, 0, 1, 1, p),  # the sizes
            (300, 200, 0, 1, 1, None)):  # u missing with rows for it
        assert step(p, m, w, k0, op, width, p, p, u) == -1, (m, w, k0, op, width)
    assert step(None, 64, 64, 0, 1, 1, p, p, p) == -1
    assert step(p, 64, 64, 0, 1, 1, None, p, p) == -1
    assert step(p, 64, 64, 0, 1, 1, p, None, p) == -1

    gather = L.sc_debug_solve_gather

    def g(width, w, mb, rel_ptr, relind, uc=p, c=p, u=p):
        rp = None if rel_ptr is None else np.asarray(rel_ptr, dtype=np.int64)
        ri = None if relind is None else np.asarray(relind, dtype=np.int32)
        return gather(width, w, mb, 0 if rp is None else len(rp) - 1, None if rp is None else rp.ctypes.data,
                      None if ri is None else ri.ctypes.data, uc, c, u)

    assert g(2, 4, 4, [0, 2], [1, 5]) == -1 and g(0, 4, 4, [0, 2], [1, 5]) == -1  # the width
    assert g(1, 0, 4, [0, 1], [1]) == -1 and g(1, 4, -1, [0, 1], [1]) == -1  # the sizes
    assert g(1, 4, 4, [1, 2], [1, 5]) == -1  # rel_ptr not from 0
    assert g(1, 4, 4, [0, 2, 1], [1, 5]) == -1  # not ascending
    assert g(16, 4, 4, [0, 2], [1, 8]) == -1 and g(1, 4, 4, [0, 2], [-1, 3]) == -1  # relind out of range
    assert g(1, 4, 4, [0, 2, 4], [1, 5, 6, 6]) == -1  # not injective within a child
    assert g(1, 4, 4, None, [1]) == -1 and g(1, 4, 4, [0, 1], None) == -1
    assert g(1, 4, 4, [0, 1], [1], uc=None) == -1 and g(1, 4, 4, [0, 1], [1], c=None) == -1
    assert g(1, 4, 4, [0, 1], [1], u=None) == -1
    assert gather(1, 4, 4, -1, np.zeros(1, dtype=np.int64).ctypes.data, None, p, p, p) == -1
