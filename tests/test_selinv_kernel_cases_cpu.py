"""The selected-inversion kernel cases without a GPU (selinv_kernel_cases.py has the read and
write sets and the bounds): (a) numpy double emulations of the three ops and the push pass the
checks the kernels face, so the derived bounds are attainable; (b) deliberately wrong emulations
each miss the named check on a named shape, so the shapes, the poison and the bounds would
notice such a kernel; (c) the two hooks refuse bad arguments before any device call."""
import ctypes
import functools

import numpy as np
import pytest

import selinv_kernel_cases as K
import solve_kernel_cases as S
import sparsecholesky_amd as sc

IDS = [K.shape_id(s) for s in K.SHAPES]


@functools.lru_cache(maxsize=None)
def _case(op, shape, family):
    """(ins, outs, count) of the emulated op on the emulated outputs of the ops before it."""
    prev = _case(op - 1, shape, family)[1] if op else None
    ins = K.inputs(op, *shape, family, lambda i: S.emulate(0, 1, *shape, i), prev)
    outs, count = K.emulate(op, *shape, ins)
    return ins, tuple(outs), count


def test_long_double_is_extended():
    K.require_long_double()


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_emulations_meet_the_bounds(shape):
    for family in K.FAMILIES:
        for op in K.OPS:
            ins, outs, count = _case(op, shape, family)
            res = K.check(op, *shape, ins, outs, count)
            print(f"EMULATED {K.NAMES[op]} family {family} {K.shape_id(shape)}: {K.fmt(res)}")
            assert K.asserted(res) <= 1.0, (op, family, res)


@pytest.mark.parametrize("name", sorted(K.MUTANTS))
def test_mutants_miss_their_check(name):
    op, family, shape, caught_by = K.MUTANTS[name]
    assert shape in K.SHAPES
    ins, outs, count = _case(op, shape, family)
    good = K.check(op, *shape, ins, outs, count)
    bad = K.check(op, *shape, ins, *K.emulate(op, *shape, ins, mutant=name))
    print(f"MUTANT {name} {K.NAMES[op]} {K.shape_id(shape)}: {K.fmt(bad)} (unmutated: {K.fmt(good)})")
    assert K.asserted(good) <= 1.0
    assert bad[caught_by] > 1.0, bad
    if name == "split_ge":  # its values are as good as the unsplit product's: only the count tells
        assert all(v <= 1.0 for k, v in bad.items() if k != "tasks"), bad


def test_the_split_boundary_and_the_task_counts():
    assert K.kchunks(512) == 1 and K.kchunks(513) == 3 and K.kchunks(600) == 3 and K.kchunks(1) == 1
    assert [K.tasks(*s, 2) for s in ((1, 1, 0), (128, 128, 0), (512, 128, 0), (513, 128, 0), (600, 64, 0))] == \
        [1, 3, 3, 12, 4]
    assert [K.tasks(*s, 0) for s in ((64, 64, 0), (65, 64, 0), (192, 128, 0), (193, 128, 0))] == [0, 1, 1, 2]
    # (513, 128, 0): the last chunk is the single term k = 512; (600, 64, 0): the seam k = nb
    # between the X^T X terms and the W^T Z_RK terms lies inside chunk 0
    assert 513 - 2 * K.KC == 1 and 0 < 64 < K.KC


def test_reference_terms_per_gamma_index():
    worst = 0.0
    for shape in K.SHAPES:
        d, live = K.zkk_depth(*shape)
        assert (d >= 1).all() and (d <= live).all()
        worst = max(worst, float((live / d).max()))
    print(f"reference terms / gamma index, worst over the shapes: {worst:.2f}")
    assert worst < 4.0  # the 1 + 2^-9 of worst()


def test_a_stray_write_is_noticed():
    shape = (300, 200, 0)
    for op in K.OPS:
        ins, outs, _ = _case(op, shape, "W")
        assert K.untouched(*shape, op, ins, outs)
        for bi, at in ((0, 0), (0, 5), (0, -1), (1, 0), (1, -K.CANARY - 1), (1, -K.CANARY), (2, 0), (2, 3), (2, -1),
                       (3, 0), (3, -1)) + (((3, 1),) if op else ()):
            bad = [b.copy() for b in outs]
            bad[bi][at] = 0.5
            assert not K.untouched(*shape, op, ins, bad), (op, bi, at)


def test_poison_fails_when_read():
    # Z_KK with one entry of the old Z_KK added: NaN, a miss
    shape = (300, 200, 0)
    ins, outs, count = _case(2, shape, "W")
    bad = [b.copy() for b in outs]
    K.fview(bad[1], *shape[:2])[5, 3] += K.fview(ins[1], *shape[:2])[5, 3]
    assert K.check(2, *shape, ins, bad, count)["Z_KK"] == float("inf")


@pytest.mark.parametrize("mbc", K.PUSH_SIZES)
def test_push_emulation_and_its_mutant(mbc):
    m, w = K.PUSH_PARENT
    rel = K.push_case(mbc)[0]
    assert len(rel) == mbc and (np.diff(rel) > 0).all() and rel.min() >= 0 and rel.max() < m
    assert mbc == 1 or ((rel < w).any() and (rel >= w).any())
    ref = K.push_reference(mbc)
    assert np.isfinite(ref).all()
    assert K.same_bits(K.push_emulate(mbc), ref)
    if mbc > 1:  # reading an upper triangle: poison
        assert not K.same_bits(K.push_emulate(mbc, upper=True), ref)


def test_hooks_refuse_bad_arguments_before_any_device_call():
    # no device pointer is ever followed: every call returns before the first HIP call
    L = sc.lib()
    p = ctypes.c_void_p(4096)
    step, push = L.sc_debug_selinv_step, L.sc_debug_selinv_push

    def refused(rc, who):
        return rc == -1 and L.sc_last_error().decode().startswith(who + ": ")

    for m, w, k0, op in ((300, 200, 200, 0), (300, 200, 256, 1),  # k0 >= w
                         (300, 200, 64, 0), (300, 200, 1, 2), (300, 200, -128, 1),  # k0 % 128
                         (300, 200, 0, -1), (300, 200, 0, 3),  # the op
                         (0, 0, 0, 0), (200, 300, 0, 0), (300, 0, 0, 0), (1 << 20, 64, 0, 0)):  # the sizes
        assert refused(step(p, p, m, w, k0, op, p, p), "sc_debug_selinv_step"), (m, w, k0, op)
    for op in K.OPS:
        assert refused(step(None, p, 300, 200, 0, op, p, p), "sc_debug_selinv_step")
        assert refused(step(p, None, 300, 200, 0, op, p, p), "sc_debug_selinv_step")
        assert refused(step(p, p, 300, 200, 0, op, None, p), "sc_debug_selinv_step")  # mb > 0
        assert refused(step(p, p, 300, 200, 0, op, p, None), "sc_debug_selinv_step")  # nr > 0
    # no row below the block: no launch, nothing touched, Z_II and W may be null
    assert step(p, p, 128, 128, 0, 0, None, None) == 0 and step(p, p, 128, 128, 0, 1, None, None) == 0

    def ps(m, w, rel, z=p, zii=p, out=p, mbc=None):
        ri = None if rel is None else np.asarray(rel, dtype=np.int32)
        return push(m, w, z, zii, len(ri) if mbc is None else mbc, None if ri is None else ri.ctypes.data, out)

    who = "sc_debug_selinv_push"
    assert refused(ps(0, 0, [0]), who) and refused(ps(90, 200, [0]), who) and refused(ps(1 << 20, 4, [0]), who)
    assert refused(ps(200, 90, [0], mbc=-1), who) and refused(ps(200, 90, [0], mbc=201), who)
    assert refused(ps(200, 90, [3, 200]), who) and refused(ps(200, 90, [-1, 3]), who)  # out of range
    assert refused(ps(200, 90, [3, 3]), who) and refused(ps(200, 90, [5, 3, 7]), who)  # not ascending
    assert refused(ps(200, 90, None, mbc=2), who)
    assert refused(ps(200, 90, [3, 100], z=None), who) and refused(ps(200, 90, [3, 100], zii=None), who)
    assert refused(ps(200, 90, [3, 100], out=None), who)
    assert ps(200, 90, [], zii=None, out=None, z=None) == 0  # mbc == 0: nothing launched
