"""The five selected-inversion kernels alone, one step of the recurrence at a time
(sc_debug_selinv_step, sc_debug_selinv_push), on caller data against long double.

selinv_kernel_cases.py has the cases, the read and write sets, the poison and canaries, the
references and the bounds with their derivations; the same checks pass on numpy emulations and
fail on wrong ones in test_selinv_kernel_cases_cpu.py.  Here: op 0 (sel_w_kernel), op 1
(sel_zrk_kernel) and op 2 (sel_zkk_kernel, sel_zkk_reduce_kernel) on both families, each on the
inverses, the W and the Z_RK the device itself left, every operand one double into its
allocation; a second run repeats the bits; a row of W depends on its own row of L_RK only; a
column of Z_RK on its own column of W only; sel_push_kernel equals numpy indexing of the
symmetric front bit for bit; bad arguments are refused with every buffer untouched."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import selinv_kernel_cases as K
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

IDS = [K.shape_id(s) for s in K.SHAPES]


def _dev(host):
    return torch.tensor(host, device="cuda", dtype=torch.float64)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() + 8)


def _inverses(shape, ins):
    d = [_dev(b) for b in ins]
    rc = sc.lib().sc_debug_solve_step(_ptr(d[0]), *shape, 0, 1, _ptr(d[1]), _ptr(d[2]), _ptr(d[3]))
    assert rc == 0, rc
    return tuple(t.cpu().numpy() for t in d)


def _run(op, shape, ins):
    d = [_dev(b) for b in ins]
    m, w, k0 = shape
    rc = sc.lib().sc_debug_selinv_step(_ptr(d[0]), _ptr(d[1]), m, w, k0, op, _ptr(d[2]), _ptr(d[3]))
    assert rc >= 0, (rc, sc.lib().sc_last_error())
    return tuple(t.cpu().numpy() for t in d), rc


@functools.lru_cache(maxsize=None)
def _case(op, shape, family):
    """(ins, outs, count) of the op on what the device left of the ops before it."""
    prev = _case(op - 1, shape, family)[1] if op else None
    ins = K.inputs(op, *shape, family, lambda i: _inverses(shape, i), prev)
    outs, count = _run(op, shape, ins)
    return ins, outs, count


@pytest.mark.parametrize("op", K.OPS, ids=[K.NAMES[op] for op in K.OPS])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_selinv_step(gpu, shape, family, op):
    ins, outs, count = _case(op, shape, family)
    res = K.check(op, *shape, ins, outs, count)
    print(f"KERNEL {K.NAMES[op]} family {family} {K.shape_id(shape)}: tasks {count}, worst error / bound: {K.fmt(res)}")
    assert K.asserted(res) <= 1.0, res
    again, count2 = _run(op, shape, ins)
    assert count2 == count and all(K.same_bits(a, b) for a, b in zip(again, outs))


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_a_row_of_w_depends_on_its_own_row_only(gpu, shape):
    """L_RK with its rows permuted gives W with its rows permuted, bit for bit, wherever a
    row's tile and wave place it."""
    m, w, k0 = shape
    nb, k1, nr, _ = K.dims(*shape)
    ins, outs, _ = _case(0, shape, "W")
    perm = np.random.default_rng([m, w, k0, 911]).permutation(nr)
    lbuf = ins[0].copy()
    K.fview(lbuf, m, w)[k1:, k0:k1] = K.fview(ins[0], m, w)[k1:, k0:k1][perm]
    outs2, _ = _run(0, shape, (lbuf,) + ins[1:])
    assert K.same_bits(K.wview(outs2[3], nr, nb), K.wview(outs[3], nr, nb)[perm])


@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_a_column_of_zrk_depends_on_its_own_column_only(gpu, shape):
    """Half of W's columns replaced: the other columns of Z_RK, and their rows of the mirror,
    keep their bits."""
    m, w, k0 = shape
    nb, k1, nr, _ = K.dims(*shape)
    ins, outs, _ = _case(1, shape, "W")
    fresh, kept = np.arange(0, nb, 2), np.arange(1, nb, 2)
    wbuf = ins[3].copy()
    K.wview(wbuf, nr, nb)[:, fresh] = np.random.default_rng([m, w, k0, 912]).uniform(-3, 3, (nr, len(fresh)))
    outs2, _ = _run(1, shape, ins[:3] + (wbuf,))
    Z, Z2 = K.fview(outs[1], m, w), K.fview(outs2[1], m, w)
    assert K.same_bits(Z2[k1:, k0:k1][:, kept], Z[k1:, k0:k1][:, kept])
    assert K.same_bits(Z2[k0:k1, k1:w][kept], Z[k0:k1, k1:w][kept])
    if nr and len(fresh):
        assert not K.same_bits(Z2[k1:, k0:k1][:, fresh], Z[k1:, k0:k1][:, fresh])


@pytest.mark.parametrize("mbc", K.PUSH_SIZES)
def test_push_equals_indexing_the_symmetric_front(gpu, mbc):
    m, w = K.PUSH_PARENT
    rel, zbuf, ibuf, obuf = K.push_case(mbc)
    dz, di, do = _dev(zbuf), _dev(ibuf), _dev(obuf)
    rc = sc.lib().sc_debug_selinv_push(m, w, _ptr(dz), _ptr(di), mbc, rel.ctypes.data, _ptr(do))
    assert rc == 0, (rc, sc.lib().sc_last_error())
    out = do.cpu().numpy()
    same = K.same_bits(out, K.push_reference(mbc))
    print(f"KERNEL sel_push mbc {mbc}: bitwise {same}, finite {bool(np.isfinite(out).all())}")
    assert same
    assert K.same_bits(dz.cpu().numpy(), zbuf) and K.same_bits(di.cpu().numpy(), ibuf)


def test_bad_arguments_leave_every_buffer_untouched(gpu):
    L = sc.lib()
    shape = (300, 200, 0)
    m, w, k0 = shape
    ins = _case(1, shape, "W")[0]
    d = [_dev(b) for b in ins]
    pl, pz, pi, pw = (_ptr(t) for t in d)
    step, push = L.sc_debug_selinv_step, L.sc_debug_selinv_push

    def refused(rc, who):
        return rc == -1 and L.sc_last_error().decode().startswith(who + ": ")

    for args in ((None, pz, m, w, 0, 1, pi, pw), (pl, None, m, w, 0, 1, pi, pw), (pl, pz, m, w, 0, 1, None, pw),
                 (pl, pz, m, w, 0, 1, pi, None),                                  # a null pointer
                 (pl, pz, m, w, 64, 1, pi, pw), (pl, pz, m, w, 1, 0, pi, pw),      # k0 % 128 != 0
                 (pl, pz, m, w, 256, 1, pi, pw), (pl, pz, m, 128, 128, 2, pi, pw),  # k0 >= w
                 (pl, pz, m, w, 0, 3, pi, pw), (pl, pz, m, w, 0, -1, pi, pw)):     # a bad op
        assert refused(step(*args), "sc_debug_selinv_step"), args[2:6]
    rel, zbuf, ibuf, obuf = K.push_case(65)
    pm, pw_ = K.PUSH_PARENT
    e = [_dev(b) for b in (zbuf, ibuf, obuf)]
    qz, qi, qo = (_ptr(t) for t in e)
    for bad in (np.r_[rel[:-1], pm], np.r_[-1, rel[1:]], rel[::-1], np.r_[rel[:5], rel[4:-1]]):
        bad = np.ascontiguousarray(bad, dtype=np.int32)
        assert len(bad) == 65
        assert refused(push(pm, pw_, qz, qi, 65, bad.ctypes.data, qo), "sc_debug_selinv_push"), bad
    assert refused(push(pm, pw_, None, qi, 65, rel.ctypes.data, qo), "sc_debug_selinv_push")
    assert refused(push(pm, pw_, qz, qi, 65, rel.ctypes.data, None), "sc_debug_selinv_push")
    assert refused(push(pm, pw_, qz, qi, 65, None, qo), "sc_debug_selinv_push")
    assert push(pm, pw_, qz, qi, 0, rel.ctypes.data, qo) == 0  # no row: nothing launched
    for t, host in zip(d + e, ins + (zbuf, ibuf, obuf)):
        assert K.same_bits(t.cpu().numpy(), host)
