"""The thirteen solve and factor-product kernels alone, one 128-column step at a time
(sc_debug_solve_step, sc_debug_solve_gather), on caller data against long double.

solve_kernel_cases.py has the cases, the poison and canaries, the references and the bounds
with their derivations; the same checks pass on numpy emulations and fail on wrong ones in
test_solve_kernel_cases_cpu.py.  Here: op 0 (solve_inv_kernel, solve_inv2_kernel) on both
families; ops 1 and 2 (solve_fwd / solve_gemv / solve_diag and their _multi forms) on both
families and widths, on the inverses the device itself stored; ops 3 and 4 (mul_l_multi,
mul_lt_gemv_multi, mul_lt_diag_multi) on family W; a column of a 16-wide step keeps its bits
when the columns are permuted and its companions replaced; the two gather kernels equal numpy
double adds in child order bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import solve_kernel_cases as K
import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

IDS = [K.shape_id(s) for s in K.SHAPES]
NAMES = {0: "solve_inv", 1: "solve_fwd", 2: "solve_bwd", 3: "mul_l", 4: "mul_lt"}
PERM = np.array([(5 * j + 3) % K.RHS for j in range(K.RHS)])
FRESH = np.arange(0, K.RHS, 2)  # the columns replaced in the second run
KEPT = np.arange(1, K.RHS, 2)


def _dev(host):
    return torch.tensor(host, device="cuda", dtype=torch.float64)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() + 8)


def _run(op, width, m, w, k0, ins):
    d = [_dev(b) for b in ins]
    rc = sc.lib().sc_debug_solve_step(_ptr(d[0]), m, w, k0, op, width, _ptr(d[1]), _ptr(d[2]), _ptr(d[3]))
    assert rc == 0, rc
    return tuple(t.cpu().numpy() for t in d)


@functools.lru_cache(maxsize=None)
def _ins(op, width, shape, family):
    # ops 1 and 2 work on the inverses the device stored (computed once per shape and family)
    return K.inputs(op, width, *shape, family, lambda ins: _run(0, 1, *shape, ins))


def _check(op, width, shape, family):
    ins = _ins(op, width, shape, family)
    outs = _run(op, width, *shape, ins)
    res = K.check(op, width, *shape, ins, outs)
    print(f"KERNEL {NAMES[op]} width {width} family {family} {K.shape_id(shape)}: worst error / bound: {K.fmt(res)}")
    assert K.asserted(res) <= 1.0, res
    return ins, outs


def _check_columns_travel_alone(op, shape, ins, outs):
    """The step again with column j at PERM[j] and the even columns replaced by other data:
    the odd columns' results are the same bits at their new places."""
    m, w, _ = shape
    ins2 = (ins[0],) + K.mixed(ins[1:], *shape, op, PERM, FRESH)
    outs2 = _run(op, K.RHS, *shape, ins2)
    for bi, rows in zip((1, 2, 3), (m, K.yrows(m, w, op), m - w)):
        a, b = K.vview(outs[bi], rows, K.RHS), K.vview(outs2[bi], rows, K.RHS)
        assert np.array_equal(a[:, KEPT].view(np.int64), b[:, PERM[KEPT]].view(np.int64)), (op, bi)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_block_inverse(gpu, shape, family):
    ins, outs = _check(0, 1, shape, family)
    # the rows below the block play no part: the inverses ops 1 and 2 use (computed with them
    # in place) are the same bits
    m, w, k0 = shape
    nb, k1, _, _ = K.dims(*shape)
    up = np.triu_indices(nb, 1)
    full = K.fview(_ins(1, 1, shape, family)[0], m, w)[k0:k1, k0:k1][up]
    assert np.array_equal(K.fview(outs[0], m, w)[k0:k1, k0:k1][up].view(np.int64), full.view(np.int64))


@pytest.mark.parametrize("width", [1, K.RHS])
@pytest.mark.parametrize("op", [1, 2], ids=["forward", "backward"])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_solve_step(gpu, shape, family, op, width):
    ins, outs = _check(op, width, shape, family)
    if width == K.RHS:
        _check_columns_travel_alone(op, shape, ins, outs)


@pytest.mark.parametrize("op", [3, 4], ids=["mul_l", "mul_lt"])
@pytest.mark.parametrize("shape", K.SHAPES, ids=IDS)
def test_product_step(gpu, shape, op):
    ins, outs = _check(op, K.RHS, shape, "W")
    _check_columns_travel_alone(op, shape, ins, outs)


@pytest.mark.parametrize("width", [1, K.RHS])
def test_gather_equals_adds_in_child_order(gpu, width):
    rel_ptr, relind, ucbuf, cbuf, ubuf = K.gather_case(width)
    duc, dc, du = _dev(ucbuf), _dev(cbuf), _dev(ubuf)
    rc = sc.lib().sc_debug_solve_gather(width, K.GATHER_W, K.GATHER_MB, len(K.GATHER_SIZES), rel_ptr.ctypes.data,
                                        relind.ctypes.data, _ptr(duc), _ptr(dc), _ptr(du))
    assert rc == 0, rc
    cref, uref = K.gather_reference(width)
    same_c = np.array_equal(dc.cpu().numpy().view(np.int64), cref.view(np.int64))
    same_u = np.array_equal(du.cpu().numpy().view(np.int64), uref.view(np.int64))
    print(f"KERNEL solve_fwd_gather width {width}: c bitwise {same_c}, u bitwise {same_u}")
    assert same_c and same_u
    assert np.array_equal(duc.cpu().numpy().view(np.int64), ucbuf.view(np.int64))


def test_gather_without_children_or_rows(gpu):
    # no child, a child of nothing, no contribution rows: nothing changes
    _, _, _, cbuf, _ = K.gather_case(1)
    dc = _dev(cbuf)
    L = sc.lib()
    rp = np.zeros(2, dtype=np.int64)
    assert L.sc_debug_solve_gather(1, K.GATHER_W, 0, 0, rp.ctypes.data, None, None, _ptr(dc), None) == 0
    assert L.sc_debug_solve_gather(1, K.GATHER_W, 0, 1, rp.ctypes.data, None, None, _ptr(dc), None) == 0
    assert np.array_equal(dc.cpu().numpy().view(np.int64), cbuf.view(np.int64))
