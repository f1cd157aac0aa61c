"""extend_add_cases.py without a GPU: the reference assemble() against an independent
long-double scatter, the generator's cases against the hook's preconditions and against the
list of shapes and features the kernels need, the small fronts' bound on a float64 restatement
of the factorization, and sc_debug_extend_add's refusals (before any device call)."""
import copy
import ctypes

import numpy as np
import pytest

import extend_add_cases as K
import sparsecholesky_amd as sc

ALL = K.cols_cases() + K.tile_cases() + K.small_cases() + list(K.small_fail_cases().values()) + K.gather_cases()


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_case_meets_the_hooks_preconditions(case):
    m, w = case.m, case.w
    assert 1 <= w <= m
    assert case.rel_ptr[0] == 0 and (np.diff(case.rel_ptr) >= 1).all() and case.rel_ptr[-1] == len(case.relind)
    for rel, cb in zip(case.rels, case.kids):
        assert rel.dtype == np.int32 and rel.min() >= 0 and rel.max() < m and (np.diff(rel) > 0).all()
        n = len(rel)
        assert cb.shape == (n, n) and cb.flags.f_contiguous
        assert np.isnan(cb[np.triu_indices(n, 1)]).all()
        low = np.abs(cb[np.tril_indices(n)])
        assert (low >= 0.5).all() and (low < 1).all()
    assert case.a_ptr[0] == 0 and (np.diff(case.a_ptr) >= 1).all() and case.a_ptr[-1] == len(case.a_pos)
    for j in range(w):
        pos = case.a_pos[case.a_ptr[j]:case.a_ptr[j + 1]]
        assert pos.min() == j and pos.max() < m and len(np.unique(pos)) == len(pos)
    assert case.a_src.min() >= 0 and case.a_src.max() < case.nval and len(np.unique(case.a_src)) == len(case.a_src)
    assert not np.array_equal(case.a_src, np.arange(len(case.a_src)))  # never the identity
    assert np.isfinite(case.ax).all()


@pytest.mark.parametrize("case", ALL, ids=repr)
def test_assemble_against_a_long_double_scatter(case):
    K.require_long_double()
    F = K.assemble(case)
    G, cnt = K.assemble_scatter(case)
    assert np.isfinite(F).all() and not np.triu(F, 1).any() and not np.triu(cnt, 1).any()
    # a sum of n terms in any order is within gamma_{n-1} of sum |terms| <= n (every |term| < 1
    # but the pivots' diagonals, which are single terms plus children)
    mag = np.abs(G) + 2 * cnt
    assert (np.abs(F.astype(K.LD) - G) <= K.gamma(np.maximum(cnt, 1)) * mag).all()
    once = cnt <= 1
    assert K.same_bits(F[once], G[once].astype(np.float64))
    assert (cnt > 1).any() or case.nchild <= 1


def test_the_order_of_the_children_shows_in_the_bits():
    # (x + a) + b and (x + b) + a differ in the last bit for a fair share of full-mantissa triples
    for case in (K.cols_cases()[-1], K.tile_cases()[0], K.gather_cases()[-1]):
        F = K.assemble(case)
        other = copy.copy(case)
        other.rels, other.kids = case.rels[::-1], case.kids[::-1]
        G = K.assemble(other)
        assert not K.same_bits(G, F) and np.abs(G - F).max() < 1e-14, case


def test_cols_shapes_and_features():
    cases = K.cols_cases()
    assert {c.m for c in cases} == {1, 17, 65, 130}
    for m in (1, 17, 65, 130):
        assert {c.w for c in cases if c.m == m} == {x for x in (1, 16, 17, m) if x <= m}
        for w in {c.w for c in cases if c.m == m}:
            assert sorted(c.nchild for c in cases if (c.m, c.w) == (m, w)) == [0, 1, 5]
    five = [c for c in cases if c.nchild == 5]
    assert all(any(len(r) == 1 for r in c.rels) for c in five)
    assert all(any(len(r) > 64 for r in c.rels) for c in five if c.m >= 65)
    assert all(any(len(r) > 1 and r.max() < 16 for r in c.rels) for c in five if c.m >= 17)
    assert all(any(15 in r and 16 in r for r in c.rels) for c in five if c.m >= 17)
    assert all(np.diff(c.a_ptr).max() > 64 for c in cases if c.m >= 65)


def test_tile_shapes_and_features():
    cases = K.tile_cases()
    assert [c.m for c in cases] == [255, 256, 257, 513, 600]
    for c, (_, _, nsmall) in zip(cases, K.TILE_SHAPES):
        small = [r for r in c.rels if len(r) <= 3]
        assert nsmall in (33, 65) and nsmall <= len(small) <= nsmall + 1 and {len(r) for r in small} == {1, 2, 3}
        assert c.nchild > 32 and any(len(r) > 64 for r in c.rels)
        assert K.tile_limits(c) == [(0, c.m), (5, 11), (16, 32), (10, 40), (c.w - 1, c.w + 1)]
        assert all(0 <= lo <= hi <= c.m for lo, hi in K.tile_limits(c))
        assert np.diff(c.a_ptr).max() > 64
    assert {n for _, _, n in K.TILE_SHAPES} == {33, 65}
    assert any(c.nchild > 64 for c in cases)  # a third staging chunk
    for c in cases:
        if c.m > 256:
            assert any(255 in r and 256 in r for r in c.rels)  # rows straddle row 256
            assert any(r[0] == 256 for r in c.rels)            # starts at a tile and block boundary
    assert any(c.w % 16 for c in cases) and any(c.w % 16 == 0 for c in cases)


def test_small_shapes_and_features():
    cases = K.small_cases()
    assert {c.m for c in cases} == set(K.SMALL_M)
    for m in K.SMALL_M:
        assert {c.w for c in cases if c.m == m} == {x for x in (1, 3, 4, 5, m) if x <= m}
    for c in cases:
        assert max(len(r) for r in c.rels) == c.m  # up to 128 rows: the second 64-row half
        if c.m >= 70:
            assert np.diff(c.a_ptr)[0] > 64
    assert {K.bucket_of(m) for m in K.SMALL_M} == set(K.BUCKETS)
    for b, c in K.small_fail_cases().items():
        assert K.bucket_of(c.m) == b and 0 <= c.fail < c.w
        F = K.assemble(c)
        assert F[c.fail, c.fail] < 0 and (np.diag(F)[:c.fail] > 0).all()


def test_gather_shapes_and_features():
    cases = K.gather_cases()
    assert {c.mb for c in cases} == set(K.GATHER_MB)
    for mb in K.GATHER_MB:
        assert {c.w for c in cases if c.mb == mb} == set(K.GATHER_W) | {K.GATHER_W_DEEP}
    for c in cases:
        w, mb = c.w, c.mb
        cbpart = [r[r >= w] - w for r in c.rels]
        assert any(len(r) == 0 for r in cbpart)                            # no segment at all
        assert any(len(r) == 1 and len(full) > 1 for r, full in zip(cbpart, c.rels))  # one CB row
        assert any(len(r) > 1 and (np.diff(r) == 1).all() for r in cbpart) or mb == 1  # contiguous
        assert any(len(r) > 1 and (np.diff(r) == 2).all() for r in cbpart) or mb < 3   # every other row
        seg = K.block_segments(c)
        assert len(seg[(0, 0)]) >= 9 and len(seg[(0, 0)]) % 4 != 0         # SB = 4 batches and a tail
        if mb >= 128:
            assert len(seg[(1, 1)]) >= 5
        if mb > 128:
            assert any(127 in r and 128 in r for r in cbpart)              # straddles row 128
        if mb > 64:
            assert any(63 in r and 64 in r for r in cbpart)                # straddles row 64
        if mb >= 33:
            assert any(cols > 32 for s in seg.values() for _, _, cols in s)  # a wave owns more than GQ columns


@pytest.mark.parametrize("case", K.small_cases(), ids=repr)
def test_small_bound_holds_for_a_float64_reference(case):
    K.require_long_double()
    F = K.assemble(case)
    L, S = K.factor_reference(F, case.w)
    assert np.isfinite(L).all() and np.isfinite(S).all()
    ratio, bmax = K.small_ratio(F, L, S, case.w)
    assert ratio <= 1.0, ratio
    # a dropped (or doubled) child entry is a residual of at least 0.5: nine orders above the bound
    assert 0.5 / bmax > 1e9, bmax
    # and it is seen: leaving out the last entry of the first child misses the bound
    G = F.copy()
    r = case.rels[0]
    G[r[-1], r[-1]] -= case.kids[0][-1, -1]
    L2, S2 = K.factor_reference(G, case.w)
    assert K.small_ratio(F, L2, S2, case.w)[0] > 1e6


def test_hook_refuses_bad_arguments_before_any_device_call():
    # no device pointer is ever followed: every call returns before the first HIP call
    L = sc.lib()
    p = ctypes.c_void_p(4096)
    case = K.cols_cases()[-1]  # m = w = 130, five children
    gcase = K.gather_cases()[0]

    def call(c, op, p0, p1=0, p2=0, **over):
        a = dict(m=c.m, w=c.w, nchild=c.nchild, rel_ptr=c.rel_ptr, relind=c.relind, a_ptr=c.a_ptr, a_pos=c.a_pos,
                 a_src=c.a_src, nval=c.nval, ax=p, kids=p, panel=p, cb=p)
        a.update(over)
        arr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        info = ctypes.c_int32(-1)
        rc = L.sc_debug_extend_add(op, a["m"], a["w"], a["nchild"], arr(a["rel_ptr"]), arr(a["relind"]), arr(a["a_ptr"]),
                                   arr(a["a_pos"]), arr(a["a_src"]), a["nval"], a["ax"], a["kids"], a["panel"], a["cb"],
                                   p0, p1, p2, ctypes.byref(info))
        return rc == -1 and L.sc_last_error().decode().startswith("sc_debug_extend_add: ")

    def edited(x, i, v):
        y = x.copy()
        y[i] = v
        return y

    m = case.m
    for op, p0, p1, p2 in ((0, m, 0, 0), (1, m, -1, -1), (2, 128, 0, 0)):
        assert call(case, op, p0, p1, p2, rel_ptr=edited(case.rel_ptr, 2, case.rel_ptr[1] - 1))  # descending rel_ptr
        assert call(case, op, p0, p1, p2, relind=edited(case.relind, 2, case.relind[1]))         # repeated
        assert call(case, op, p0, p1, p2, relind=edited(case.relind, 2, case.relind[3] + 1))     # not ascending
        assert call(case, op, p0, p1, p2, relind=edited(case.relind, 0, m))                      # out of range
        assert call(case, op, p0, p1, p2, relind=edited(case.relind, 0, -1))
        q5 = int(case.a_ptr[5])
        assert call(case, op, p0, p1, p2, a_pos=edited(case.a_pos, q5, 4))                        # above the diagonal
        assert call(case, op, p0, p1, p2, a_pos=edited(case.a_pos, q5, m))
        assert call(case, op, p0, p1, p2, a_pos=edited(case.a_pos, q5, case.a_pos[q5 + 1]))       # twice in a column
        assert call(case, op, p0, p1, p2, a_src=edited(case.a_src, 0, case.nval))                 # out of range
        assert call(case, op, p0, p1, p2, a_src=edited(case.a_src, 0, -1))
        assert call(case, op, p0, p1, p2, a_ptr=edited(case.a_ptr, 1, case.a_ptr[2] + 1))         # descending a_ptr
        assert call(case, op, p0, p1, p2, a_ptr=edited(case.a_ptr, 0, 1))
        assert call(case, op, p0, p1, p2, w=m + 1) and call(case, op, p0, p1, p2, w=0) and call(case, op, p0, p1, p2, m=0)
        assert call(case, op, p0, p1, p2, nchild=-1)
        assert call(case, op, p0, p1, p2, rel_ptr=None) and call(case, op, p0, p1, p2, panel=None)
        assert call(case, op, p0, p1, p2, ax=None) and call(case, op, p0, p1, p2, kids=None)
    assert call(case, -1, m) and call(case, 4, m)
    assert call(case, 0, m - 1) and call(case, 0, 0) and call(case, 0, m, 1, 2)                   # ncol; cols has no limits
    assert call(case, 1, m, 5, 4) and call(case, 1, m, 0, m + 1) and call(case, 1, m, -1, 3)       # limits
    for bucket in (0, 31, 100, 129, 256):
        assert call(case, 2, bucket)                                                              # a bad bucket
    small = K.small_cases()[-1]
    assert small.m == 128 and call(small, 2, 96)                                                  # m above the bucket
    assert call(gcase, 3, 128, 1, 0)                                                              # lean with bt = 128
    assert call(gcase, 3, 96, 0, 0) and call(gcase, 3, 64, 2, 0) and call(gcase, 3, 64, 0, 2)
    assert call(gcase, 3, 64, 0, 0, cb=None)
    assert call(case, 3, 64, 0, 0)                                                                # m = w: no CB to gather into
