"""Rank-k update / downdate, the host side of the C ABI (no device): the symbols, the
argument errors with their messages, and sc_updown_check -- admissibility by the row-subtree
walk and the path a sweep touches -- against the pattern of L and the supernode partition
the analysis exports."""
import ctypes

import numpy as np
import pytest

import sparsecholesky_amd as sc
from test_solve_multi import _matrix

SC_ERR_ARG = -1
NEW = ("sc_updown_check", "sc_updown_host", "sc_debug_updown_block")

# id -> (input, analysis options)
CASES = {
    "bcsstk01": ("bcsstk01", {}),
    "1138_bus": ("1138_bus", {}),
    "1138_bus_nd": ("1138_bus", dict(ordering=1)),
    "1138_bus_amd": ("1138_bus", dict(ordering=2)),
    "lap16": ("lap16", {}),
}
_symb = {}


def _case(case):
    if case not in _symb:
        name, kw = CASES[case]
        _symb[case] = sc.Symbolic(_matrix(name), **kw)
    return _symb[case]


def _err():
    return sc.lib().sc_last_error().decode()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exported_and_bound():
    raw = ctypes.CDLL(sc.LIB_PATH)
    for s in NEW:
        assert hasattr(raw, s), s
        assert s in sc.exported_symbols(), s
    assert sc.lib().sc_version() == 121
    for meth in ("update", "downdate", "updown"):
        assert callable(getattr(sc.Numeric, meth))
    assert callable(sc.Symbolic.updown_check)


def test_argument_errors_carry_their_messages():
    L = sc.lib()
    symb = _case("bcsstk01")
    Wp = np.array([0, 1], dtype=np.int64)
    Wi = np.array([3], dtype=np.int32)
    Wx = np.array([1.0])
    # sc_updown_check
    assert L.sc_updown_check(None, 1, _p(Wp), _p(Wi), None, None) == SC_ERR_ARG
    assert _err() == "sc_updown_check: null handle"
    assert L.sc_updown_check(symb.h, -1, _p(Wp), _p(Wi), None, None) == SC_ERR_ARG
    assert _err() == "sc_updown_check: k < 0"
    assert L.sc_updown_check(symb.h, 1, None, _p(Wi), None, None) == SC_ERR_ARG
    assert _err() == "sc_updown_check: null Wp"
    assert L.sc_updown_check(symb.h, 1, _p(Wp), None, None, None) == SC_ERR_ARG
    assert _err() == "sc_updown_check: null Wi"
    # k == 0 touches nothing and needs no arrays
    path = np.full(3, -5, dtype=np.int64)
    assert L.sc_updown_check(symb.h, 0, None, None, None, _p(path)) == 0
    assert path.tolist() == [0, 0, 0]
    # a row out of range
    for bad in (-1, symb.n):
        assert L.sc_updown_check(symb.h, 1, _p(Wp), _p(np.array([bad], dtype=np.int32)), None, None) == SC_ERR_ARG
        assert _err().startswith("sc_updown_check: column 0 of W") and "out of range" in _err() and str(bad) in _err()
    # sc_updown_host: every argument error is found before the handle's state is looked at
    assert L.sc_updown_host(None, 1, 1, _p(Wp), _p(Wi), _p(Wx)) == SC_ERR_ARG
    assert _err() == "sc_updown_host: null handle"


def _unit(rows):
    k = len(rows)
    return np.arange(k + 1, dtype=np.int64), np.asarray(rows, dtype=np.int32), np.ones(k)


def _path_from_supernodes(symb, first):
    """path[] recounted from the exported partition: the union of the parent chains from the
    supernodes of the first columns; 64-column blocks and m w summed over it."""
    sn = symb.supernodes()
    _, post = symb.etree()
    ipost = np.empty(symb.n, dtype=np.int64)
    ipost[post] = np.arange(symb.n)
    on = set()
    for j0 in first:
        if j0 < 0:
            continue
        s = int(np.searchsorted(sn["start"], ipost[j0], side="right") - 1)
        while s >= 0 and s not in on:
            on.add(s)
            s = int(sn["parent"][s])
    w = sn["w"].astype(np.int64)
    m = sn["m"].astype(np.int64)
    idx = np.array(sorted(on), dtype=np.int64)
    return dict(supernodes=len(idx), blocks=int(((w[idx] + 63) // 64).sum()), panel_entries=int((m[idx] * w[idx]).sum()))


@pytest.mark.parametrize("case", list(CASES))
def test_unit_vectors_are_admissible(case):
    symb = _case(case)
    n = symb.n
    perm = symb.perm().astype(np.int64)
    iperm = np.empty(n, dtype=np.int64)
    iperm[perm] = np.arange(n)
    rng = np.random.default_rng(11)
    rows = np.concatenate([[0, n - 1], rng.integers(0, n, 30)])
    first, path = symb.updown_check(_unit(rows))
    assert np.array_equal(first, iperm[rows])
    assert path == _path_from_supernodes(symb, first)
    # one column alone: its own chain
    f1, p1 = symb.updown_check(_unit(rows[2:3]))
    assert p1 == _path_from_supernodes(symb, f1) and p1["supernodes"] >= 1
    # the dense form is the same matrix
    D = np.zeros((n, 3))
    D[rows[:3], np.arange(3)] = 2.5
    fd, pd = symb.updown_check(D)
    assert np.array_equal(fd, first[:3]) and pd == _path_from_supernodes(symb, fd)


def _columns_of_L(symb, ncols, seed):
    """Per chosen column j0 of L (order of P A P^T) with at least two entries: (j0, a random
    subset of its true pattern that holds j0, the rows of P A P^T outside its pattern)."""
    Lp, Li = symb.pattern()
    n = symb.n
    rng = np.random.default_rng(seed)
    cand = np.flatnonzero(np.diff(Lp) >= 2)
    out = []
    for j0 in rng.choice(cand, min(ncols, len(cand)), replace=False):
        col = Li[Lp[j0]:Lp[j0 + 1]].astype(np.int64)
        assert col[0] == j0
        rest = col[1:]
        take = rest[rng.random(len(rest)) < 0.6]
        outside = np.setdiff1d(np.arange(j0 + 1, n), col)
        out.append((int(j0), np.concatenate([[j0], take]), outside))
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_subsets_of_a_column_of_L(case):
    symb = _case(case)
    perm = symb.perm().astype(np.int64)  # perm[row of P A P^T] = A's own row
    L = sc.lib()
    cols = _columns_of_L(symb, 12, 5)
    assert cols
    # all of them in one W, rows shuffled inside each column, in A's numbering
    rng = np.random.default_rng(6)
    Wp = np.concatenate([[0], np.cumsum([len(r) for _, r, _ in cols])]).astype(np.int64)
    Wi = np.concatenate([perm[rng.permutation(r)] for _, r, _ in cols]).astype(np.int32)
    first, path = symb.updown_check((Wp, Wi, np.ones(len(Wi))))
    assert first.tolist() == [j0 for j0, _, _ in cols]
    assert path == _path_from_supernodes(symb, first)
    for c, (j0, rows, outside) in enumerate(cols):
        if len(outside) == 0:
            continue
        # one more row, outside the pattern of L(:, j0): rejected, column and row named
        extra = int(outside[len(outside) // 2])
        bad = np.concatenate([rows, [extra]])
        # as column 1 after an admissible unit vector, so that the column number is not 0 by chance
        wp = np.array([0, 1, 1 + len(bad)], dtype=np.int64)
        wi = np.concatenate([[perm[j0]], perm[bad]]).astype(np.int32)
        rc = L.sc_updown_check(symb.h, 2, _p(wp), _p(wi), None, None)
        assert rc == SC_ERR_ARG, (case, j0, extra)
        msg = _err()
        assert msg.startswith("sc_updown_check: column 1 of W is not admissible"), msg
        assert f"row {int(perm[extra])} " in msg, msg
        with pytest.raises(sc.LibraryError, match="column 1 of W is not admissible"):
            symb.updown_check((wp, wi, np.ones(len(wi))))
        # a duplicate row
        dup = np.concatenate([rows, rows[-1:]])
        wp = np.array([0, len(dup)], dtype=np.int64)
        wi = perm[dup].astype(np.int32)
        assert L.sc_updown_check(symb.h, 1, _p(wp), _p(wi), None, None) == SC_ERR_ARG
        assert "column 0 of W" in _err() and "appears twice" in _err() and f"row {int(wi[-1])} " in _err()


def test_empty_columns_and_explicit_pattern():
    symb = _case("lap16")
    Wp = np.array([0, 0, 1, 1], dtype=np.int64)
    Wi = np.array([7], dtype=np.int32)
    first, path = symb.updown_check((Wp, Wi, np.zeros(1)))  # an explicit zero is a pattern entry
    assert first.tolist() == [-1, 7, -1]
    assert path == _path_from_supernodes(symb, first) and path["supernodes"] >= 1
    first, path = symb.updown_check((np.zeros(3, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0)))
    assert first.tolist() == [-1, -1] and path == dict(supernodes=0, blocks=0, panel_entries=0)
