"""SPD matrices whose assembly tree is prescribed front by front, a catalogue of them that
aims at structural code paths (long chains, fan-in, forests, the tiny-tree limits, large
fronts whose updates run on every instance of the MFMA SYRK: the big_ cases), and
long-double references.  Helper module (not collected by pytest), used by
tests/test_zoo_cpu.py and tests/test_zoo_gpu.py.

A spec is a list of fronts, children before parents: (w, parent index or -1, mb, pick).
Columns are numbered in spec order (the natural order is a postorder) and each front's
columns are contiguous.  Row sets are built top-down: a root's rows are its own columns; a
child's rows are its w columns followed by mb rows chosen from the parent's front rows by
position.  Position 0 is always chosen, so the etree parent of the child's last column is the
parent's first column; the other positions are rows of the parent's front, so every row the
child passes up is already a row of the parent.  A single child needs mb <= m(parent) - 1,
otherwise it would merge with its parent into one fundamental supernode.

The pattern of A is the upper triangle of each front's w x w block plus a dense w x mb
coupling to its rows; it is closed under elimination (the pattern of L is the pattern of A).
"""
import functools

import numpy as np

import sparsecholesky_amd as sc

PICKS = ("head", "tail", "stride", "rand")
LD = np.longdouble


# --------------------------------------------------------------------------
# generator
# --------------------------------------------------------------------------
def _positions(pick, mb, mp, rng):
    """mb distinct ascending positions in [0, mp), position 0 among them."""
    assert 1 <= mb <= mp, (mb, mp)
    if pick == "head":
        return np.arange(mb)
    if pick == "tail":
        return np.concatenate([[0], np.arange(mp - (mb - 1), mp)]).astype(np.int64)
    if pick == "stride":
        return (np.arange(mb) * mp) // mb
    if pick == "rand":
        rest = np.sort(rng.choice(np.arange(1, mp), mb - 1, replace=False)) if mb > 1 else []
        return np.concatenate([[0], rest]).astype(np.int64)
    raise ValueError(pick)


def side_by_side(*specs):
    """Several specs as one forest: parent indices shifted, the trees in the order given."""
    out = []
    for sp in specs:
        base = len(out)
        out += [(w, p + base if p >= 0 else -1, mb, pick) for (w, p, mb, pick) in sp]
    return out


class Structure:
    """The fronts of a spec: start[f] (first column), w[f], m[f], parent[f], rows[f] (the
    front's global rows, ascending, its own columns first)."""

    def __init__(self, spec, seed=0):
        nf = len(spec)
        self.spec = list(spec)
        self.w = np.array([f[0] for f in spec], dtype=np.int64)
        self.parent = np.array([f[1] for f in spec], dtype=np.int64)
        self.start = np.concatenate([[0], np.cumsum(self.w)])
        self.n = int(self.start[-1])
        self.rows = [None] * nf
        nchild = np.bincount(self.parent[self.parent >= 0], minlength=nf)
        rng = np.random.default_rng(seed)
        for f in range(nf - 1, -1, -1):
            w, p, mb, pick = spec[f]
            own = np.arange(self.start[f], self.start[f + 1])
            if p < 0:
                assert mb == 0, "a root has no rows below its columns"
                self.rows[f] = own
                continue
            assert p > f, "children come before parents"
            pr = self.rows[p]
            assert mb <= len(pr) - (1 if nchild[p] == 1 else 0), "a single child must not merge with its parent"
            self.rows[f] = np.concatenate([own, pr[_positions(pick, mb, len(pr), rng)]])
        self.m = np.array([len(r) for r in self.rows], dtype=np.int64)
        self.nchild = nchild
        self.nnz_L = int(sum(int(m) * int(w) - int(w) * (int(w) - 1) // 2 for m, w in zip(self.m, self.w)))

    def front_of_col(self):
        return np.repeat(np.arange(len(self.w)), self.w)

    def col_rows(self, j, f=None):
        """Rows of column j of L, diagonal first."""
        f = int(np.searchsorted(self.start, j, side="right") - 1) if f is None else f
        return self.rows[f][j - self.start[f]:]

    def pattern(self):
        """(Lp, Li) of L (= the lower pattern of A), rows ascending, diagonal first."""
        cols = [self.col_rows(j, f) for f in range(len(self.w)) for j in range(self.start[f], self.start[f + 1])]
        Lp = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
        return Lp, np.concatenate(cols).astype(np.int32)

    def pairs(self):
        """Extend-add pairs a tiny tree of exactly these fronts would hold."""
        mb = (self.m - self.w)[self.parent >= 0]
        return int((mb * (mb + 1) // 2).sum())

    def tiny_lds(self):
        mb = self.m - self.w
        return int((self.m * (self.m + 1) // 2 + mb * (mb + 1) // 2).sum())


def values(st, mode, seed):
    """(ti, tj, tx) upper triplets of A on the structure's pattern; mode 'dd' or 'llt'."""
    Lp, Li = st.pattern()
    n = st.n
    cols = np.repeat(np.arange(n), np.diff(Lp))
    rows = Li.astype(np.int64)
    rng = np.random.default_rng(seed)
    if mode == "dd":
        v = rng.uniform(-1, 1, len(rows))
        off = rows != cols
        deg = np.zeros(n)
        np.add.at(deg, rows[off], np.abs(v[off]))
        np.add.at(deg, cols[off], np.abs(v[off]))
        v[~off] = deg + 1.0 + rng.uniform(0, 1, n)
    elif mode == "llt":
        # a random factor on the closed pattern: diagonal in [1, 2], each column's
        # off-diagonals uniform(-1, 1) / sqrt(column length); A = L0 L0^T in double, so
        # every position of the pattern carries an update as large as the entry
        clen = np.diff(Lp)[cols]
        l0 = rng.uniform(-1, 1, len(rows)) / np.sqrt(clen)
        l0[rows == cols] = rng.uniform(1, 2, n)
        L0 = np.zeros((n, n))
        L0[rows, cols] = l0
        v = (L0 @ L0.T)[rows, cols]
    else:
        raise ValueError(mode)
    return cols, rows, v  # upper: (row, col) = (smaller, larger)


class Case:
    """One catalogue entry with one value mode: the structure, A (upper CSC) and, on demand
    and cached, the long-double references."""

    def __init__(self, name, spec, mode, seed):
        self.name, self.mode = name, mode
        self.st = Structure(spec, seed)
        ti, tj, tx = values(self.st, mode, seed + 1)
        self.A = sc.triplet_to_csc_matrix(ti, tj, tx, self.st.n)
        self.n = self.st.n

    def dense(self, x=None):
        """Full symmetric A (double)."""
        A = self.A
        cols = np.repeat(np.arange(self.n), np.diff(A.p))
        D = np.zeros((self.n, self.n))
        D[A.i, cols] = A.x if x is None else x
        D[cols, A.i] = A.x if x is None else x
        return D

    @functools.cached_property
    def ref(self):
        return Reference(self.st, self.dense())


def require_long_double():
    # a long double that is only a double cannot referee double arithmetic: fail, not skip
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not an extended type on this platform"


class Reference:
    """Long-double factor of a dense symmetric matrix on a structure's pattern (column by
    column, right-looking, only the column's nonzero rows updated) and operations with it."""

    def __init__(self, st, D):
        require_long_double()
        self.st = st
        n = st.n
        S = D.astype(LD)
        L = np.zeros((n, n), dtype=LD)
        for f in range(len(st.w)):
            for j in range(st.start[f], st.start[f + 1]):
                r = st.col_rows(j, f)
                d = np.sqrt(S[j, j])
                assert d > 0
                l = S[r, j] / d
                L[r, j] = l
                if len(r) > 1:
                    t = r[1:]
                    S[np.ix_(t, t)] -= np.outer(l[1:], l[1:])
        self.L = L
        self.Lp, self.Li = st.pattern()
        cols = np.repeat(np.arange(n), np.diff(self.Lp))
        self.Lx = L[self.Li, cols]  # long double, CSC order
        self.cols = cols
        self.logdet = 2 * np.log(np.diag(L)).sum()

    def front_errors(self, Lx):
        """Relative Frobenius error of a CSC value array against the long-double factor,
        per front of the spec (column ranges)."""
        st = self.st
        d2 = (Lx.astype(LD) - self.Lx) ** 2
        r2 = self.Lx ** 2
        edge = self.Lp[st.start]
        num = np.add.reduceat(d2, edge[:-1])
        den = np.add.reduceat(r2, edge[:-1])
        return np.sqrt(num / den).astype(np.float64)

    def solve_L(self, B):
        st, L = self.st, self.L
        X = np.array(B, dtype=LD)
        for f in range(len(st.w)):
            for j in range(st.start[f], st.start[f + 1]):
                r = st.col_rows(j, f)
                X[j] = X[j] / L[j, j]
                if len(r) > 1:
                    X[r[1:]] -= np.multiply.outer(L[r[1:], j], X[j]) if X.ndim == 2 else L[r[1:], j] * X[j]
        return X

    def solve_Lt(self, B):
        st, L = self.st, self.L
        X = np.array(B, dtype=LD)
        for f in range(len(st.w) - 1, -1, -1):
            for j in range(st.start[f + 1] - 1, st.start[f] - 1, -1):
                r = st.col_rows(j, f)
                if len(r) > 1:
                    X[j] = X[j] - L[r[1:], j] @ X[r[1:]]
                X[j] = X[j] / L[j, j]
        return X

    def solve(self, B):
        return self.solve_Lt(self.solve_L(B))

    def mul_L(self, Z):
        return self.L @ np.asarray(Z, dtype=LD)

    def mul_Lt(self, Z):
        return self.L.T @ np.asarray(Z, dtype=LD)


# --------------------------------------------------------------------------
# the catalogue
# --------------------------------------------------------------------------
def _star(leaves, root_w):
    """leaves: [(w, mb, pick)] under one root."""
    nl = len(leaves)
    return [(w, nl, mb, pick) for (w, mb, pick) in leaves] + [(root_w, -1, 0, "head")]


def _tiny_hbm_pairs():
    return _star([(8, 30, PICKS[i % 4]) for i in range(8)], 40)


def _tiny_limits(nleaves, root_w):
    return _star([(2, 20, PICKS[i % 4]) for i in range(nleaves)], root_w)


def _tiny_lds(last_w):
    # 8 x (741 + 465) + the last leaf + 2080 (root): 12281 doubles with a last leaf of
    # (2, 22), 12306 with (3, 22); the limit is 12288
    return _star([(8, 30, PICKS[i % 4]) for i in range(8)] + [(last_w, 22, "stride")], 64)


CHAIN_M = (128, 127, 97, 96, 95, 89, 88, 87, 65, 64, 63, 33, 32, 31, 8, 3, 2)


def _chain300_edges():
    # built top-down from the root; k = 0 is the chain's last front, whose rows land in the root
    chain = []
    mpar = 140
    for k in range(300):
        w = 1 + k % 4
        m = CHAIN_M[(k // 3) % len(CHAIN_M)]
        mb = max(1, min(m - w, mpar - 1))
        chain.append((w, mb, "tail" if k == 0 else PICKS[k % 4]))
        mpar = w + mb
    chain.reverse()
    return [(w, i + 1, mb, pick) for i, (w, mb, pick) in enumerate(chain)] + [(140, -1, 0, "head")]


def _chain_into_large_tail():
    return [(2, 1, 5, "head"), (2, 2, 5, "stride"), (2, 3, 5, "rand"), (2, 4, 5, "tail"), (3, 5, 40, "tail"),
            (300, -1, 0, "head")]


STAR_M = (31, 32, 33, 63, 64, 65, 87, 88, 89, 95, 96, 97, 127, 128)


def _star300_large_root():
    leaves = []
    for i in range(300):
        w = 1 + i % 5
        leaves.append((w, STAR_M[i % len(STAR_M)] - w, PICKS[i % 4]))
    return _star(leaves, 140)


def _star100_small_root():
    return _star([(1, 1 + i % 60, PICKS[i % 4]) for i in range(100)], 100)


def _fanin300_mid_cb():
    leaves = [(1 + i % 3, 300, 1 + (7 * i) % 120, PICKS[i % 4]) for i in range(300)]
    return leaves + [(70, 301, 200, "rand"), (260, -1, 0, "head")]


def _edges(shapes, root_w):
    return _star([(w, mb, PICKS[i % 4]) for i, (w, mb) in enumerate(shapes)], root_w)


def _forest():
    one = [(1, -1, 0, "head")]
    small = [(3, 2, 4, "stride"), (3, 2, 4, "tail"), (6, -1, 0, "head")]
    chain = [(3, 1, 4, "rand"), (3, 2, 4, "tail"), (3, 3, 3, "stride"), (3, 4, 3, "head"), (3, 5, 2, "tail"),
             (3, -1, 0, "head")]
    large = [(65, 1, 100, "rand"), (150, -1, 0, "head")]
    return side_by_side(one, [(2, -1, 0, "head")], small, one, chain, large, [(130, -1, 0, "head")], one)


# ---- large fronts: the 128-tile, lean and deep-K SYRK instances on irregular maps ----
# five children of every kind of row map, CBs from 10 to 300 rows
KIDS = ((130, 300, "stride"), (70, 257, "rand"), (200, 129, "tail"), (64, 64, "head"), (3, 10, "rand"))


def _under(kids, parent, root_w):
    """kids [(w, mb, pick)] under one parent (w, mb, pick) under a root."""
    nk = len(kids)
    return [(w, nk, mb, pick) for (w, mb, pick) in kids] + [parent[:1] + (nk + 1,) + parent[1:],
                                                            (root_w, -1, 0, "head")]


def _big_gather_k200():
    # fronts of 642, 677 and 713 rows: the write-once assembly's 256-row tiles, the TRSM's
    # 256-row workgroups, the selected inversion's K split
    kids = ((130, 512, "stride"), (70, 257, "rand"), (257, 420, "rand"), (64, 64, "head"))
    return _under(kids, (200, 513, "stride"), 530)


def _big_nested_gather():
    # four levels: the parent gathers the mid front's CB, which a gather wrote
    return [(90, 3, 200, "rand"), (20, 3, 260, "stride"), (5, 3, 70, "tail"), (140, 5, 280, "rand"),
            (66, 5, 257, "stride"), (70, 6, 300, "rand"), (310, -1, 0, "head")]


def _big_fanin40_tile128():
    kids = [(1 + i % 7, 60 + (37 * i) % 200, PICKS[i % 4]) for i in range(40)]
    return _under(kids, (150, 300, "rand"), 310)


def _big_cb(mb):
    # the parent's CB is mb x mb: 255 stays on 64-tiles, 256 is three 128-tiles, 257 six.  The
    # root's second child comes after the parent, so the parent is not the front before its
    # parent and the default amalgamation cannot merge it
    return [(129, 3, 200, "rand"), (8, 3, 30, "stride"), (64, 3, mb, "tail"), (40, 5, mb, "tail"),
            (25, 5, 30, "rand"), (mb + 3, -1, 0, "head")]


SPECS = {
    "tiny_hbm_pairs": _tiny_hbm_pairs,
    "tiny_16_m64": lambda: _tiny_limits(15, 64),
    "tiny_17": lambda: _tiny_limits(16, 64),
    "tiny_m65": lambda: _tiny_limits(15, 65),
    "tiny_lds_under": lambda: _tiny_lds(2),
    "tiny_lds_over": lambda: _tiny_lds(3),
    "chain300_edges": _chain300_edges,
    "chain_into_large_tail": _chain_into_large_tail,
    "star300_large_root": _star300_large_root,
    "star100_small_root": _star100_small_root,
    "fanin300_mid_cb": _fanin300_mid_cb,
    "edges_a": lambda: _edges([(63, 1), (64, 64), (65, 63), (1, 128), (1, 129)], 200),
    "edges_b": lambda: _edges([(128, 255), (129, 257), (64, 256), (127, 129)], 330),
    "forest": _forest,
    "big_gather_k40": lambda: _under(KIDS, (40, 300, "stride"), 320),
    "big_gather_k100": lambda: _under(KIDS[:4], (100, 300, "stride"), 320),
    "big_gather_k200": _big_gather_k200,
    "big_nested_gather": _big_nested_gather,
    "big_fanin40_tile128": _big_fanin40_tile128,
    "big_cb255": lambda: _big_cb(255),
    "big_cb256": lambda: _big_cb(256),
    "big_cb257": lambda: _big_cb(257),
}
NAMES = tuple(SPECS)
BIG_FRONTS = tuple(n for n in NAMES if n.startswith("big_"))
MODES = ("dd", "llt")
TINY = ("tiny_hbm_pairs", "tiny_16_m64", "tiny_17", "tiny_m65", "tiny_lds_under", "tiny_lds_over")
# cases whose structure is meant to survive the default relaxation (the chains need relax=0)
SURVIVE_RELAX = ("tiny_hbm_pairs", "star300_large_root", "star100_small_root", "fanin300_mid_cb", "big_cb255",
                 "big_cb256", "big_cb257")
# cases with large fronts (m > 128 somewhere)
LARGE = ("chain300_edges", "chain_into_large_tail", "star300_large_root", "fanin300_mid_cb", "edges_a", "edges_b",
         "forest") + BIG_FRONTS
# too many entries for a dense inverse to be the quick reference (the big_ cases have n <= 1251:
# the dense inverse stays their reference)
BIG = ("star300_large_root", "star100_small_root", "fanin300_mid_cb")


# analysis options by tag (the GPU tests factor under them, the host tests read their schedules)
OPTS = {
    "relax0": dict(relax=0),
    "default": {},
    "allfronts": dict(relax=0, small_front_max=0),       # every front through the blocked MFMA path
    "tiled_nogather": dict(relax=0, asm_tile_min_m=1, cb_gather=0),  # tiled assembly, CBs assembled, not gathered
    # 128-column slabs: slab ends, the lookahead stream and its panel instances (epi = 0)
    "nbo128": dict(relax=0, panel_nb_outer=128),
    "nbo128_rl": dict(relax=0, panel_nb_outer=128, inner_order=0, lookahead=0),  # right-looking, one stream
    # 192-column slabs: outer updates deeper than the lean instance takes (K = 192), on the lookahead stream
    "nbo192": dict(relax=0, panel_nb_outer=192),
    "tile128": dict(relax=0, syrk_tile=128),             # every SYRK on 128-tiles, every TRSM fused
    "trsm_split": dict(relax=0, trsm_split_wg=1),        # every full block: POTRF launch + prefactored TRSM
}
BIG_TAGS = ("relax0", "default", "allfronts", "tiled_nogather", "nbo128", "nbo128_rl", "tile128", "trsm_split")


def tags(name):
    if name in BIG_FRONTS:
        return list(BIG_TAGS) + (["nbo192"] if name == "big_gather_k200" else [])
    t = ["relax0", "default"]
    if name in LARGE:
        t.append("allfronts")
    if name.startswith("edges_"):
        t.append("tiled_nogather")
    return t


@functools.lru_cache(maxsize=None)
def case(name, mode="dd"):
    seed = 1000 + 17 * NAMES.index(name)
    return Case(name, SPECS[name](), mode, seed)


# --------------------------------------------------------------------------
# not positive definite inputs: diagonals set to -1
# --------------------------------------------------------------------------
def with_bad_pivots(A, cols):
    """A copy of A (upper CSC) with the diagonals of `cols` set to -1."""
    x = A.x.copy()
    for j in cols:
        k = int(A.p[j + 1]) - 1  # upper CSC: the diagonal is the column's last entry
        assert A.i[k] == j
        x[k] = -1.0
    return sc.csc_matrix(A.n_rows, A.n_cols, A.p, A.i, x, A.S)


def _first_col(name, front):
    return int(case(name).st.start[front])


# one broken pivot: case -> (matrix, column)
SINGLE_FAILURES = {
    # front 280 of the chain runs in the second chain launch (the first takes 256 fronts)
    "chain300_second_launch": lambda: (case("chain300_edges").A, _first_col("chain300_edges", 280) + 1),
    # leaf 6 of 8: its 465 extend-add pairs are pairs 2790.. of the tiny tree, past the 2048 in LDS
    "tiny_hbm_pairs_leaf6": lambda: (case("tiny_hbm_pairs").A, _first_col("tiny_hbm_pairs", 6) + 3),
    "star300_leaf299": lambda: (case("star300_large_root").A, _first_col("star300_large_root", 299)),
    "forest_last_root": lambda: (case("forest").A, case("forest").n - 1),
}
def _renumbered_first(A, c):
    """A with column c renumbered 0 and the columns before it shifted up by one.  c must be a
    leaf of the etree (a leaf front's first column), so parents keep larger numbers than
    their children.  The catalogue's own order is a postorder, which the analysis keeps as
    it is; after this renumbering it is not one any more, and the analysis reaches the
    subtree of the new column 0 after subtrees with larger numbers."""
    n = A.size()
    perm = np.concatenate([[c], np.arange(c), np.arange(c + 1, n)])  # perm[new] = old
    return sc.permute_symmetric(A, perm)


def _golden(name):
    import os

    return sc.load_matrix_market_to_csc(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                                     name + ".mtx"))


@functools.lru_cache(maxsize=None)
def _bcsstk01_renumbered():
    """bcsstk01 (n = 48: the tiny kernels; its own order is a postorder) with the first etree
    leaf c renumbered 0 for which the analysis then reaches column 1 before column 0."""
    A = _golden("bcsstk01")
    parent = sc.etree(A)
    for c in range(1, A.size()):
        if c in parent:
            continue
        B = _renumbered_first(A, c)
        post = sc.post_order(sc.etree(B))
        if list(post).index(0) > list(post).index(1):
            return B
    raise AssertionError("no leaf of bcsstk01 gives the order wanted")


# two broken pivots in independent subtrees: case -> (matrix, (a, b)), a < b
DOUBLE_FAILURES = {
    "bcsstk01_renumbered": lambda: (_bcsstk01_renumbered(), (0, 1)),
    # leaf 299's first column renumbered 0: a = 0 in leaf 299, b = 1 the column of leaf 0
    "star300_leaves_0_299": lambda: (_renumbered_first(case("star300_large_root").A,
                                                       _first_col("star300_large_root", 299)), (0, 1)),
    # the first column of the large tree's child renumbered 0: a = 0 there, b = 1 the first 1 x 1 root
    "forest_two_trees": lambda: (_renumbered_first(case("forest").A, _first_col("forest", 12)), (0, 1)),
    "1138_bus_cols_0_1": lambda: (_golden("1138_bus"), (0, 1)),
}


def single_failure(name):
    return SINGLE_FAILURES[name]()


def double_failure(name):
    return DOUBLE_FAILURES[name]()
