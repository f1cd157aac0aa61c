"""Cases and references for the four extend-add implementations alone (sc_debug_extend_add),
shared by test_extend_add_kernels_gpu.py (the kernels) and test_extend_add_cases_cpu.py (the
references, the generator's features, the hook's refusals).

A case is one parent front (m rows, w pivots, mb = m - w) with prescribed children and A
entries.  Child q has mbc_q contribution rows at the strictly ascending parent positions
rels[q]; its contribution block is mbc_q x mbc_q column-major, the lower triangle data, the
strict upper triangle NaN (the kernels must never load it).  Pivot column j has A entries at
the front rows a_pos (>= j, distinct, the diagonal among them) with the values Ax[a_src];
a_src is a piece of a random permutation of [0, nval), nval = entries + 7: never the identity.

assemble(case) is the expected front, bit for bit: per entry 0.0, overwritten by the A entry if
there is one, then += each child's entry in child order -- every sum a fixed sequence of fp64
additions, which numpy performs like the kernels (no atomics, no reassociation, no FMA: there
is no product).  All values carry full mantissas (uniform draws), so two orders of the same
sum differ in their last bits for all but a few entries and a swapped child shows.

Device buffers (buffers()): every operand starts one double into its allocation and ends in
CANARY doubles; lead-in, canaries, the panel and the CB hold finite random values that must
come back bit for bit outside the written window (window(), untouched()).

The bound of the small-front kernel.  Let F = assemble(case), L the returned panel (m x w,
lower trapezoid) and S the returned CB (lower triangle).  u = 2^-53, gamma_k = k u / (1 - k u).
front_small_kernel factors right-looking in registers, four pivots per step; per entry the
operations are those of the textbook algorithm:
  (i, j), j < w:   x = f_ij - sum_{t<j} l_it l_jt by j FMAs in ascending t (one rounding per term),
                   l_ij = fl(x r_j) with r_j = rsqrt_f64(d_j) ~ 1 / sqrt(d_j), and the diagonal
                   l_jj = fl(d_j r_j).  With r_j = (1 + e_j) / sqrt(d_j), |e_j| <= 8 u (rsqrt_f64 is
                   a v_rsq_f64 seed and two Newton steps, about 1 ulp; 8 u is the allowance of
                   the panel bound in test_kernels_gpu.py), l_ij l_jj = x (1 + e_j)^2 (1 + d)(1 + d'):
                   the last term passes 2 + 16 roundings' worth, the others at most j + 1 more than
                   that never -- Higham 8.5 / 10.3 give |f_ij - sum_{t<=j} l_it l_jt| <=
                   gamma_{j+1+16} sum |l_it| |l_jt|, and j + 1 <= w.
  (i, j), j >= w:  s_ij = f_ij - sum_{t<w} l_it l_jt by w FMAs: |f_ij - sum l_it l_jt - s_ij| <=
                   gamma_w (sum |l_it| |l_jt| + |s_ij|).
So entry by entry on the lower trapezoid |F - L L^T - [0 0; 0 S]| <= gamma_{w+17} (|L| |L|^T + |S|):
the panel bound's nb + 17 with the w pivot steps in the place of nb.  Derived from the counts,
never fitted.  The residual is evaluated in long double (products of two doubles are exact
there, a sum of w + 1 of them is within (w + 1) 2^-64, below 2^-10 of the bound) and the bound
is taken times 1 + 2^-9.
A dropped child entry: every child entry has magnitude in [0.5, 1) and the pivots' A diagonals
are (nchild + 2) m (1 + x), x in (0, 1), at most 2 * 7 * 128, so the largest entry of |L| |L|^T
+ |S| is about that and the largest bound gamma_{145} * 1800 = 2.9e-11 (m = w = 128): an entry
left out (or added twice) is a residual of at least 0.5, ten orders above the largest bound and
more above most (test_extend_add_cases_cpu.py asserts 0.5 / bound > 1e9 on every case, and that
a float64 factorization of the front with one child entry left out misses the bound by 1e6).
The bound is tight enough to see the ORDER of the children where sums cancel: with two children
swapped, fronts of w <= 5 miss it (gamma_{w+17} of a small |s_ij| against one ulp of a partial
sum of several entries of magnitude 0.5 to 1).
"""
import functools

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
CANARY = 8
BUCKETS = (32, 64, 88, 96, 128)


def gamma(k):
    return k * U / (1 - k * U)


def require_long_double():
    import zoo
    zoo.require_long_double()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def bucket_of(m):
    return next(b for b in BUCKETS if m <= b)


class Case:
    """One parent front with its children and A entries (see the module docstring)."""

    def __init__(self, kind, name, m, w, rels, seed, full_col=None, spd=False, fail=None):
        self.kind, self.name, self.m, self.w, self.mb = kind, name, m, w, m - w
        self.rels = [np.asarray(r, dtype=np.int32) for r in rels]
        self.fail = fail
        rng = np.random.default_rng(seed)
        self.rel_ptr = np.zeros(len(rels) + 1, dtype=np.int64)
        self.rel_ptr[1:] = np.cumsum([len(r) for r in self.rels])
        self.relind = np.concatenate(self.rels + [np.zeros(0, dtype=np.int32)]).astype(np.int32)
        # A entries: the diagonal, a random half of the rows below, one column (full_col) whole
        pos = []
        for j in range(w):
            below = np.arange(j + 1, m)
            pick = below if j == full_col else below[rng.random(len(below)) < 0.5]
            pos.append(rng.permutation(np.concatenate(([j], pick))))  # any order within a column
        self.a_ptr = np.zeros(w + 1, dtype=np.int64)
        self.a_ptr[1:] = np.cumsum([len(p) for p in pos])
        self.a_pos = np.concatenate(pos).astype(np.int32)
        na = len(self.a_pos)
        self.nval = na + 7
        self.a_src = rng.permutation(self.nval)[:na].astype(np.int64)
        self.ax = rng.uniform(-1, 1, self.nval)
        if spd:  # the pivot block diagonally dominant: off-diagonal row sums stay below (nchild + 1) m
            cols = np.repeat(np.arange(w), np.diff(self.a_ptr))
            diag = self.a_pos == cols
            self.ax[self.a_src[diag]] = (len(rels) + 2) * m * (1 + rng.random(w))
            if fail is not None:
                self.ax[self.a_src[diag][fail]] = -(len(rels) + 2.0) * m
        # children's CBs: lower triangle of magnitude [0.5, 1), either sign; strict upper NaN
        self.kids = []
        for r in self.rels:
            n = len(r)
            v = rng.uniform(0.5, 1, (n, n)) * rng.choice([-1.0, 1.0], (n, n))
            v[np.triu_indices(n, 1)] = np.nan
            self.kids.append(np.asfortranarray(v))
        self.seed = seed

    def __repr__(self):
        return f"{self.kind}:{self.name}"

    @property
    def nchild(self):
        return len(self.rels)


def assemble(case):
    """The assembled front (m x m, lower triangle; zeros above), in plain fp64: per entry 0.0,
    the A entry, then += each child's entry in child order."""
    F = np.zeros((case.m, case.m))
    for j in range(case.w):
        q = slice(case.a_ptr[j], case.a_ptr[j + 1])
        F[case.a_pos[q], j] = case.ax[case.a_src[q]]
    for rel, cb in zip(case.rels, case.kids):
        for jc in range(len(rel)):  # column jc of the child, rows jc .. mbc - 1; rel is injective
            F[rel[jc:], rel[jc]] += cb[jc:, jc]
    return F


def assemble_scatter(case):
    """The same front by an independent route: every contribution as a (row, column, value)
    triplet, scattered into a dense long-double matrix by np.add.at.  Returns (sum, count of
    contributions per entry)."""
    rows, cols, vals = [], [], []
    for j in range(case.w):
        q = slice(case.a_ptr[j], case.a_ptr[j + 1])
        rows.append(case.a_pos[q])
        cols.append(np.full(q.stop - q.start, j))
        vals.append(case.ax[case.a_src[q]])
    for rel, cb in zip(case.rels, case.kids):
        ic, jc = np.tril_indices(len(rel))
        rows.append(rel[ic])
        cols.append(rel[jc])
        vals.append(cb[ic, jc])
    rows, cols, vals = (np.concatenate(x) for x in (rows, cols, vals))
    F = np.zeros((case.m, case.m), dtype=LD)
    cnt = np.zeros((case.m, case.m), dtype=np.int64)
    np.add.at(F, (rows, cols), vals.astype(LD))
    np.add.at(cnt, (rows, cols), 1)
    return F, cnt


def host_args(case):
    """The hook's host arrays, in its argument order from nchild to nval."""
    return (case.nchild, case.rel_ptr.ctypes.data, case.relind.ctypes.data if len(case.relind) else None,
            case.a_ptr.ctypes.data, case.a_pos.ctypes.data, case.a_src.ctypes.data, case.nval)


def buffers(case, cb_nan=False, rows_nan=False):
    """(ax, kids, panel, cb) host images of the device buffers: lead-in double, operand, CANARY
    doubles.  Panel and CB hold finite random values (cb_nan: the CB all NaN; rows_nan: the
    panel's rows < w NaN -- what the gathering SYRK must not read)."""
    rng = np.random.default_rng([case.m, case.w, case.nchild, 77])
    m, w, mb = case.m, case.w, case.mb

    def wrap(body):
        buf = rng.uniform(-1, 1, 1 + len(body) + CANARY)
        buf[1:1 + len(body)] = body
        return buf

    kids = np.concatenate([k.ravel(order="F") for k in case.kids] + [np.zeros(0)])
    panel = rng.uniform(-1, 1, (m, w))
    if rows_nan:
        panel[:w] = np.nan
    cb = np.full(mb * mb, np.nan) if cb_nan else rng.uniform(-1, 1, mb * mb)
    return wrap(case.ax), wrap(kids), wrap(panel.ravel(order="F")), wrap(cb)


def pview(buf, m, w):
    """The m x w panel inside its buffer (a view)."""
    return buf[1:1 + m * w].reshape(w, m).T


def cview(buf, mb):
    return buf[1:1 + mb * mb].reshape(mb, mb).T


def window(case, ncol=None, lo=None, hi=None):
    """(panel mask, CB mask) of the entries an assembly of front columns [0, ncol) within the
    limits [lo, hi) writes: the lower trapezoid of those columns."""
    m, w, mb = case.m, case.w, case.mb
    ncol = m if ncol is None else ncol
    lo, hi = (0, m) if lo is None else (lo, hi)
    cols = (np.arange(m) < ncol) & (np.arange(m) >= lo) & (np.arange(m) < hi)
    low = np.tril(np.ones((m, m), dtype=bool)) & cols[None, :]
    return low[:, :w], low[w:, w:]


def untouched(out, inp, view, mask):
    """out equals inp bit for bit outside mask (a mask over view(buffer))."""
    kept = out.copy()
    view(kept)[mask] = view(inp)[mask]
    return same_bits(kept, inp)


# --------------------------------------------------------------------------
# small fronts: reference and bound
# --------------------------------------------------------------------------
def factor_reference(F, w):
    """Right-looking Cholesky of the first w columns of the lower front F in plain float64:
    (L, m x w lower trapezoid; S, the updated trailing lower triangle)."""
    A = np.tril(F).copy()
    m = A.shape[0]
    for j in range(w):
        A[j, j] = np.sqrt(A[j, j])
        A[j + 1:, j] /= A[j, j]
        c = A[j + 1:, j]
        A[j + 1:, j + 1:] -= np.tril(np.outer(c, c))
    return A[:, :w].copy(), A[w:, w:].copy()


def small_ratio(F, L, S, w):
    """Worst residual / bound of a factored front over the lower trapezoid, and the largest
    bound (module docstring)."""
    m = F.shape[0]
    Ll = np.tril(L).astype(LD)
    T = np.zeros((m, m), dtype=LD)
    T[w:, w:] = np.tril(S).astype(LD)
    res = np.abs(np.tril(F).astype(LD) - Ll @ Ll.T - T)
    bound = gamma(w + 17) * (np.abs(Ll) @ np.abs(Ll).T + np.abs(T)) * (1 + LD(2.0) ** -9)
    low = np.tril(np.ones((m, m), dtype=bool))
    return float((res[low] / bound[low]).max()), float(bound[low].max())


# --------------------------------------------------------------------------
# the generator
# --------------------------------------------------------------------------
def _subset(rng, lo, hi, n):
    """n distinct ascending positions in [lo, hi) (all of them if there are fewer)."""
    n = min(n, hi - lo)
    return np.sort(rng.choice(np.arange(lo, hi), n, replace=False))


def _clip(rows, m):
    return np.unique(np.asarray([r for r in rows if 0 <= r < m]))


def _cols_children(m, nchild, rng):
    if nchild == 0:
        return []
    if nchild == 1:
        return [_subset(rng, 0, m, max(1, m // 2))]
    return [
        _subset(rng, 0, m, 1),                                  # mbc = 1
        _subset(rng, 0, m, 70),                                 # more than 64 rows where m allows
        _subset(rng, 0, min(m, 16), 5),                         # every column in 16-column block 0
        _clip([3, 14, 15, 16, 17, 40, m - 1], m),               # straddles column 16 exactly
        _subset(rng, 0, m, max(1, m // 2)),
    ]


@functools.lru_cache(maxsize=None)
def cols_cases():
    out = []
    for m in (1, 17, 65, 130):
        for w in sorted({x for x in (1, 16, 17, m) if x <= m}):
            for nchild in (0, 1, 5):
                rng = np.random.default_rng([1, m, w, nchild])
                out.append(Case("cols", f"m{m}-w{w}-c{nchild}", m, w, _cols_children(m, nchild, rng),
                                [11, m, w, nchild], full_col=0))
    return out


TILE_SHAPES = [(255, 20, 33), (256, 48, 65), (257, 17, 33), (513, 300, 65), (600, 33, 33)]  # m, w, small children


def tile_limits(case):
    m, w = case.m, case.w
    return [(0, m), (5, 11), (16, 32), (10, 40), (w - 1, w + 1)]


@functools.lru_cache(maxsize=None)
def tile_cases():
    out = []
    for m, w, nsmall in TILE_SHAPES:
        rng = np.random.default_rng([2, m, w])
        kids = [_subset(rng, 0, m, int(rng.integers(1, 4))) for _ in range(nsmall)]  # 1 to 3 rows each
        kids.insert(7, _clip([250, 254, 255, 256, 257, 300, m - 1] if m > 256 else [3, 100, 200, 254, m - 1], m))
        kids.insert(20, _clip([256, 257, 270, 512, 513, m - 1] if m > 256 else [240, 241, 250, 251, m - 1], m))  # starts at a boundary
        kids.append(_subset(rng, 0, m, 150))  # more than 64 rows of a column inside one tile
        out.append(Case("tile", f"m{m}-w{w}-c{len(kids)}", m, w, kids, [12, m, w], full_col=1))
    return out


SMALL_M = (1, 4, 5, 63, 64, 65, 88, 89, 96, 127, 128)
SMALL_FAIL = {32: (5, 5, 3), 64: (63, 5, 0), 88: (88, 88, 70), 96: (96, 4, 3), 128: (127, 127, 64)}  # bucket: m, w, p


def _small_children(m, rng):
    kids = [_subset(rng, 0, m, m)]                       # every row: up to 128, the second 64-row half
    kids.append(_subset(rng, 0, m, max(1, m // 3)))
    kids.append(_subset(rng, 0, m, max(1, (2 * m) // 3)))
    kids.append(_subset(rng, 0, m, 1))
    kids.append(_subset(rng, m // 2, m, 70))
    return kids


@functools.lru_cache(maxsize=None)
def small_cases():
    out = []
    for m in SMALL_M:
        for w in sorted({x for x in (1, 3, 4, 5, m) if x <= m}):
            rng = np.random.default_rng([3, m, w])
            out.append(Case("small", f"m{m}-w{w}", m, w, _small_children(m, rng), [13, m, w], full_col=0, spd=True))
    return out


@functools.lru_cache(maxsize=None)
def small_fail_cases():
    out = {}
    for b, (m, w, p) in SMALL_FAIL.items():
        rng = np.random.default_rng([4, m, w])
        out[b] = Case("small", f"m{m}-w{w}-fail{p}", m, w, _small_children(m, rng), [14, m, w], full_col=0, spd=True, fail=p)
    return out


GATHER_MB = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)
GATHER_W = (1, 8, 9, 16, 17)
GATHER_W_DEEP = 130  # the non-lean instances too
GATHER_INSTANCES = [(64, 0), (64, 1), (128, 0)]  # (bt, lean)


def _gather_children(mb, w, rng):
    m = w + mb
    cbrows = lambda rows: w + _clip(rows, mb)  # noqa: E731
    kids = [
        cbrows(range(0, 50)),                                          # contiguous; > 32 columns in block 0
        cbrows(range(0, mb, 2)),                                       # every other row
        cbrows(list(range(60, 70)) + list(range(124, 132))),           # straddles rows 64 and 128
        _subset(rng, 0, w, 3),                                         # nothing in the CB part: no segment
        np.concatenate((_subset(rng, 0, w, 2), cbrows([mb // 2]))),    # one CB row, pivots before it
    ]
    for _ in range(9):                                                 # nine more segments in block (0, 0)
        kids.append(np.concatenate((_subset(rng, 0, w, 1), w + _subset(rng, 0, min(mb, 64), 3))))
    for _ in range(2):                                                 # with the three above: five in block (1, 1)
        if mb > 64:
            kids.append(w + _subset(rng, 64, min(mb, 128), 4))
    kids.append(w + _subset(rng, 0, mb, max(1, mb // 2)))
    return [np.unique(k) for k in kids if len(k)]


@functools.lru_cache(maxsize=None)
def gather_cases():
    out = []
    for mb in GATHER_MB:
        for w in GATHER_W + (GATHER_W_DEEP,):
            rng = np.random.default_rng([5, mb, w])
            out.append(Case("gather", f"mb{mb}-w{w}", w + mb, w, _gather_children(mb, w, rng), [15, mb, w]))
    return out


def block_segments(case):
    """Per 64 x 64 block (rb, cb <= rb) of the parent's CB, the children with rows and columns
    in it (what gather_segments_front lists), in child order."""
    w, mb = case.w, case.mb
    out = {}
    for rb in range((mb + 63) // 64):
        for cb in range(rb + 1):
            seg = []
            for q, rel in enumerate(case.rels):
                r = rel - w
                rows = ((r >= 64 * rb) & (r < 64 * rb + 64)).sum()
                cols = ((r >= 64 * cb) & (r < 64 * cb + 64)).sum()
                if rows and cols:
                    seg.append((q, int(rows), int(cols)))
            out[(rb, cb)] = seg
    return out
