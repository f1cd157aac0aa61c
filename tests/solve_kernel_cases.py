"""Cases, long-double references, checks and numpy emulations for the solve and factor-product
kernels alone (sc_debug_solve_step, sc_debug_solve_gather), shared by
test_solve_kernels_gpu.py (the kernels) and test_solve_kernel_cases_cpu.py (the emulations and
their mutants: the bounds are attainable, and a wrong kernel would miss them).

One step works on block B = [k0, k0 + nb), nb = min(128, w - k0), of an m x w panel F
(column-major, ld = m) whose row list is the identity; R = [k0 + nb, m) are the rows below,
nR = |R|, cut into ng = ceil(nR / 256) tasks.  op 0 stores X = inv(L11) into the block's strict
upper triangle (X(i, k), k < i, at row k, column i; two 64-blocks Xa, Xb and, for nb > 64, the
quadrant E = -Xb B21 Xa), op 1 is the forward step, op 2 the backward step, op 3 the L Z step,
op 4 the L^T Z step (sparsecholesky_debug.h).  Vectors are rows x width arrays, width 1 or 16.

Data.  Family W: diagonal in [1, 2], every other entry of the block's columns uniform in (-1, 1)
/ sqrt(m) (the rule of the panel tests).  Family K: diagonal in [1, 2], the off-diagonals inside
the diagonal block -0.15 (1 + 0.1 xi), xi uniform in (-1, 1), rows below as W: the inverse
grows away from the diagonal -- the largest |X| entry at nb = 128 (shape (128, 128, 0), long
double on the CPU) is 3.4e4 (X(127, 0); the CPU test prints it), against 1 for family W and
far from overflow in double -- so an explicit inverse is no longer substitution in other
clothes.  Every bound carries |X^|, the inverse as the device left it, so the same bounds hold
for both families.

Poison.  What a step must not read is NaN: columns outside B, rows above k0, the strict upper
triangle of the diagonal block unless it holds the inverses an op needs (op 0 owns it and must
overwrite it; ops 3 and 4 must not look at it), the rows below for op 0, and every row of c, y
and u the op does not read.  A finite result proves that none of it was used.  Operands start
one double into their allocations and end in 8 canary doubles; what a step may write is put
back from the input and the whole buffers are compared bitwise (untouched()).

Bounds.  Derived, not measured; applied entry by entry.  u = 2^-53, gamma_k = k u / (1 - k u)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.: Lemma 3.1 and (3.4) -- an
inner product of n terms summed in ANY order, with or without fused multiply-adds, has every
term within gamma_n, and gamma_d if no term passes more than d roundings; Lemma 8.4 / Theorem
8.5 for substitution; section 14.1 for residuals of computed inverses).  Exact zeros (dead
lanes, the zeros above a diagonal) add no rounding.  An fp64 MFMA is taken as at most one
rounding per product-and-add it contains (a chain of four per instruction), so an MFMA chain
over n live terms is within gamma_n like any other order.  1.0 / L(i, i) is the correctly
rounded quotient: the library is compiled without fast-math options, for which the compiler
emits the IEEE division sequence; X^'s diagonal is formed the same way here.  The counts:

  op 0, a 64-block of n columns: lane k substitutes column k of X: x_q = (delta_qk - sum_{k <=
    J < q} L(q, J) x_J) * fl(1 / L(q, q)), an fma chain of q - k <= n - 1 terms, the rounded
    reciprocal and the product with it: |La X^a - I| <= gamma_{n+1} |La| |X^a| (the right
    residual, Theorem 8.5 with one more rounding for the reciprocal).
  op 0, the quadrant: T^ = fl(B X^a) (chains of 64) and E^ = -fl(X^b T^) (chains of <= 64), so
    E^ = -X^b (B X^a + D1) + D2, |D1| <= gamma_64 |B| |X^a|, |D2| <= gamma_64 |X^b| |T^|, and
    B X^a + Lb E^ = (I - Lb X^b) B X^a - Lb X^b D1 + Lb D2.  With |I - Lb X^b| <= g |Lb| |X^b|,
    g = gamma_{nbb+1}, and |T| = (1 + gamma_64) |B| |X^a| >= |T^|:
    |B X^a + Lb E^| <= g |Lb| |X^b| |T| + gamma_64 |B| |X^a| + gamma_64 |Lb| |X^b| |T|.
  op 0, the left residual X^ L11 - I against gamma_{nb+1} |L11^-1| |L11| |X^| |L11| (Higham
    (14.7)) is reported, not asserted: the backward step applies X^^T.
  op 1, the block: row i of y^ = X^ c_B has i + 1 live terms; the single-vector kernel sums
    chains of 16, four of them in three adds and the two quadrants of a row in one more (20
    roundings at most), the panel kernel one MFMA chain: |y^ - X^ c_B|_i <= gamma_{min(i+1, D)}
    (|X^| |c_B|)_i, D = 20 (width 1) or 128 (width 16).
  op 1, a row r below: a chain over the nb live terms, then one subtraction:
    |got - (old - L(r, B) y^)| <= gamma_{nb+1} (|old| + |L(r, B)| |y^|), y^ the device's own.
  op 2: a task's partial sums at most 256 rows: products, 64 sequential adds (or a 64-term MFMA
    chain), three adds across the quarters (waves); the diagonal kernel adds the ng partials to
    c_B one after the other.  So t^ = c_B - L(R, B)^T x_R has |t^ - t| <= delta = gamma_dg (|c_B|
    + |L(R, B)|^T |x_R|), dg = min(nR, 67) + ng (0 for nR = 0).  Column k of x^ = X^^T t^ has nb
    - k live terms, two chains of 64 and an add (width 1: 65 roundings) or one MFMA chain:
    |x^ - X^^T t|_k <= sum_i |X^(i, k)| (gamma_{min(nb-k, D)} (|t_i| + delta_i) + delta_i), D =
    65 or 128.
  op 3: the block: row i of L11 z_B has i + 1 terms, then one add to the preloaded c:
    gamma_{i+2} (|c_B| + |L11| |z_B|)_i; a row below: gamma_{nb+1} (|old| + |L(r, B)| |z_B|).
  op 4: column k: L11^T z_B has nb - k terms, the partials as in op 2, then ng adds:
    |x^ - (L11^T z_B + L(R, B)^T z_R)|_k <= gamma_{max(nb-k, min(nR, 67)) + ng} (|L11|^T |z_B| +
    |L(R, B)|^T |z_R|)_k.

The references are long double (u_ld = 2^-64 = 2^-11 u) and sum at most 32 times as many terms
as the index of the gamma they are held against (2300 rows against gamma_76 at the tallest
shape), so their own rounding is at most 32 * 2^-11 = 2^-6 of a bound: worst() grants it,
every bound is taken times 1 + 2^-6.
The gather has no bound: it equals numpy double adds child by child, bit for bit.
"""
import functools

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
NB, PNB, ROWS, RHS, CANARY = 128, 64, 256, 16, 8

# (m, w, k0): the smallest shapes that reach every path of the kernels
SHAPES = [
    (1, 1, 0),          # a single column and row
    (63, 63, 0),        # partial 64-block, no rows below (r0 = -1)
    (64, 64, 0),        # full 64-block
    (65, 64, 0),        # one row below
    (100, 65, 0),       # nb = 65: the quadrant with one row
    (127, 127, 0),      # nb = 127, no rows below
    (128, 128, 0),      # full 128-block
    (129, 128, 0),      # one row below a full 128-block
    (384, 128, 0),      # exactly 256 rows below
    (385, 128, 0),      # 257 rows below: a second task with one row
    (300, 200, 0),      # rows below split between own pivots and contribution rows
    (300, 200, 128),    # k0 > 0, nb = 72
    (450, 193, 128),    # nb = 65
    (700, 320, 256),    # nb = 64 at k0 = 256
    (2300, 128, 0),     # 9 GEMV tasks: the second round of the diag kernels' partial loop
]
FAMILIES = ("W", "K")


def shape_id(s):
    return "m%d-w%d-k%d" % s


def require_long_double():
    # a long double that is only a double cannot referee double arithmetic: fail, not skip
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not an extended type on this platform"


def gamma(k):
    k = np.asarray(k, dtype=LD)
    return k * U / (1 - k * U)


def dims(m, w, k0):
    """nb, k1 = k0 + nb, nR = rows below, ng = GEMV tasks."""
    nb = min(NB, w - k0)
    k1 = k0 + nb
    return nb, k1, m - k1, (m - k1 + ROWS - 1) // ROWS


def yrows(m, w, op):
    return m if op == 4 else w


def fview(fbuf, m, w):
    return fbuf[1:1 + m * w].reshape(w, m).T


def vview(buf, rows, width):
    return buf[1:1 + rows * width].reshape(rows, width)


def _seed(m, w, k0, *more):
    return [m, w, k0, *more]


@functools.lru_cache(maxsize=None)
def factor(m, w, k0, family):
    """The block's columns from row k0 down, (m - k0) x nb: lower trapezoid, zeros above."""
    nb = dims(m, w, k0)[0]
    rng = np.random.default_rng(_seed(m, w, k0, FAMILIES.index(family)))
    L = rng.uniform(-1, 1, (m - k0, nb)) / np.sqrt(m)
    if family == "K":
        L[:nb] = -0.15 * (1 + 0.1 * rng.uniform(-1, 1, (nb, nb)))
    L[:nb][np.triu_indices(nb, 1)] = 0.0
    L[np.arange(nb), np.arange(nb)] = rng.uniform(1, 2, nb)
    L.setflags(write=False)
    return L


@functools.lru_cache(maxsize=None)
def panel(m, w, k0, family, rows_below=True):
    """The panel buffer (lead-in, m x w, canaries): the lower part of block B, everything
    else NaN; rows_below = False (op 0) poisons the rows below the block too."""
    nb, k1, _, _ = dims(m, w, k0)
    rng = np.random.default_rng(_seed(m, w, k0, 77))
    fbuf = np.full(1 + m * w + CANARY, np.nan)
    fbuf[0] = rng.standard_normal()
    fbuf[1 + m * w:] = rng.standard_normal(CANARY)
    F = fview(fbuf, m, w)
    L = factor(m, w, k0, family)
    low = np.tril_indices(nb)
    F[k0:k1, k0:k1][low] = L[:nb][low]
    if rows_below:
        F[k1:, k0:k1] = L[nb:]
    fbuf.setflags(write=False)
    return fbuf


def _reads(m, w, k0, op):
    """Row ranges of (c, y, u) the op reads (what it only writes is poisoned as well)."""
    nb, k1, _, _ = dims(m, w, k0)
    none, allu = (0, 0), (0, m - w)
    return {
        0: (none, none, none),
        1: ((k0, w), none, allu),
        2: ((k0, m), none, none),
        3: ((k0, w), (k0, k1), allu),
        4: (none, (k0, m), none),
    }[op]


def writes(m, w, k0, op):
    """Row ranges of (c, y, u) the op may write."""
    nb, k1, _, _ = dims(m, w, k0)
    none, allu = (0, 0), (0, m - w)
    return {
        0: (none, none, none),
        1: ((k1, w), (k0, k1), allu),
        2: ((k0, k1), none, none),
        3: ((k0, w), none, allu),
        4: ((k0, k1), none, none),
    }[op]


@functools.lru_cache(maxsize=None)
def vectors(m, w, k0, op, width, variant=0):
    """(cbuf, ybuf, ubuf): lead-in, rows x width, canaries; rows the op does not read NaN.
    Nonzero everywhere it reads (the products add to preloaded c and u on purpose)."""
    rng = np.random.default_rng(_seed(m, w, k0, op, width, variant))
    out = []
    for rows, (lo, hi) in zip((m, yrows(m, w, op), m - w), _reads(m, w, k0, op)):
        buf = rng.standard_normal(1 + rows * width + CANARY)
        V = vview(buf, rows, width)
        keep = V[lo:hi].copy()
        V[:] = np.nan
        V[lo:hi] = keep
        buf.setflags(write=False)
        out.append(buf)
    return tuple(out)


def mixed(bufs, m, w, k0, op, perm, fresh):
    """The 16-wide vectors with column j moved to perm[j], the columns listed in fresh replaced
    by other data first (NaN rows stay NaN)."""
    other = vectors(m, w, k0, op, RHS, variant=1)
    out = []
    for buf, alt, rows in zip(bufs, other, (m, yrows(m, w, op), m - w)):
        new = buf.copy()
        V, A, N = vview(buf, rows, RHS), vview(alt, rows, RHS), vview(new, rows, RHS)
        src = V.copy()
        src[:, fresh] = 3.0 * A[:, fresh]
        N[:, perm] = src
        out.append(new)
    return tuple(out)


# ---------------------------------------------------------------------------------------
# what the device left
# ---------------------------------------------------------------------------------------
def lower(F, m, w, k0):
    """(L11 lower triangular, L21) of block B from a panel view, as doubles."""
    nb, k1, _, _ = dims(m, w, k0)
    return np.tril(F[k0:k1, k0:k1]), F[k1:, k0:k1].copy()


def inverse(F, m, w, k0, diag_as_l=False):
    """X^ (nb x nb, lower triangular): read back from the strict upper triangle, the diagonal
    1 / L(i, i) as the kernels form it."""
    nb, k1, _, _ = dims(m, w, k0)
    blk = F[k0:k1, k0:k1]
    X = np.triu(blk, 1).T.copy()
    d = np.diag(blk)
    X[np.arange(nb), np.arange(nb)] = d if diag_as_l else 1.0 / d
    return X


def worst(err, bound):
    """max err / bound; a zero bound demands a zero error; anything non-finite is inf."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return float("inf")
    bound = bound * (1 + LD(2.0) ** -6)  # the long-double reference's own rounding
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def untouched(m, w, k0, op, width, ins, outs):
    """True when everything the step must not write came back bitwise: the lower part of F
    and its poison (op 0 owns the block's strict upper triangle, nothing else; the other ops
    own nothing of F), the rows of c, y and u outside the step, lead-ins and canaries."""
    nb, k1, _, _ = dims(m, w, k0)
    ok = True
    kept = outs[0].copy()
    if op == 0:
        up = np.triu_indices(nb, 1)
        fview(kept, m, w)[k0:k1, k0:k1][up] = fview(ins[0], m, w)[k0:k1, k0:k1][up]
    ok &= np.array_equal(_bits(kept), _bits(ins[0]))
    for bi, rows, (lo, hi) in zip((1, 2, 3), (m, yrows(m, w, op), m - w), writes(m, w, k0, op)):
        kept = outs[bi].copy()
        vview(kept, rows, width)[lo:hi] = vview(ins[bi], rows, width)[lo:hi]
        ok &= np.array_equal(_bits(kept), _bits(ins[bi]))
    return bool(ok)


def _tri_inv_ld(L):
    """inv(L) of a lower triangular matrix in long double, by substitution."""
    n = L.shape[0]
    X = np.zeros((n, n), dtype=LD)
    for q in range(n):
        e = np.zeros(n, dtype=LD)
        e[q] = 1
        X[q] = (e - L[q, :q] @ X[:q]) / L[q, q]
    return X


# ---------------------------------------------------------------------------------------
# the checks: each returns {name: worst error / bound}
# ---------------------------------------------------------------------------------------
def check(op, width, m, w, k0, ins, outs):
    require_long_double()
    nb, k1, nR, ng = dims(m, w, k0)
    Fi, Fo = fview(ins[0], m, w), fview(outs[0], m, w)
    L11, L21 = lower(Fi, m, w, k0)
    L11l, L21l = L11.astype(LD), L21.astype(LD)
    res = {"untouched": 0.0 if untouched(m, w, k0, op, width, ins, outs) else float("inf")}
    if op == 0:
        X = inverse(Fo, m, w, k0)
        Xl = X.astype(LD)
        res["left(reported)"] = worst(np.abs(Xl @ L11l - np.eye(nb)),
                                      gamma(nb + 1) * (np.abs(_tri_inv_ld(L11l)) @ np.abs(L11l) @ np.abs(Xl) @ np.abs(L11l)))
        for name, a in (("Xa", 0), ("Xb", PNB)):
            n = min(PNB, nb - a)
            if n <= 0:
                continue
            La, Xa = L11l[a:a + n, a:a + n], Xl[a:a + n, a:a + n]
            res[name] = worst(np.abs(La @ Xa - np.eye(n)), gamma(n + 1) * (np.abs(La) @ np.abs(Xa)))
        if nb > PNB:
            nbb = nb - PNB
            B, Lb = L11l[PNB:, :PNB], L11l[PNB:, PNB:]
            Xa, Xb, E = Xl[:PNB, :PNB], Xl[PNB:, PNB:], Xl[PNB:, :PNB]
            BX = np.abs(B) @ np.abs(Xa)
            LXT = np.abs(Lb) @ np.abs(Xb) @ ((1 + gamma(64)) * BX)
            res["E"] = worst(np.abs(B @ Xa + Lb @ E), gamma(nbb + 1) * LXT + gamma(64) * BX + gamma(64) * LXT)
        return res
    ci, yi, ui = vview(ins[1], m, width), vview(ins[2], yrows(m, w, op), width), vview(ins[3], m - w, width)
    co, yo, uo = vview(outs[1], m, width), vview(outs[2], yrows(m, w, op), width), vview(outs[3], m - w, width)
    old = np.vstack([ci[k1:w], ui]).astype(LD)   # the rows below: own later pivots, then u
    got = np.vstack([co[k1:w], uo]).astype(LD)
    rows_i = np.arange(nb)
    if op in (1, 2):
        Xl = inverse(Fi, m, w, k0).astype(LD)
    if op == 1:
        cB, y = ci[k0:k1].astype(LD), yo[k0:k1].astype(LD)
        a = np.minimum(rows_i + 1, 20 if width == 1 else 128)
        res["block"] = worst(np.abs(y - Xl @ cB), gamma(a)[:, None] * (np.abs(Xl) @ np.abs(cB)))
        res["rows"] = worst(np.abs(got - (old - L21l @ y)), gamma(nb + 1) * (np.abs(old) + np.abs(L21l) @ np.abs(y)))
    elif op == 2:
        cB, xR = ci[k0:k1].astype(LD), ci[k1:m].astype(LD)
        t = cB - L21l.T @ xR
        delta = gamma(min(nR, 67) + ng if nR else 0) * (np.abs(cB) + np.abs(L21l).T @ np.abs(xR))
        a = np.minimum(nb - rows_i, 65 if width == 1 else 128)
        AX = np.abs(Xl).T
        bound = gamma(a)[:, None] * (AX @ (np.abs(t) + delta)) + AX @ delta
        res["x"] = worst(np.abs(co[k0:k1].astype(LD) - Xl.T @ t), bound)
    elif op == 3:
        cB, zB = ci[k0:k1].astype(LD), yi[k0:k1].astype(LD)
        res["block"] = worst(np.abs(co[k0:k1].astype(LD) - (cB + L11l @ zB)),
                             gamma(rows_i + 2)[:, None] * (np.abs(cB) + np.abs(L11l) @ np.abs(zB)))
        res["rows"] = worst(np.abs(got - (old + L21l @ zB)), gamma(nb + 1) * (np.abs(old) + np.abs(L21l) @ np.abs(zB)))
    else:
        zB, zR = yi[k0:k1].astype(LD), yi[k1:m].astype(LD)
        a = np.maximum(nb - rows_i, min(nR, 67)) + ng
        res["x"] = worst(np.abs(co[k0:k1].astype(LD) - (L11l.T @ zB + L21l.T @ zR)),
                         gamma(a)[:, None] * (np.abs(L11l).T @ np.abs(zB) + np.abs(L21l).T @ np.abs(zR)))
    return res


def asserted(res):
    """The worst asserted ratio of a check's result (the reported ones left out)."""
    return max(v for k, v in res.items() if "reported" not in k)


def fmt(res):
    return ", ".join(f"{k} {v:.3f}" for k, v in res.items())


# ---------------------------------------------------------------------------------------
# numpy double emulations of the kernels' arithmetic (in numpy's order), and their mutants
# ---------------------------------------------------------------------------------------
MUTANTS = {
    # name: (op, width, family, the shape that must catch it)
    "drop_k": (1, 1, "W", (65, 64, 0)),            # one K term dropped from a product
    "partial_twice": (2, 16, "W", (385, 128, 0)),  # one GEMV partial (a one-row task's) added twice
    "e_sign": (0, 1, "K", (100, 65, 0)),           # E with the wrong sign
    "diag_as_l": (1, 1, "W", (1, 1, 0)),           # the diagonal of X taken as L(i, i)
    "skip_last_row": (1, 16, "W", (385, 128, 0)),  # the last row of a partial tile skipped
    "swap_u_c": (1, 1, "W", (300, 200, 0)),        # row r = w written to c, not u
    "read_upper": (3, 16, "W", (450, 193, 128)),   # a product reads one entry above the diagonal
}


def _dot_tree(A, V, size):
    """A V as the kernels cut it: products over chunks of `size` terms (numpy's order inside
    a chunk, no deeper than its length), the chunks' results added left to right."""
    acc = np.zeros((A.shape[0], V.shape[1]))
    for j in range(0, A.shape[1], size):
        p = A[:, j:j + size] @ V[j:j + size]
        acc = p if j == 0 else acc + p
    return acc


def emulate(op, width, m, w, k0, ins, mutant=None):
    """The step on host buffers in numpy double; returns the four output buffers.  Where a
    bound counts on the kernels' cut of a sum (chains of 16 and the quadrants in the forward
    block product, quarters of 64 rows in a partial, halves of 64 in the backward block
    product), the sum is cut the same way here."""
    nb, k1, nR, ng = dims(m, w, k0)
    outs = [b.copy() for b in ins]
    Fi, Fo = fview(ins[0], m, w), fview(outs[0], m, w)
    L11, L21 = lower(Fi, m, w, k0)
    if op == 0:
        X = np.zeros((nb, nb))
        for a in (0, PNB):
            n = min(PNB, nb - a)
            if n <= 0:
                continue
            La, Xa, eye = L11[a:a + n, a:a + n], np.zeros((n, n)), np.eye(n)
            invd = 1.0 / np.diag(La)
            for q in range(n):
                Xa[q] = (eye[q] - La[q, :q] @ Xa[:q]) * invd[q]
            X[a:a + n, a:a + n] = Xa
        if nb > PNB:
            E = X[PNB:, PNB:] @ (L11[PNB:, :PNB] @ X[:PNB, :PNB])
            X[PNB:, :PNB] = E if mutant == "e_sign" else -E
        up = np.triu_indices(nb, 1)
        Fo[k0:k1, k0:k1][up] = X.T[up]
        return outs
    ci, yi, ui = vview(ins[1], m, width), vview(ins[2], yrows(m, w, op), width), vview(ins[3], m - w, width)
    co, yo, uo = vview(outs[1], m, width), vview(outs[2], yrows(m, w, op), width), vview(outs[3], m - w, width)

    def below(acc, sign):  # rows below the block: to c for r < w, to u for the rest
        new = np.vstack([ci[k1:w], ui]) + sign * acc
        if mutant == "skip_last_row" and nR % ROWS:
            new[-1] = np.vstack([ci[k1:w], ui])[-1]
        co[k1:w] = new[:w - k1]
        uo[:] = new[w - k1:]
        if mutant == "swap_u_c" and k1 <= w < m:
            uo[0] = ui[0]
            co[w] = ci[w] + sign * acc[w - k1]

    def partials(V):  # one per GEMV task, in task order
        return [_dot_tree(L21[g * ROWS:(g + 1) * ROWS].T, V[g * ROWS:(g + 1) * ROWS], PNB) for g in range(ng)]

    if op == 1:
        X = inverse(Fi, m, w, k0, diag_as_l=mutant == "diag_as_l")
        cB = ci[k0:k1]
        y = _dot_tree(X[:PNB, :PNB], cB[:PNB], 16)
        if nb > PNB:
            y = np.vstack([y, _dot_tree(X[PNB:, :PNB], cB[:PNB], 16) + _dot_tree(X[PNB:, PNB:], cB[PNB:], 16)])
        yo[k0:k1] = y
        below(L21[:, :-1] @ y[:-1] if mutant == "drop_k" else L21 @ y, -1.0)
    elif op == 2:
        X = inverse(Fi, m, w, k0)
        t = ci[k0:k1].copy()
        ps = partials(ci[k1:m])
        for p in ps + (ps[-1:] if mutant == "partial_twice" else []):
            t = t + (-p)
        co[k0:k1] = _dot_tree(X.T, t, PNB)
    elif op == 3:
        A = L11.copy()
        if mutant == "read_upper" and nb > 1:
            A[0, nb - 1] = Fi[k0, k1 - 1]
        co[k0:k1] = ci[k0:k1] + A @ yi[k0:k1]
        below(L21 @ yi[k0:k1], 1.0)
    else:
        x = L11.T @ yi[k0:k1]
        for p in partials(yi[k1:m]):
            x = x + p
        co[k0:k1] = x
    return outs


def with_inverse(m, w, k0, family, run_op0):
    """The panel ops 1 and 2 work on: panel() after an op 0 step; run_op0(ins) -> outs."""
    ins = (panel(m, w, k0, family),) + vectors(m, w, k0, 0, 1)
    fbuf = run_op0(ins)[0].copy()
    fbuf.setflags(write=False)
    return fbuf


def inputs(op, width, m, w, k0, family, run_op0):
    """The four input buffers of a case; op 0 works on the panel with the rows below poisoned."""
    if op == 0:
        f = panel(m, w, k0, family, rows_below=False)
    elif op in (1, 2):
        f = with_inverse(m, w, k0, family, run_op0)
    else:
        f = panel(m, w, k0, family)
    return (f,) + vectors(m, w, k0, op, width)


# ---------------------------------------------------------------------------------------
# the gather
# ---------------------------------------------------------------------------------------
GATHER_W, GATHER_MB = 40, 1300
GATHER_SIZES = (1025, 0, 255, 1, 257, 256)  # 1025: past the panel kernel's 1024 threads


@functools.lru_cache(maxsize=None)
def gather_case(width):
    """(rel_ptr, relind, ucbuf, cbuf, ubuf): children whose targets overlap, on both sides of
    w, with values spread over sixteen orders of magnitude, so another order of the adds
    changes bits; c and u preloaded."""
    rng = np.random.default_rng([width, 4242])
    n = GATHER_W + GATHER_MB
    rel_ptr = np.concatenate([[0], np.cumsum(GATHER_SIZES)]).astype(np.int64)
    relind = np.concatenate([rng.permutation(n)[:sz] for sz in GATHER_SIZES]).astype(np.int32)
    relind[rel_ptr[3]] = GATHER_W - 1  # the one-entry child: the last pivot row
    first = relind[:GATHER_SIZES[0]]
    assert (first < GATHER_W).any() and (first >= GATHER_W).any() and GATHER_W - 1 in first
    tot = int(rel_ptr[-1])
    bufs = []
    for rows in (tot, GATHER_W, GATHER_MB):
        buf = rng.standard_normal(1 + rows * width + CANARY)
        bufs.append(buf)
    uc = vview(bufs[0], tot, width)
    uc *= 10.0 ** rng.uniform(-8, 8, uc.shape)
    for b in bufs:
        b.setflags(write=False)
    return rel_ptr, relind, bufs[0], bufs[1], bufs[2]


def gather_reference(width, order=None):
    """c and u buffers after the adds, child by child (order: of the children), in double."""
    rel_ptr, relind, ucbuf, cbuf, ubuf = gather_case(width)
    cout, uout = cbuf.copy(), ubuf.copy()
    uc = vview(ucbuf, int(rel_ptr[-1]), width)
    c, u = vview(cout, GATHER_W, width), vview(uout, GATHER_MB, width)
    for q in (range(len(GATHER_SIZES)) if order is None else order):
        t, v = relind[rel_ptr[q]:rel_ptr[q + 1]], uc[rel_ptr[q]:rel_ptr[q + 1]]
        pc, pu = t < GATHER_W, t >= GATHER_W
        c[t[pc]] += v[pc]  # injective within a child: one add per target
        u[t[pu] - GATHER_W] += v[pu]
    return cout, uout
