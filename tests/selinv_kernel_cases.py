"""Cases, long-double references, checks and numpy emulations for the selected-inversion kernels
alone (sc_debug_selinv_step, sc_debug_selinv_push), shared by test_selinv_kernels_gpu.py (the
kernels) and test_selinv_kernel_cases_cpu.py (the emulations and their mutants: the bounds are
attainable, and a wrong kernel would miss them).  Built on solve_kernel_cases.py: gamma,
require_long_double, the families W and K of factor / panel, the one-double lead-in, the 8
canary doubles and the untouched() idea are that module's.

One step works on block K = [k0, k1), nb = min(128, w - k0), k1 = k0 + nb, of a front of m rows
and w pivots whose row list is the identity; R = [k1, m), nr = |R|, mb = m - w.  L and Z are m x
w panels (column-major, ld = m), Z_II is mb x mb (ld = mb), W is nr x nb (ld = nr).  X = inv(L_KK)
is read in its stored form: X(i, k), k < i, at row k, column i of the block (the strict upper
triangle an sc_debug_solve_step op 0 call filled), X(i, i) = 1 / L(i, i), zero above.
  op 0  W = L_RK X                  sel_w_kernel, one workgroup per 64 rows of R
  op 1  Z_RK = -Z_RR W, its mirror  sel_zrk_kernel, the same tiles
  op 2  Z_KK = X^T X - W^T Z_RK     sel_zkk_kernel per 64 x 64 tile (0, 0), (1, 0), (1, 1); for
        K = nb + nr > 512 one workgroup per chunk of 256 terms of the K range (the nb terms of
        X^T X, then the nr of -W^T Z_RK) and sel_zkk_reduce_kernel per tile
The hook returns the workgroups launched; tasks() is what the library's rule gives, and check()
holds the hook (or an emulation) to it: that is what tells the split rule K > 512 from K >= 512,
whose results both meet the bounds.

Read and write sets, from the kernels (kernels.hip: sel_x, sel_zfront, sel_mma's range checks):
  sel_x(i, k) returns 0 for k > i without a load, else the panel entry (row k0 + k, column k0 +
    i) of L, k <= i: the block's diagonal and strict upper triangle.  The strict LOWER triangle
    of L's diagonal block is read by no op.
  op 0 reads the block's diagonal and strict upper triangle of L and L(R, K); writes W.  Z, Z_II
    are not touched.
  op 1 reads W and Z_RR(i, k) = sel_zfront(k1 + i, k1 + k): for a column q = k1 + k < w the panel
    entry (p, q), any row p in R -- the pivot square [k1, w)^2 in both triangles and the rows >=
    w straight; for q >= w and p < w the panel entry (q, p) -- the same rows >= w, transposed;
    else Z_II(p - w, q - w), both triangles.  So: rows R of columns [k1, w) of Z, all of Z_II.
    Writes rows R of columns K of Z and, for p < w, the mirror: rows K of columns [k1, w).  L is
    not touched; columns K of Z are not read; rows < k1 of columns >= k1 are not read.
  op 2 reads the block's diagonal and strict upper triangle of L, W, and rows R of columns K of
    Z (Z_RK); writes rows K x columns K of Z (entries i >= j, each to both triangles).  Z_RR,
    Z_II, the old Z_KK and L below the block are not read.
  every op: columns of L outside K and rows of L above k0 are not read; columns of Z before k0
    are neither read nor written.
  push reads element (max(pa, pb), min(pa, pb)) of the front: the panel's lower trapezoid and the
    lower triangle of Z_II; the strict upper triangles of the pivot square and of Z_II never.
Everything outside an op's read set is NaN (op 0: all of Z and Z_II; op 1: all of L; op 2: Z_II,
L below the block), W before op 0 too.  A finite result proves the claim.  Operands start one
double into their allocations and end in 8 canary doubles; what a step may write is put back
from the input and the whole buffers are compared bitwise (untouched()).

Data.  L: families W and K of solve_kernel_cases (K: the inverse grows to 3.4e4 away from the
diagonal).  Z_RR and Z_II: one symmetric matrix, uniform in (-1, 1): the kernels are linear
algebra, Z need not be an inverse.  Ops 1 and 2 run on the W and Z_RK the device (or the
emulation) itself produced, and every product is held against its own operands as they were left
(X^, W^, Z^_RK), so a bound covers one kernel.

Bounds.  Derived, not measured; entry by entry; u = 2^-53, gamma_k = k u / (1 - k u), with the
assumptions of solve_kernel_cases: exact zeros (the zeros of X, dead lanes and tails, which
sel_mma loads as 0.0) add no rounding; an fp64 MFMA chain over n live terms is within gamma_n;
no term of a sum passes more roundings than the gamma index; 1.0 / L(i, i) is the correctly
rounded quotient; negation is exact.
  W(i, j) = sum_{k >= j} L_RK(i, k) X(k, j): nb - j live terms.
    |W^ - L_RK X^| <= gamma_{nb-j} |L_RK| |X^|.
  Z_RK: nr terms, one negation.  |Z^_RK + Z_RR W^| <= gamma_nr |Z_RR| |W^|.
  Z_KK(i, j), i >= j: X(k, i) X(k, j) lives for k >= i: nb - i terms, and nr of W^T Z_RK.
    unsplit: gamma_{nb-i+nr} (|X^|^T |X^| + |W^|^T |Z^_RK|)_ij.
    split into nch chunks [256 c, min(K, 256 c + 256)): chunk c has live_c(i) = max(0, min(K,
    256 c + 256) - max(i, 256 c)) live terms (<= 256), one MFMA chain; the reduction starts from
    0.0 + part_0, which is exact, and adds nch - 1 times: gamma_{max_c live_c(i) + nch - 1}.
    The upper triangle is the lower one's bits, so entry (i, j) takes the index of max(i, j).
The counts are as the issue that asked for these tests read them; none turned out different.
The references are long double (u_ld = 2^-64 = 2^-11 u).  They sum as many live terms as the
kernels: nb - j for W, nr for Z_RK, nb - i + nr (and one subtraction) for Z_KK, against a gamma
index that is the same but for the split Z_KK, where it is max_c live_c + nch - 1 >= 256: at most
2.4 times as many terms as the index over SHAPES ((600, 64, 0): 600 against 258; the CPU test
asserts < 4).  So a reference's own rounding is below 4 * 2^-11 = 2^-9 of a bound, and worst()
takes every bound times 1 + 2^-9.
The push has no bound: it equals numpy indexing of the symmetric front bit for bit.
"""
import functools

import numpy as np

import solve_kernel_cases as S
from solve_kernel_cases import CANARY, FAMILIES, LD, fview, gamma, require_long_double, shape_id  # noqa: F401

BM, KT, KC, KSPLIT = 64, 64, 256, 512

# (m, w, k0): the smallest shapes that reach each path
SHAPES = [
    (1, 1, 0),          # nb = 1, nr = 0: Z_KK = fl(1 / l)^2, no W / Z_RK launch
    (64, 64, 0),        # full 64-block, nr = 0
    (65, 64, 0),        # nr = 1: R is contribution rows only
    (100, 65, 0),       # nb = 65: the quadrant tiles with one row / column; K = nb is no multiple of 4
    (128, 128, 0),      # full 128-block, no rows below
    (129, 128, 0),      # one row below a full 128-block
    (192, 128, 0),      # exactly one 64-row tile
    (193, 128, 0),      # a second tile of one row
    (300, 200, 0),      # R spans own pivots and contribution rows: every form of Z_RR, the mirror
    (300, 200, 128),    # k0 > 0, nb = 72, no mirror (k1 = w)
    (400, 300, 128),    # k0 > 0 with the mirror (k1 = 256 < w)
    (450, 193, 128),    # nb = 65, nr = 257
    (512, 128, 0),      # K = 512: the last unsplit depth
    (513, 128, 0),      # K = 513: three chunks, the last of one term
    (600, 64, 0),       # split with nb = 64: one tile, the X^T X / W^T Z_RK seam inside chunk 0
    (700, 320, 256),    # nb = 64 at k0 = 256
]
OPS = (0, 1, 2)
NAMES = {0: "sel_w", 1: "sel_zrk", 2: "sel_zkk"}
PUSH_PARENT = (200, 90)
PUSH_SIZES = (1, 64, 65, 130)


def dims(m, w, k0):
    """nb, k1 = k0 + nb, nr = rows below, mb = contribution rows."""
    nb, k1, nr, _ = S.dims(m, w, k0)
    return nb, k1, nr, m - w


def kchunks(K, split_ge=False):
    """selinv_kchunks: one product up to K = 512, else chunks of 256 (split_ge: the wrong rule)."""
    return 1 if (K < KSPLIT if split_ge else K <= KSPLIT) else -(-K // KC)


def tasks(m, w, k0, op, split_ge=False):
    """Workgroups the library launches for the step: 64-row tiles (ops 0, 1); per tile of Z_KK's
    lower triangle one product, or nch chunk products and one reduction (op 2)."""
    nb, _, nr, _ = dims(m, w, k0)
    if op < 2:
        return -(-nr // BM)
    nch, ntile = kchunks(nb + nr, split_ge), 1 if nb <= KT else 3
    return ntile if nch == 1 else ntile * (nch + 1)


def zkk_depth(m, w, k0):
    """The gamma index of Z_KK's row i (i >= j), and the live terms the reference sums there."""
    nb, _, nr, _ = dims(m, w, k0)
    i, K = np.arange(nb), nb + nr
    nch = kchunks(K)
    live = nb - i + nr
    if nch == 1:
        return live, live
    per = [np.maximum(0, min(K, KC * c + KC) - np.maximum(i, KC * c)) for c in range(nch)]
    return np.max(per, axis=0) + nch - 1, live


def iview(buf, mb):
    return buf[1:1 + mb * mb].reshape(mb, mb).T


def wview(buf, nr, nb):
    return buf[1:1 + nr * nb].reshape(nb, nr).T


def _blank(n, seed):
    """lead-in, n NaN, canaries"""
    rng = np.random.default_rng(seed)
    buf = np.full(1 + n + CANARY, np.nan)
    buf[0] = rng.standard_normal()
    buf[1 + n:] = rng.standard_normal(CANARY)
    return buf


@functools.lru_cache(maxsize=None)
def zsym(m, w, k0):
    """The symmetric m x m matrix Z_RR and Z_II are cut from."""
    A = np.random.default_rng([m, w, k0, 901]).uniform(-1, 1, (m, m))
    Z = np.tril(A) + np.tril(A, -1).T
    Z.setflags(write=False)
    return Z


def inputs(op, m, w, k0, family, run_inv, prev=None):
    """(lbuf, zbuf, ibuf, wbuf) of a case.  run_inv(ins) -> outs runs op 0 of the SOLVE step
    (the block inverses); prev: the output buffers of this module's op - 1 on the same shape and
    family (op 1 takes its W, op 2 its W and Z_RK)."""
    nb, k1, nr, mb = dims(m, w, k0)
    lbuf = S.with_inverse(m, w, k0, family, run_inv).copy()
    L = fview(lbuf, m, w)
    L[k0:k1, k0:k1][np.tril_indices(nb, -1)] = np.nan  # no op reads the block's strict lower triangle
    if op == 1:
        L[:] = np.nan
    elif op == 2:
        L[k1:, k0:k1] = np.nan
    zbuf, ibuf = _blank(m * w, [m, w, k0, 902]), _blank(mb * mb, [m, w, k0, 903])
    wbuf = _blank(nr * nb, [m, w, k0, 904]) if op == 0 else prev[3].copy()
    Z = fview(zbuf, m, w)
    if op == 1:
        Z[k1:, k1:w] = zsym(m, w, k0)[k1:, k1:w]
        iview(ibuf, mb)[:] = zsym(m, w, k0)[w:, w:]
    elif op == 2:
        Z[k1:, k0:k1] = fview(prev[1], m, w)[k1:, k0:k1]
    out = (lbuf, zbuf, ibuf, wbuf)
    for b in out:
        b.setflags(write=False)
    return out


def zrr(ins, m, w, k0, transposed_only=False):
    """Z_RR (nr x nr) as sel_zfront assembles it from the Z panel and Z_II.  transposed_only:
    the wrong kernel that takes rows >= w of a pivot column from the transposed address p m + q
    too -- past the panel's last column, whatever lies there (NaN beyond the buffer)."""
    nb, k1, nr, mb = dims(m, w, k0)
    Z, npiv = fview(ins[1], m, w), w - k1
    R = np.empty((nr, nr))
    R[:, :npiv] = Z[k1:, k1:w]
    R[:npiv, npiv:] = Z[w:, k1:w].T
    R[npiv:, npiv:] = iview(ins[2], mb)
    if transposed_only and npiv and mb:
        flat = np.concatenate([ins[1][1:], np.full(m * m, np.nan)])
        p, q = np.meshgrid(np.arange(w, m), np.arange(k1, w), indexing="ij")
        R[npiv:, :npiv] = flat[p * m + q]
    return R


# ---------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------
def worst(err, bound):
    """max err / bound; a zero bound demands a zero error; anything non-finite is inf."""
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    if err.size == 0:
        return 0.0
    if not (np.all(np.isfinite(err)) and np.all(np.isfinite(bound))):
        return float("inf")
    bound = bound * (1 + LD(2.0) ** -9)  # the long-double reference's own rounding
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1), np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def same_bits(a, b):
    return bool(np.array_equal(_bits(a), _bits(b)))


def untouched(m, w, k0, op, ins, outs):
    """True when everything the step must not write came back bitwise: all of L and Z_II, Z
    outside the step's window, W unless op 0 owns it, lead-ins and canaries."""
    nb, k1, nr, mb = dims(m, w, k0)
    kept = [o.copy() for o in outs]
    Zi, Zk = fview(ins[1], m, w), fview(kept[1], m, w)
    if op == 0:
        kept[3][1:1 + nr * nb] = ins[3][1:1 + nr * nb]
    elif op == 1:
        Zk[k1:, k0:k1] = Zi[k1:, k0:k1]
        Zk[k0:k1, k1:w] = Zi[k0:k1, k1:w]
    else:
        Zk[k0:k1, k0:k1] = Zi[k0:k1, k0:k1]
    return all(same_bits(a, b) for a, b in zip(kept, ins))


def check(op, m, w, k0, ins, outs, count):
    """{name: worst error / bound, or 0 / inf for a property} of one step; count: the workgroups
    the hook (or the emulation) reports."""
    require_long_double()
    nb, k1, nr, mb = dims(m, w, k0)
    res = {"untouched": 0.0 if untouched(m, w, k0, op, ins, outs) else float("inf"),
           "tasks": 0.0 if count == tasks(m, w, k0, op) else float("inf")}
    Li, Zi, Zo = fview(ins[0], m, w), fview(ins[1], m, w), fview(outs[1], m, w)
    if op != 1:
        Xl = S.inverse(Li, m, w, k0).astype(LD)
    if op == 0:
        Lrk = Li[k1:, k0:k1].astype(LD)
        got = wview(outs[3], nr, nb).astype(LD)
        res["W"] = worst(np.abs(got - Lrk @ Xl), gamma(nb - np.arange(nb))[None, :] * (np.abs(Lrk) @ np.abs(Xl)))
    elif op == 1:
        R, Wl = zrr(ins, m, w, k0).astype(LD), wview(ins[3], nr, nb).astype(LD)
        got = Zo[k1:, k0:k1]
        res["Z_RK"] = worst(np.abs(got.astype(LD) + R @ Wl), gamma(nr) * (np.abs(R) @ np.abs(Wl)))
        ok = same_bits(Zo[k0:k1, k1:w], got[:w - k1].T) and bool(np.isfinite(Zo[k0:k1, k1:w]).all())
        res["mirror"] = 0.0 if ok else float("inf")
    else:
        Wl, Zrk = wview(ins[3], nr, nb).astype(LD), Zi[k1:, k0:k1].astype(LD)
        got = Zo[k0:k1, k0:k1]
        d = zkk_depth(m, w, k0)[0]
        D = d[np.maximum.outer(np.arange(nb), np.arange(nb))]
        res["Z_KK"] = worst(np.abs(got.astype(LD) - (Xl.T @ Xl - Wl.T @ Zrk)),
                            gamma(D) * (np.abs(Xl).T @ np.abs(Xl) + np.abs(Wl).T @ np.abs(Zrk)))
        res["symmetric"] = 0.0 if same_bits(got, got.T) else float("inf")
    return res


def asserted(res):
    return max(res.values())


def fmt(res):
    return ", ".join(f"{k} {v:.3f}" for k, v in res.items())


# ---------------------------------------------------------------------------------------
# numpy double emulations of the kernels' arithmetic, and their mutants
# ---------------------------------------------------------------------------------------
MUTANTS = {
    # name: (op, family, the shape that must catch it, the check that does)
    "drop_ktail_w": (0, "W", (100, 65, 0), "W"),            # the last K % 16 terms dropped (K = nb = 65)
    "drop_ktail_zrk": (1, "W", (193, 128, 0), "Z_RK"),      # the same in Z_RK (K = nr = 65)
    "drop_ktail_zkk": (2, "K", (300, 200, 128), "Z_KK"),    # and in Z_KK (K = 172)
    "diag_as_l": (2, "W", (1, 1, 0), "Z_KK"),               # the diagonal of X taken as L(i, i)
    "x_strict_lower": (0, "W", (100, 65, 0), "W"),          # X read from the strict lower triangle: poison
    "seam_twice": (2, "W", (513, 128, 0), "Z_KK"),          # chunk 0 runs one term into chunk 1
    "seam_skip": (2, "W", (600, 64, 0), "Z_KK"),            # chunk 1 starts one term late
    "split_ge": (2, "W", (512, 128, 0), "tasks"),           # split at K >= 512: only the task count tells
    "no_mirror": (1, "W", (300, 200, 0), "mirror"),         # the pivot square's mirror not written
    "zrk_sign": (1, "W", (65, 64, 0), "Z_RK"),              # Z_RK = +Z_RR W
    "zrr_transposed_only": (1, "W", (300, 200, 0), "Z_RK"),  # rows >= w read at p m + q: past the panel
}


def emulate(op, m, w, k0, ins, mutant=None):
    """The step on host buffers in numpy double; returns (output buffers, workgroups).  Sums are
    numpy's own order inside one product (a chunk of the split Z_KK is one product), the chunks
    are added in chunk order from 0.0 as sel_zkk_reduce_kernel adds them."""
    nb, k1, nr, mb = dims(m, w, k0)
    outs = [b.copy() for b in ins]
    if op < 2 and nr == 0:
        return outs, 0
    Li, Zi, Zo = fview(ins[0], m, w), fview(ins[1], m, w), fview(outs[1], m, w)
    tail = (lambda K: K - K % 16) if mutant and mutant.startswith("drop_ktail") else (lambda K: K)
    if op != 1:
        X = S.inverse(Li, m, w, k0, diag_as_l=mutant == "diag_as_l")
        if mutant == "x_strict_lower":
            X = np.tril(Li[k0:k1, k0:k1], -1) + np.diag(np.diag(X))
    if op == 0:
        wview(outs[3], nr, nb)[:] = Li[k1:, k0:k1][:, :tail(nb)] @ X[:tail(nb)]
        return outs, tasks(m, w, k0, 0)
    W = wview(ins[3], nr, nb)
    if op == 1:
        R = zrr(ins, m, w, k0, transposed_only=mutant == "zrr_transposed_only")
        P = R[:, :tail(nr)] @ W[:tail(nr)]
        Zrk = P if mutant == "zrk_sign" else -P
        Zo[k1:, k0:k1] = Zrk
        if mutant != "no_mirror":
            Zo[k0:k1, k1:w] = Zrk[:w - k1].T
        return outs, tasks(m, w, k0, 1)
    # one K range: the nb terms of X^T X, then the nr terms of (-W)^T Z_RK
    A, B, K = np.hstack([X.T, -W.T]), np.vstack([X, Zi[k1:, k0:k1]]), nb + nr
    nch = kchunks(K, split_ge=mutant == "split_ge")
    if nch == 1:
        V = A[:, :tail(K)] @ B[:tail(K)]
    else:
        V = np.zeros((nb, nb))
        for c in range(nch):
            kb, ke = KC * c, min(K, KC * c + KC)
            if c == 0 and mutant == "seam_twice":
                ke += 1
            if c == 1 and mutant == "seam_skip":
                kb += 1
            V = V + A[:, kb:ke] @ B[kb:ke]
    Zo[k0:k1, k0:k1] = np.tril(V) + np.tril(V, -1).T  # the lower triangle decides both
    return outs, tasks(m, w, k0, 2, split_ge=mutant == "split_ge")


# ---------------------------------------------------------------------------------------
# the push
# ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def push_case(mbc):
    """(relind, zbuf, ibuf, obuf): the parent's Z with NaN in the strict upper triangles of its
    pivot square and of Z_II; relind ascending, mbc // 2 pivot positions and the rest
    contribution positions (mbc = 1: the first contribution row); obuf preloaded."""
    m, w = PUSH_PARENT
    mb = m - w
    rng = np.random.default_rng([mbc, 905])
    Zs = zsym(m, w, 0)
    zbuf, ibuf = _blank(m * w, [mbc, 906]), _blank(mb * mb, [mbc, 907])
    Z, Zii = fview(zbuf, m, w), iview(ibuf, mb)
    Z[:] = Zs[:, :w]
    Z[:w][np.triu_indices(w, 1)] = np.nan
    Zii[:] = Zs[w:, w:]
    Zii[np.triu_indices(mb, 1)] = np.nan
    npiv = mbc // 2
    rel = np.sort(np.concatenate([rng.choice(w, npiv, replace=False),
                                  w + rng.choice(mb, mbc - npiv, replace=False) if mbc > 1 else [w]])).astype(np.int32)
    obuf = rng.standard_normal(1 + mbc * mbc + CANARY)
    for b in (rel, zbuf, ibuf, obuf):
        b.setflags(write=False)
    return rel, zbuf, ibuf, obuf


def push_emulate(mbc, upper=False):
    """The output buffer after the push, from the buffers as stored: element (max, min) of the
    front (upper: the wrong kernel's (min, max))."""
    m, w = PUSH_PARENT
    rel, zbuf, ibuf, obuf = push_case(mbc)
    F = np.full((m, m), np.nan)
    F[:, :w] = fview(zbuf, m, w)
    F[:w, w:] = fview(zbuf, m, w)[w:].T
    F[w:, w:] = iview(ibuf, m - w)
    pa, pb = np.meshgrid(rel, rel, indexing="ij")
    hi, lo = np.maximum(pa, pb), np.minimum(pa, pb)
    out = obuf.copy()
    out[1:1 + mbc * mbc] = (F[lo, hi] if upper else F[hi, lo]).T.ravel()
    return out


def push_reference(mbc):
    """The output buffer the push must leave: numpy Zfront[np.ix_(rel, rel)] of the symmetric
    front built from the lower triangles alone."""
    m, w = PUSH_PARENT
    rel, zbuf, ibuf, obuf = push_case(mbc)
    F = np.zeros((m, m))
    F[:, :w] = np.tril(fview(zbuf, m, w))
    F[w:, w:] = np.tril(iview(ibuf, m - w))
    F = F + np.tril(F, -1).T
    out = obuf.copy()
    out[1:1 + mbc * mbc] = F[np.ix_(rel, rel)].T.ravel()
    return out
