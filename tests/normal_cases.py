"""Cases, exact references and numpy emulations shared by the normal-equations tests.

S = C + J^T diag(w) J + diag(d) + lambda I.  What a test compares against is computed here in
rational arithmetic (fractions.Fraction on the fp64 inputs), from dense copies of the small
matrices, so nothing under test is its own yardstick.  The numpy emulations restate what the
kernels and the least-squares iteration do; test_normal_cases_cpu.py checks them (and
deliberately wrong variants of them) against the exact values without a GPU, before the GPU
tests rely on the bounds and caps they justify.
"""
from fractions import Fraction

import numpy as np

import sparsecholesky_amd as sc

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


# --------------------------------------------------------------------------
# matrices
# --------------------------------------------------------------------------
def csc_of(D, mask=None, upper=False):
    """Dense array (entries where mask, default: nonzero) as a csc_matrix, rows ascending."""
    D = np.asarray(D, dtype=np.float64)
    m, n = D.shape
    mask = (D != 0) if mask is None else np.asarray(mask, dtype=bool)
    p = np.zeros(n + 1, dtype=np.int64)
    ii, xx = [], []
    for j in range(n):
        for i in np.flatnonzero(mask[:, j]):
            if upper and i > j:
                continue
            ii.append(i), xx.append(D[i, j])
        p[j + 1] = len(ii)
    return sc.csc_matrix(m, n, p, np.array(ii, dtype=np.int32), np.array(xx, dtype=np.float64),
                         sc.sym.upper if upper else sc.sym.none)


def dense_of(A):
    D = np.zeros((A.n_rows, A.n_cols))
    for j in range(A.n_cols):
        for q in range(int(A.p[j]), int(A.p[j + 1])):
            D[int(A.i[q]), j] = A.x[q]
    return D


def mask_of(A):
    M = np.zeros((A.n_rows, A.n_cols), dtype=bool)
    for j in range(A.n_cols):
        M[A.i[int(A.p[j]):int(A.p[j + 1])], j] = True
    return M


def random_sparse(m, n, density, seed, empty_cols=(), empty_rows=()):
    rng = np.random.default_rng(seed)
    M = rng.random((m, n)) < density
    M[:, list(empty_cols)] = False
    M[list(empty_rows), :] = False
    return csc_of(np.where(M, rng.standard_normal((m, n)), 0.0), M)


def two_dense_columns(m, seed):
    """m x 2 dense: each of the three entries of S has a list of m terms."""
    rng = np.random.default_rng(seed)
    return csc_of(rng.standard_normal((m, 2)), np.ones((m, 2), dtype=bool))


def expected_pattern(J, base=None):
    """Upper CSC pattern of S from dense boolean algebra: J^T J, C and the diagonal."""
    n = J.n_cols
    M = mask_of(J).astype(np.int64)
    P = (M.T @ M) > 0
    if base is not None:
        P |= mask_of(base)
    P |= np.eye(n, dtype=bool)
    P = np.triu(P)
    Sp = np.zeros(n + 1, dtype=np.int64)
    Si = []
    for j in range(n):
        Si.extend(np.flatnonzero(P[:, j]).tolist())
        Sp[j + 1] = len(Si)
    return Sp, np.array(Si, dtype=np.int32)


def expected_terms(J, base=None):
    """Per entry of expected_pattern: [(pa, pb, r), ..] with rows ascending, and the position in
    the base's value array or -1, from dictionaries over J's raw arrays."""
    n = J.n_cols
    at = {}
    for j in range(n):
        for q in range(int(J.p[j]), int(J.p[j + 1])):
            at[(int(J.i[q]), j)] = q
    cat = {}
    if base is not None:
        for j in range(n):
            for q in range(int(base.p[j]), int(base.p[j + 1])):
                cat[(int(base.i[q]), j)] = q
    Sp, Si = expected_pattern(J, base)
    lists, cpos = [], []
    for j in range(n):
        for e in range(int(Sp[j]), int(Sp[j + 1])):
            i = int(Si[e])
            lists.append([(at[(r, i)], at[(r, j)], r) for r in range(J.n_rows) if (r, i) in at and (r, j) in at])
            cpos.append(cat.get((i, j), -1))
    return lists, cpos


# --------------------------------------------------------------------------
# exact arithmetic
# --------------------------------------------------------------------------
def _fr(v):
    return Fraction(float(v))


def exact_form(J, Jx, w, base, Cx, d, lam):
    """(values, magnitudes, list lengths) per entry of expected_pattern, exactly:
    S_e = c_e + [i = j] (d_i + lam) + sum_r J[r, i] w_r J[r, j] and the bound's denominator
    |c_e| + |d_i + lam| + sum |J w J|."""
    lists, cpos = expected_terms(J, base)
    Sp, Si = expected_pattern(J, base)
    vals, mags, lens = [], [], []
    e = 0
    for j in range(J.n_cols):
        for q in range(int(Sp[j]), int(Sp[j + 1])):
            i = int(Si[q])
            c = _fr(Cx[cpos[e]]) if (Cx is not None and cpos[e] >= 0) else Fraction(0)
            sh = ((_fr(d[i]) if d is not None else Fraction(0)) + _fr(lam)) if i == j else Fraction(0)
            s, a = c + sh, abs(c) + abs(sh)
            for (pa, pb, r) in lists[e]:
                t = _fr(Jx[pa]) * (_fr(w[r]) if w is not None else 1) * _fr(Jx[pb])
                s += t
                a += abs(t)
            vals.append(s), mags.append(a), lens.append(len(lists[e]))
            e += 1
    return vals, mags, lens


def exact_mul(J, Jx, x, b=None):
    """Per row r: (b_r - sum_j J[r, j] x_j, or the plain product without b; |b_r| + sum |J| |x|; row length)."""
    m = J.n_rows
    s = [Fraction(0) if b is None else _fr(b[r]) for r in range(m)]
    a = [Fraction(0) if b is None else abs(_fr(b[r])) for r in range(m)]
    k = [0] * m
    sign = 1 if b is None else -1
    for j in range(J.n_cols):
        xj = _fr(x[j])
        for q in range(int(J.p[j]), int(J.p[j + 1])):
            r = int(J.i[q])
            t = _fr(Jx[q]) * xj
            s[r] += sign * t
            a[r] += abs(t)
            k[r] += 1
    return s, a, k


def exact_mult(J, Jx, w, y):
    """Per column j: (sum_r J[r, j] w_r y_r, sum |J w y|, column length)."""
    out = []
    for j in range(J.n_cols):
        s = a = Fraction(0)
        for q in range(int(J.p[j]), int(J.p[j + 1])):
            r = int(J.i[q])
            t = _fr(Jx[q]) * (_fr(w[r]) if w is not None else 1) * _fr(y[r])
            s += t
            a += abs(t)
        out.append((s, a, int(J.p[j + 1] - J.p[j])))
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def exact_solve(A, b):
    """Gaussian elimination over the rationals (A: list of lists of Fraction, nonsingular)."""
    n = len(b)
    M = [list(A[i]) + [b[i]] for i in range(n)]
    for k in range(n):
        piv = next(i for i in range(k, n) if M[i][k] != 0)
        M[k], M[piv] = M[piv], M[k]
        for i in range(k + 1, n):
            if M[i][k] != 0:
                f = M[i][k] / M[k][k]
                for c in range(k, n + 1):
                    M[i][c] -= f * M[k][c]
    x = [Fraction(0)] * n
    for k in range(n - 1, -1, -1):
        x[k] = (M[k][n] - sum(M[k][c] * x[c] for c in range(k + 1, n))) / M[k][k]
    return x


def exact_lstsq(Jd, w, b, Cd=None, d=None, lam=0.0):
    """The exact minimiser of ||W^1/2 (J x - b)||^2 + x^T (C + diag d + lam I) x: the rational
    solution of its normal equations (dense inputs; C full symmetric)."""
    m, n = Jd.shape
    Jf = [[_fr(Jd[r, j]) for j in range(n)] for r in range(m)]
    wf = [_fr(v) for v in w]
    S = [[sum(Jf[r][i] * wf[r] * Jf[r][j] for r in range(m)) for j in range(n)] for i in range(n)]
    for i in range(n):
        for j in range(n):
            if Cd is not None:
                S[i][j] += _fr(Cd[i, j])
        S[i][i] += (_fr(d[i]) if d is not None else 0) + _fr(lam)
    g = [sum(Jf[r][i] * wf[r] * _fr(b[r]) for r in range(m)) for i in range(n)]
    return exact_solve(S, g)


# --------------------------------------------------------------------------
# numpy emulations
# --------------------------------------------------------------------------
def emulate_form(lists, cpos, diag, Jx, w, Cx, d, lam, drop_weight=False, shift_everywhere=False):
    """The form in plain fp64, the base first, then every list in list order (one of the orders
    the derived bound covers).  diag[e]: the entry's column when diagonal, else -1.  The two
    flags produce deliberately wrong values."""
    out = np.zeros(len(lists))
    for e, terms in enumerate(lists):
        s = Cx[cpos[e]] if (Cx is not None and cpos[e] >= 0) else 0.0
        if diag[e] >= 0 or shift_everywhere:
            s = s + ((d[max(diag[e], 0)] if d is not None else 0.0) + lam)
        for (pa, pb, r) in terms:
            aw = Jx[pa] * w[r] if (w is not None and not drop_weight) else Jx[pa]
            s = s + aw * Jx[pb]
        out[e] = s
    return out


def diag_of(Sp, Si):
    n = len(Sp) - 1
    out = np.full(int(Sp[n]), -1, dtype=np.int32)
    for j in range(n):
        for e in range(int(Sp[j]), int(Sp[j + 1])):
            if Si[e] == j:
                out[e] = j
    return out


def base_times(Cu, d, lam, x, mirrored=True, dtype=np.longdouble):
    """(C + diag d + lam I) x for the upper-triangular dense Cu; mirrored=False forgets the
    strictly lower half (a deliberately wrong variant)."""
    n = len(x)
    xl = x.astype(dtype)
    y = np.zeros(n, dtype=dtype)
    if Cu is not None:
        Cl = np.triu(Cu).astype(dtype)
        y += Cl @ xl
        if mirrored:
            y += np.triu(Cu, 1).astype(dtype).T @ xl
    y += ((d.astype(dtype) if d is not None else 0) + dtype(lam)) * xl
    return y


CONVERGED, STALLED, MAXITER, DIVERGED = range(4)


def emulate_lstsq(Jd, w, b, Cu=None, d=None, lam=0.0, max_iter=10, rho_max=0.5, mirrored=True, pair=False):
    """The library's iteration on the host: S formed in fp64, a numpy Cholesky, x_0 = the plain
    normal-equations solve, then corrected semi-normal steps under the stopping rules of the
    refinement.  pair=False: the residual and the base product in longdouble, each rounded to
    fp64 (the emulation the error cap was set with).  pair=True models the library's
    compensated mode, which keeps the residual and the gradient as unevaluated pairs: both are
    formed exactly here and the gradient is rounded once.  Returns x, info."""
    m, n = Jd.shape
    JW = Jd.T * w
    S = JW @ Jd
    if Cu is not None:
        S = S + np.triu(Cu) + np.triu(Cu, 1).T
    S = S + np.diag((d if d is not None else np.zeros(n)) + lam)
    L = np.linalg.cholesky(S)

    def solve(g):
        return np.linalg.solve(L.T, np.linalg.solve(L, g))

    base = Cu is not None or d is not None or lam != 0.0

    def gradient_pair(x):
        xf = [_fr(v) for v in x]
        r = [_fr(b[i]) - sum(_fr(Jd[i, j]) * xf[j] for j in range(n)) for i in range(m)]
        g = [sum(_fr(Jd[i, j]) * _fr(w[i]) * r[i] for i in range(m)) for j in range(n)]
        if base:
            for i in range(n):
                g[i] -= ((_fr(d[i]) if d is not None else 0) + _fr(lam)) * xf[i]
                if Cu is not None:
                    for j in range(n):
                        c = Cu[min(i, j), max(i, j)] if (mirrored or j >= i) else 0.0
                        g[i] -= _fr(c) * xf[j]
        return np.array([float(v) for v in r]), np.array([float(v) for v in g])

    def gradient(x):
        if pair:
            return gradient_pair(x)
        r = (b.astype(np.longdouble) - Jd.astype(np.longdouble) @ x.astype(np.longdouble)).astype(np.float64)
        g = JW @ r
        if base:
            g = (g.astype(np.longdouble) - base_times(Cu, d, lam, x, mirrored)).astype(np.float64)
        return r, g

    x = solve(JW @ b)
    r, g = gradient(x)
    g0 = np.max(np.abs(g)) if n else 0.0
    iters, dlast, dprev = 0, 0.0, np.max(np.abs(x)) if n else 0.0
    if g0 == 0.0:
        state = CONVERGED
    elif max_iter == 0:
        state = MAXITER
    else:
        state = None
    while state is None:
        dx = solve(g)
        dk = np.max(np.abs(dx))
        dlast = dk
        if not dk < dprev:
            state = DIVERGED
            break
        x = x + dx
        iters += 1
        r, g = gradient(x)
        if dk <= U * np.max(np.abs(x)) or np.max(np.abs(g)) == 0.0:
            state = CONVERGED
        elif dk > rho_max * dprev:
            state = STALLED
        elif iters >= max_iter:
            state = MAXITER
        else:
            dprev = dk
    xn = np.max(np.abs(x)) if n else 0.0
    info = dict(iters=iters, state=state, grad_norm=float(np.max(np.abs(g))) if n else 0.0, grad_norm0=float(g0),
                resid_norm=float(np.sqrt(np.sum(w * r * r))), dx_ratio=0.0 if (dlast == 0.0 and xn == 0.0) else dlast / xn)
    return x, info


# --------------------------------------------------------------------------
# least-squares cases: m = 24, n = 8, entries of J rounded to 2^-20
# --------------------------------------------------------------------------
LSQ_M, LSQ_N = 24, 8


def _prescribed(kappa, rng):
    Uo, _ = np.linalg.qr(rng.standard_normal((LSQ_M, LSQ_N)))
    Vo, _ = np.linalg.qr(rng.standard_normal((LSQ_N, LSQ_N)))
    sv = np.logspace(0.0, -np.log10(kappa), LSQ_N)
    return np.round((Uo * sv) @ Vo.T * 2.0 ** 20) / 2.0 ** 20


def lstsq_case(name):
    """dict(J (dense), w, b, C (upper dense or None), d, lam, consistent) of a named case."""
    kind, kexp, seed = LSQ_CASES[name]
    rng = np.random.default_rng(seed)
    J = _prescribed(10.0 ** kexp, rng)
    J[J == 0.0] = 2.0 ** -20  # a dense pattern whatever the rounding did
    w = np.round(rng.uniform(0.5, 2.0, LSQ_M) * 1024) / 1024
    C = d = None
    lam = 0.0
    if kind == "consistent":
        b = J @ rng.integers(-8, 9, LSQ_N).astype(np.float64)  # exact in fp64: 21 + 4 + 5 bits
    else:
        b = rng.standard_normal(LSQ_M)
    if kind == "damped":
        lam = 2.0 ** -10
    if kind == "base":
        C = np.triu(np.diag(np.full(LSQ_N, 0.5)) + np.diag(np.full(LSQ_N - 1, -0.125), 1))
        d = np.round(rng.uniform(0.0, 0.25, LSQ_N) * 1024) / 1024
        lam = 2.0 ** -12
    return dict(J=J, w=w, b=b, C=C, d=d, lam=lam, consistent=kind == "consistent")


LSQ_CASES = {
    "consistent_1e1": ("consistent", 1, 101), "random_1e1": ("random", 1, 102),
    "consistent_1e3": ("consistent", 3, 103), "random_1e3": ("random", 3, 104),
    "consistent_1e5": ("consistent", 5, 105), "random_1e5": ("random", 5, 106),
    "damped_1e3": ("damped", 3, 107), "base_1e3": ("base", 3, 108),
}


def lstsq_reference(case):
    """numpy.linalg.lstsq on (W^1/2 J, W^1/2 b) in fp64; with a base, the augmented system
    [W^1/2 J; R] x = [W^1/2 b; 0], R^T R = C + diag d + lam I (dense Cholesky)."""
    J, w, b = case["J"], case["w"], case["b"]
    A = np.sqrt(w)[:, None] * J
    rhs = np.sqrt(w) * b
    if case["C"] is not None or case["d"] is not None or case["lam"] != 0.0:
        n = J.shape[1]
        Bm = np.zeros((n, n))
        if case["C"] is not None:
            Bm += np.triu(case["C"]) + np.triu(case["C"], 1).T
        Bm += np.diag((case["d"] if case["d"] is not None else np.zeros(n)) + case["lam"])
        A = np.vstack([A, np.linalg.cholesky(Bm).T])
        rhs = np.concatenate([rhs, np.zeros(n)])
    return np.linalg.lstsq(A, rhs, rcond=None)[0]


def lstsq_exact(case):
    C = case["C"]
    Cfull = None if C is None else np.triu(C) + np.triu(C, 1).T
    return exact_lstsq(case["J"], case["w"], case["b"], Cfull, case["d"], case["lam"])


def max_error(x, xe):
    """max_i |x_i - xe_i| with xe exact rationals, evaluated exactly and rounded once."""
    return max(float(abs(_fr(v) - e)) for v, e in zip(x, xe))


def lstsq_cap(case, xe):
    """What the refined solution may miss the exact one by: 8 x the error of numpy's lstsq on
    the same case plus 8 u relative."""
    ref = lstsq_reference(case)
    return 8.0 * max_error(ref, xe) + 8.0 * U * max(float(abs(e)) for e in xe)


# --------------------------------------------------------------------------
# the known answer: grid incidence over identity
# --------------------------------------------------------------------------
def grid_incidence(k):
    """J = [incidence of the k^3 grid graph; I] (edges x vertices over the identity), entries +-1."""
    n = k ** 3
    idx = np.arange(n).reshape(k, k, k)
    rows = []
    for ax in range(3):
        a = np.take(idx, np.arange(k - 1), axis=ax).ravel()
        b = np.take(idx, np.arange(1, k), axis=ax).ravel()
        rows.extend(zip(a.tolist(), b.tolist()))
    m = len(rows) + n
    cols = [[] for _ in range(n)]
    for r, (a, b) in enumerate(rows):
        cols[a].append((r, 1.0))
        cols[b].append((r, -1.0))
    for v in range(n):
        cols[v].append((len(rows) + v, 1.0))
    p = np.zeros(n + 1, dtype=np.int64)
    ii, xx = [], []
    for v in range(n):
        for r, val in sorted(cols[v]):
            ii.append(r), xx.append(val)
        p[v + 1] = len(ii)
    return sc.csc_matrix(m, n, p, np.array(ii, dtype=np.int32), np.array(xx), sc.sym.none), rows


def grid_laplacian_plus_identity(k):
    """The graph Laplacian of the k^3 grid plus I as an upper csc_matrix, built from degrees."""
    n = k ** 3
    _, edges = grid_incidence(k)
    D = {}
    for v in range(n):
        D[(v, v)] = 1.0
    for a, b in edges:
        D[(a, a)] += 1.0
        D[(b, b)] += 1.0
        D[(min(a, b), max(a, b))] = -1.0
    cols = [[] for _ in range(n)]
    for (i, j), v in D.items():
        cols[j].append((i, v))
    p = np.zeros(n + 1, dtype=np.int64)
    ii, xx = [], []
    for j in range(n):
        for i, v in sorted(cols[j]):
            ii.append(i), xx.append(v)
        p[j + 1] = len(ii)
    return sc.csc_matrix(n, n, p, np.array(ii, dtype=np.int32), np.array(xx), sc.sym.upper)
