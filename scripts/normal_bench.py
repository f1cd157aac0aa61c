#!/usr/bin/env python3
"""Forming the weighted normal equations next to the operations they stand beside, one handle per case.

  python scripts/normal_bench.py [--case bus1138 grid128] [--reps 7] [--outdir profiles/normal]

Cases:
  grid128  J = [incidence of the 128^3 grid graph; I] with the vertices in the geometric ND order
           of bench.py (the edges are read off laplacian3d(128)'s off-diagonal entries), so S = J^T
           W J has that Laplacian's pattern: m ~ 4 n, T ~ 3 m terms, all lists short;
  bus1138  a random J with n = 1138, m = 4 n rows of 4 entries each over an identity block, damped:
           the launch-bound end.
Every case runs in a child process of its own under `timeout`, one after the other, and the first
failure ends the run (nothing more is started on the device after a fault or a hang).  Per case one
JSON line; device arrays; every time is the median of --reps synchronous calls after a warm-up,
clocks as found:
  * the form (sc_normal_values_device), with the bytes of the term lists plus the values written
    (12 T + 8 (ne + 1) + 8 ne) and GB/s over them;
  * Y = J X and G = J^T W Y on 16 columns, beside the compensated residual pass over S on 16
    columns (sc_residual_device_multi; its bytes counted as 20 per entry of the mirrored S plus
    three 128-byte panel rows per row) and sc_pattern_outer_device on 16 columns;
  * the factorization alone (sc_factor_device on the formed values) and sc_normal_factor_device;
  * one sc_normal_lstsq_device_multi of 16 columns held to two increments."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = {"grid128": 1100, "bus1138": 300}  # seconds per child


def note(msg):
    print(f"normal_bench: {msg}", file=sys.stderr, flush=True)


def csc_from_triplets(sc, np, m, n, rows, cols, vals):
    order = np.lexsort((rows, cols))
    rows, cols, vals = rows[order], cols[order], vals[order]
    p = np.zeros(n + 1, dtype=np.int64)
    np.add.at(p, cols + 1, 1)
    return sc.csc_matrix(m, n, np.cumsum(p), rows.astype(np.int32), vals.astype(np.float64), sc.sym.none)


def build_case(sc, np, case):
    """(J, damping, Symbolic keywords)."""
    if case.startswith("grid"):
        k = int(case[4:])
        A = sc.laplacian3d(k)
        n = A.size()
        col = np.repeat(np.arange(n, dtype=np.int64), np.diff(A.p))
        row = A.i.astype(np.int64)
        off = row < col
        a, b = row[off], col[off]
        ne = len(a)
        e = np.arange(ne, dtype=np.int64)
        rows = np.concatenate([e, e, ne + np.arange(n, dtype=np.int64)])
        cols = np.concatenate([a, b, np.arange(n, dtype=np.int64)])
        vals = np.concatenate([np.ones(ne), -np.ones(ne), np.ones(n)])
        return csc_from_triplets(sc, np, ne + n, n, rows, cols, vals), 0.0, {}
    n = 1138
    rng = np.random.default_rng(1138)
    m0 = 4 * n
    cols = np.concatenate([rng.choice(n, 4, replace=False) for _ in range(m0)] + [np.arange(n)]).astype(np.int64)
    rows = np.concatenate([np.repeat(np.arange(m0, dtype=np.int64), 4), m0 + np.arange(n, dtype=np.int64)])
    vals = np.concatenate([rng.standard_normal(4 * m0), np.ones(n)])
    return csc_from_triplets(sc, np, m0 + n, n, rows, cols, vals), 1e-3, dict(ordering=1)


def child(case, reps, out):
    import numpy as np
    import torch

    import sparsecholesky_amd as sc

    L = sc.lib()
    if L.sc_device_count() <= 0:
        raise SystemExit("normal_bench: no HIP device visible")
    J, damping, kw = build_case(sc, np, case)
    m, n = J.n_rows, J.n_cols
    note(f"{case}: J is {m} x {n} with {len(J.x)} entries; building the structure")
    t0 = time.perf_counter()
    ne_ = sc.NormalEquations(J, device=0)
    t_struct = time.perf_counter() - t0
    A = ne_.matrix()
    T, nv = ne_.terms, ne_.nvalues
    note(f"T = {T} terms, {nv} entries of S, structure {t_struct:.2f} s; analysing")
    symb = sc.Symbolic(A, **kw)
    num = sc.Numeric(symb, device=0)
    rng = np.random.default_rng(2)
    dev = "cuda:0"
    dJ = torch.from_numpy(J.x).to(dev)
    dw = torch.from_numpy(rng.uniform(0.5, 2.0, m)).to(dev)
    dS = torch.empty(max(nv, 1), device=dev, dtype=torch.float64)
    vp = C.c_void_p

    def median_ms(fn):
        fn()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # synchronous: returns after the library's stream is idle
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    def ok(rc):
        assert rc == 0, (rc, L.sc_last_error())

    form = median_ms(lambda: ok(L.sc_normal_values_device(ne_.h, vp(dJ.data_ptr()), vp(dw.data_ptr()), None, None,
                                                          damping, vp(dS.data_ptr()))))
    fbytes = 12 * T + 8 * (nv + 1) + 8 * nv
    note(f"form {form:.4f} ms, {fbytes / form / 1e6:.1f} GB/s over {fbytes} bytes")
    nfac = median_ms(lambda: ok(L.sc_normal_factor_device(ne_.h, num.h, vp(dJ.data_ptr()), vp(dw.data_ptr()), None, None,
                                                          damping)))
    sx = ne_.values_ptr
    fac = median_ms(lambda: ok(num.factor_device(sx, sync=True)))
    note(f"factorization {fac:.3f} ms, form + factorization {nfac:.3f} ms")
    # the least-squares solve accepts only the factor of the handle's own last factor call: the
    # plain factorizations just timed have replaced it
    ok(L.sc_normal_factor_device(ne_.h, num.h, vp(dJ.data_ptr()), vp(dw.data_ptr()), None, None, damping))
    dXn = torch.from_numpy(rng.standard_normal(16 * n)).to(dev)
    dYm = torch.from_numpy(rng.standard_normal(16 * m)).to(dev)
    dOm = torch.empty(16 * m, device=dev, dtype=torch.float64)
    dOn, dRn, dGv = (torch.empty(16 * n, device=dev, dtype=torch.float64) for _ in range(3))
    mul = median_ms(lambda: ok(L.sc_normal_mul_device_multi(ne_.h, 16, vp(dJ.data_ptr()), vp(dXn.data_ptr()), n,
                                                            vp(dOm.data_ptr()), m)))
    mult = median_ms(lambda: ok(L.sc_normal_mult_device_multi(ne_.h, 16, vp(dJ.data_ptr()), vp(dw.data_ptr()),
                                                              vp(dYm.data_ptr()), m, vp(dOn.data_ptr()), n)))
    res = median_ms(lambda: num.residual_device_multi(sx, dOn.data_ptr(), 16, n, dXn.data_ptr(), n, dRn.data_ptr(), n))
    dG = torch.empty(max(nv, 1), device=dev, dtype=torch.float64)
    outer = median_ms(lambda: num.pattern_outer_device(dXn.data_ptr(), dOn.data_ptr(), 16, n, n, dG.data_ptr()))
    note(f"J X {mul:.4f} ms, J^T W Y {mult:.4f} ms; compensated residual over S {res:.4f} ms, outer product {outer:.4f} ms")
    info = (sc.LstsqInfo * 16)()
    o = sc.Numeric._refine_options(2, "dd", 0.5)
    lsq = median_ms(lambda: ok(L.sc_normal_lstsq_device_multi(ne_.h, num.h, C.byref(o), 16, vp(dJ.data_ptr()),
                                                              vp(dw.data_ptr()), vp(dYm.data_ptr()), m,
                                                              vp(dGv.data_ptr()), n, info)))
    iters = [info[c].iters for c in range(16)]
    solve = median_ms(lambda: num.solve_device_multi(dOn.data_ptr(), 16, n, dRn.data_ptr(), n))
    note(f"lstsq {lsq:.3f} ms with {min(iters)}..{max(iters)} increments; one panel solve {solve:.3f} ms")
    rec = dict(bench="normal", case=case, m=m, n=n, nnz_J=len(J.x), terms=T, entries_S=nv, reps=reps,
               structure_s=round(t_struct, 3), form_ms=round(form, 4), form_bytes=fbytes,
               form_gbps=round(fbytes / form / 1e6, 1), factor_ms=round(fac, 3), normal_factor_ms=round(nfac, 3),
               form_over_factor=round(form / fac, 4), mul16_ms=round(mul, 4), mult16_ms=round(mult, 4),
               residual_dd16_ms=round(res, 4), pattern_outer16_ms=round(outer, 4),
               mul_over_residual=round(mul / res, 3), mult_over_residual=round(mult / res, 3),
               residual_bytes=20 * (2 * nv - n) + 3 * 128 * n, residual_gbps=round((20 * (2 * nv - n) + 384 * n) / res / 1e6, 1),
               lstsq16_ms=round(lsq, 3), lstsq_iters=[min(iters), max(iters)], solve16_ms=round(solve, 3),
               memory=ne_.memory())
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=["bus1138", "grid128"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "normal"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.reps, os.path.join(a.outdir, f"normal_{a.case[0]}.jsonl"))
        return
    for case in a.case:  # one child per case, each under its own limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), sys.executable, os.path.abspath(__file__),
                             "--child", "--case", case, "--reps", str(a.reps), "--outdir", a.outdir]).returncode
        if rc != 0:
            raise SystemExit(f"normal_bench: {case} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
