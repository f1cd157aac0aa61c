#!/usr/bin/env python3
"""Rank-k update / downdate (sc_updown_host) on lap k^3 (ND order), one handle per size, next
to the factorization of the same handle in the same run.

  python scripts/updown_bench.py [--k 128] [--reps 5] [--out FILE]

Cases: W = 1 and 16 unit vectors at seeded random grid points (the observation of a GMRF at
k points), and 16 unit vectors whose rows are columns of the root separator (the shortest
path: the root supernode alone).  Per case one JSON line: the median wall time of --reps
synchronous updates and of --reps downdates of the same W, alternating (so the matrix
returns to A), after a warm-up pair; the path of the sweep from sc_updown_check (touched
supernodes, 64-column block steps, panel entries m w); the kernel launches of one sweep
counted from the supernode partition (1 scatter, 1 block kernel per block step, 1 row
kernel per block step with front rows below it); the algorithmic bytes 16 x panel entries
(every touched panel read once and written once) and the GB/s they give; the factorization
time.  Validation at scale: after the first update, the backward error of a solve against
A + W W^T formed on the host."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import sparsecholesky_amd as sc  # noqa: E402


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # synchronous: returns after the library stream is idle
    return (time.perf_counter() - t0) * 1e3


def unit_vectors(rows):
    k = len(rows)
    return np.arange(k + 1, dtype=np.int64), np.asarray(rows, dtype=np.int32), np.ones(k)


def count_launches(symb, first):
    sn = symb.supernodes()
    _, post = symb.etree()
    ipost = np.empty(symb.n, dtype=np.int64)
    ipost[post] = np.arange(symb.n)
    on = set()
    for j0 in first:
        s = int(np.searchsorted(sn["start"], ipost[j0], side="right") - 1)
        while s >= 0 and s not in on:
            on.add(s)
            s = int(sn["parent"][s])
    launches = 1
    for s in on:
        w, m = int(sn["w"][s]), int(sn["m"][s])
        for k0 in range(0, w, 64):
            launches += 2 if m > min(w, k0 + 64) else 1
    return launches


def run(k, reps, out):
    import scipy.sparse as sp

    A = sc.laplacian3d(k)
    symb = sc.Symbolic(A)
    n = A.size()
    num = sc.Numeric(symb, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0  # warm-up (code objects)
    t_factor = [wall_ms(lambda: num.factor_device(d_Ax.data_ptr(), sync=True)) for _ in range(3)]
    sn = symb.supernodes()
    _, post = symb.etree()
    root = int(np.flatnonzero(sn["parent"] < 0)[-1])
    rng = np.random.default_rng(k)
    pts = rng.choice(n, 16, replace=False)
    rootcols = post[int(sn["start"][root]) + rng.choice(int(sn["w"][root]), 16, replace=False)]
    cases = [("random_points_k1", pts[:1]), ("random_points_k16", pts), ("root_separator_k16", rootcols)]
    U = sp.csc_matrix((A.x, A.i, A.p), shape=(n, n))
    Afull = (U + sp.triu(U, 1).T).tocsr()
    b = np.random.default_rng(1).standard_normal(n)
    mem0 = num.memory()
    for name, rows in cases:
        W = unit_vectors(rows)
        first, path = symb.updown_check(W)
        t_first = wall_ms(lambda: num.update(W))  # the very first call also allocates the workspace
        x = num.solve(b)
        r = Afull @ x + np.bincount(rows, weights=x[rows], minlength=n) - b
        berr = float(np.abs(r).max() / (abs(Afull).sum(axis=1).max() * np.abs(x).max() + np.abs(b).max()))
        assert num.downdate(W) == 0
        up, dn = [], []
        for _ in range(reps):
            up.append(wall_ms(lambda: num.update(W)))
            dn.append(wall_ms(lambda: num.downdate(W)))
        assert num.status() == 0
        ms_up, ms_dn = statistics.median(up), statistics.median(dn)
        nbytes = 16 * path["panel_entries"]
        rec = dict(bench="updown", case=name, k=k, n=n, columns=len(rows), reps=reps,
                   factor_ms=round(statistics.median(t_factor), 3), first_call_ms=round(t_first, 3),
                   update_ms=round(ms_up, 3), update_min_ms=round(min(up), 3), update_max_ms=round(max(up), 3),
                   downdate_ms=round(ms_dn, 3), downdate_min_ms=round(min(dn), 3), downdate_max_ms=round(max(dn), 3),
                   path=path, launches=count_launches(symb, first), algorithmic_bytes=nbytes,
                   update_gbps=round(nbytes / (ms_up * 1e-3) / 1e9, 2), downdate_gbps=round(nbytes / (ms_dn * 1e-3) / 1e9, 2),
                   factor_over_update=round(statistics.median(t_factor) / ms_up, 2),
                   hot_kernel="updown_rows_kernel (v_mfma_f64_16x16x4_f64)",
                   solve_backward_error_after_update=berr)
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
            with open(out, "a") as f:
                f.write(line + "\n")
    mem1 = num.memory()
    print(json.dumps(dict(bench="updown_memory", k=k, before=mem0, after=mem1)), flush=True)
    # the factor after the update / downdate pairs is still the factor of A to rounding
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("updown_bench: no HIP device visible")
    for k in a.k:
        run(k, a.reps, a.out)


if __name__ == "__main__":
    main()
