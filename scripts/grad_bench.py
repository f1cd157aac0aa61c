#!/usr/bin/env python3
"""Gradients on A's pattern next to the operations they stand beside, on one handle per case.

  python scripts/grad_bench.py [--case 1138_bus lap128] [--reps 5] [--outdir profiles/grad]

Cases: lap128 (3D 7-point Laplacian 128^3 in the geometric ND order of bench.py) and 1138_bus
(ND).  Every case runs in a child process of its own under `timeout`, one after the other, and
the first failure ends the run (nothing more is started on the device after a fault or a
hang).  Per case one JSON line, device arrays, every time the median of --reps synchronous calls
after a warm-up:
  * the Z gather: sc_logdet_grad_device with the Z panel current, with the bytes the algorithm
    moves (per effective entry a_pos 4 + a_src 8 + Z 8 + G 8, per column a_ptr 8) and GB/s;
  * sc_pattern_outer_device of 16 columns (two transposes and one pass over the entry list)
    beside sc_spmv_device_multi of 16 columns;
  * sc_selinv, and sc_logdet_grad_device after a new factorization (Z stale: it runs the
    selected inversion itself), so what the gradient costs beyond its sc_selinv;
  * sc_solve_grad_device of 16 columns beside one sc_solve_device_multi of 16 columns."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = {"lap128": 900, "1138_bus": 300}  # seconds per child


def note(msg):
    print(f"grad_bench: {msg}", file=sys.stderr, flush=True)


def child(case, reps, out):
    import numpy as np
    import torch

    import sparsecholesky_amd as sc

    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("grad_bench: no HIP device visible")
    if case == "lap128":
        A, kw = sc.laplacian3d(128), {}
    else:
        A = sc.load_matrix_market_to_csc(os.path.join(ROOT, "tests", "golden", case + ".mtx"))
        kw = dict(ordering=1)
    n, nnz = A.size(), len(A.x)
    note(f"{case}: analysing n = {n}")
    symb = sc.Symbolic(A, **kw)
    ne = int(symb.value_entries()[2].sum())
    num = sc.Numeric(symb, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    ax = d_Ax.data_ptr()
    note("factoring")
    assert num.factor_device(ax, sync=True) == 0

    def median_ms(fn, before=None):
        (before or (lambda: None))()
        fn()
        t = []
        for _ in range(reps):
            if before:
                before()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # synchronous: returns after the library stream is idle
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    rng = np.random.default_rng(1)
    dB = torch.from_numpy(rng.standard_normal(16 * n)).to("cuda:0")
    dX, dY, dW = (torch.empty(16 * n, device="cuda:0", dtype=torch.float64) for _ in range(3))
    dG = torch.empty(max(nnz, 1), device="cuda:0", dtype=torch.float64)
    b, x, y, w, g = (t.data_ptr() for t in (dB, dX, dY, dW, dG))
    solve = median_ms(lambda: num.solve_device_multi(b, 16, n, x, n))
    mul = median_ms(lambda: num.spmv_device_multi(ax, x, 16, n, y, n))
    outer = median_ms(lambda: num.pattern_outer_device(b, x, 16, n, n, g))
    note(f"solve {solve:.3f} ms, product {mul:.4f} ms, outer product {outer:.4f} ms")
    sgrad = median_ms(lambda: num.solve_grad_device(b, x, 16, n, n, w, n, g))
    note(f"solve_grad {sgrad:.3f} ms")
    selinv = median_ms(lambda: num.selinv())
    gather = median_ms(lambda: num.logdet_grad_device(g))
    trace = num.pattern_dot_device(g, ax)
    gbytes = 28 * ne + 8 * n
    note(f"selinv {selinv:.3f} ms, gather {gather:.4f} ms, sum a_k g_k - n = {trace - n:.3e}")
    stale = median_ms(lambda: num.logdet_grad_device(g), before=lambda: num.factor_device(ax, sync=True))
    dot = median_ms(lambda: num.pattern_dot_device(g, ax))
    rec = dict(bench="grad", case=case, n=n, values=nnz, effective_entries=ne, reps=reps,
               gather_ms=round(gather, 4), gather_bytes=gbytes, gather_gbps=round(gbytes / gather / 1e6, 1),
               outer16_ms=round(outer, 4), product16_ms=round(mul, 4), outer_over_product=round(outer / mul, 3),
               selinv_ms=round(selinv, 3), logdet_grad_stale_ms=round(stale, 3),
               logdet_grad_beyond_selinv_ms=round(stale - selinv, 3),
               solve_grad16_ms=round(sgrad, 3), solve16_ms=round(solve, 3),
               solve_grad_beyond_solve_ms=round(sgrad - solve, 3), dot_ms=round(dot, 4),
               homogeneity_residual=trace - n, memory=num.memory())
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=["1138_bus", "lap128"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "grad"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.reps, os.path.join(a.outdir, f"grad_{a.case[0]}.jsonl"))
        return
    for case in a.case:  # one child per case, each under its own limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), sys.executable, os.path.abspath(__file__),
                             "--child", "--case", case, "--reps", str(a.reps), "--outdir", a.outdir]).returncode
        if rc != 0:
            raise SystemExit(f"grad_bench: {case} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
