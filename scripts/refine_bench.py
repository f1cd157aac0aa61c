#!/usr/bin/env python3
"""Residual pass and refined solve next to the panel solve, on one handle.

  python scripts/refine_bench.py [--case lap128 1138_bus] [--reps 5] [--outdir profiles/refine]

Cases: lap128 (3D 7-point Laplacian 128^3 in the geometric ND order of bench.py) and
1138_bus (ND).  Every case runs in a child process of its own under `timeout`, one after the
other, and the first failure ends the run (nothing more is started on the device after a
fault or a hang).  Per case one JSON line:
  * the residual pass of a 16-column device panel in both modes: ms, algorithmic bytes
    (structure 12 B per entry + 8 B row pointers + 16 B per task, the values, and the X, B and
    R panels once each) and GB/s, and the product pass;
  * sc_solve_device_multi and sc_solve_refine_device_multi (both residual modes) of the same
    16 columns: ms, increments per column, and the ratio to (1 + increments) panel solves;
  * the error measures before (max_iter = 0) and after refinement.
Each time is the median of --reps synchronous calls after a warm-up."""
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


def child(case, reps, out):
    import numpy as np
    import torch

    import sparsecholesky_amd as sc

    def median_ms(fn):
        fn()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # synchronous: returns after the library stream is idle
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("refine_bench: no HIP device visible")
    if case == "lap128":
        A, kw = sc.laplacian3d(128), {}
    else:
        A = sc.load_matrix_market_to_csc(os.path.join(ROOT, "tests", "golden", case + ".mtx"))
        kw = dict(ordering=1)
    n = A.size()
    symb = sc.Symbolic(A, **kw)
    num = sc.Numeric(symb, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0
    rp, ci, _ = symb.spmv_structure()
    nz = len(ci)
    ntask = int(np.maximum(-(-np.diff(rp) // 256), 1).sum())
    del ci
    rng = np.random.default_rng(1)
    dB = torch.from_numpy(rng.standard_normal(16 * n)).to("cuda:0")
    dX = torch.empty(16 * n, device="cuda:0", dtype=torch.float64)
    dR = torch.empty(16 * n, device="cuda:0", dtype=torch.float64)
    ax, b, x, r = d_Ax.data_ptr(), dB.data_ptr(), dX.data_ptr(), dR.data_ptr()
    solve = median_ms(lambda: num.solve_device_multi(b, 16, n, x, n))
    mem0 = num.memory()
    passes = {}
    bytes_pass = 12 * nz + 8 * (n + 1) + 16 * ntask + 8 * len(A.x) + 3 * 16 * 8 * n
    for mode in ("fp64", "dd"):
        ms = median_ms(lambda: num.residual_device_multi(ax, b, 16, n, x, n, r, n, mode=mode))
        passes[mode] = dict(ms=round(ms, 4), bytes=bytes_pass, gbps=round(bytes_pass / (ms * 1e-3) / 1e9, 1),
                            frac_of_panel_solve=round(ms / solve, 4))
    mul = median_ms(lambda: num.spmv_device_multi(ax, x, 16, n, r, n))
    mem1 = num.memory()
    before = num.solve_refined_device_multi(ax, b, 16, n, x, n, max_iter=0)
    refined = {}
    for mode in ("fp64", "dd"):
        info = num.solve_refined_device_multi(ax, b, 16, n, x, n, residual=mode)
        ms = median_ms(lambda: num.solve_refined_device_multi(ax, b, 16, n, x, n, residual=mode))
        it = int(info["iters"].max())
        # a panel runs until its last column stops: 1 + max increments solves, and as many passes + 1
        refined[mode] = dict(ms=round(ms, 3), iters=info["iters"].tolist(), states=info["state"].tolist(),
                             ratio_to_panel_solves=round(ms / ((1 + it) * solve), 4),
                             berr_comp_max=float(info["berr_comp"].max()), berr_norm_max=float(info["berr_norm"].max()),
                             dx_ratio_max=float(info["dx_ratio"].max()))
    rec = dict(bench="refine", case=case, n=n, nnz_full=nz, tasks=ntask, reps=reps, solve16_ms=round(solve, 3),
               residual16=passes, product16_ms=round(mul, 4),
               plain_solve=dict(berr_comp_max=float(before["berr_comp"].max()),
                                berr_norm_max=float(before["berr_norm"].max())),
               refined16=refined, memory_before=mem0, memory_after=mem1,
               hot_kernel="spmv_sym_panel_kernel<SPMV_RES_DD>")
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
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "refine"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.reps, os.path.join(a.outdir, f"refine_{a.case[0]}.jsonl"))
        return
    for case in a.case:  # one child per case, each under its own limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), sys.executable, os.path.abspath(__file__),
                             "--child", "--case", case, "--reps", str(a.reps), "--outdir", a.outdir]).returncode
        if rc != 0:
            raise SystemExit(f"refine_bench: {case} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
