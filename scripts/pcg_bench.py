#!/usr/bin/env python3
"""Conjugate gradients preconditioned with the factor, next to the panel solve and the product
on the same handle, and against refinement on the same drifted values.

  python scripts/pcg_bench.py [--case 1138_bus lap128] [--reps 5] [--outdir profiles/pcg]
  python scripts/pcg_bench.py --trace lap128        # kernel times, in a run of its own

Cases: lap128 (3D 7-point Laplacian 128^3 in the geometric ND order of bench.py) and
1138_bus (ND).  Every case runs in a child process of its own under `timeout`, one after the
other, and the first failure ends the run (nothing more is started on the device after a
fault or a hang).  Per case one JSON line, 16 device columns, every time the median of --reps
synchronous calls after a warm-up:
  * sc_solve_device_multi and sc_spmv_device_multi;
  * the time per iteration: A' = D A D, D = diag(1 + 0.1 U(-1, 1)), tol = 0, from the
    difference of a run of 3 and a run of 7 steps, and its ratio to solve + product;
  * end to end on that A' and on A with three diagonal entries times 1.5, 3 and 8: iterations
    and time of sc_solve_pcg_device_multi to relres 1e-10, and of sc_solve_refine_device_multi
    (fp64 residuals) with the fewest increments that bring every column's true relative
    residual to 1e-10, if any number up to 64 does.
--trace runs 8 steps of one panel under `rocprofv3 --kernel-trace --stats` and prints, per
vector kernel, calls, average microseconds and GB/s over the bytes the algorithm moves (dot:
two panels per call of a step, one for b.b, r.r and the closing residual; update: four read,
two written; direction: two read -- one at the first step -- and two written; a panel is
128 n bytes)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = {"lap128": 1100, "1138_bus": 300}  # seconds per child
TRACE_STEPS = 8


def note(msg):
    print(f"pcg_bench: {msg}", file=sys.stderr, flush=True)


def setup(case):
    import numpy as np
    import torch

    import sparsecholesky_amd as sc

    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("pcg_bench: no HIP device visible")
    if case == "lap128":
        A, kw = sc.laplacian3d(128), {}
    else:
        A = sc.load_matrix_market_to_csc(os.path.join(ROOT, "tests", "golden", case + ".mtx"))
        kw = dict(ordering=1)
    n = A.size()
    note(f"{case}: analysing n = {n}")
    num = sc.Numeric(sc.Symbolic(A, **kw), device=0)
    note("factoring")
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0
    rng = np.random.default_rng(1)
    d = 1.0 + 0.1 * rng.uniform(-1.0, 1.0, n)
    cols = np.repeat(np.arange(n), np.diff(A.p))
    d_Ad = torch.from_numpy(A.x * d[A.i] * d[cols]).to("cuda:0")
    x3 = A.x.copy()
    for i, f in zip((1, n // 2, n - 2), (1.5, 3.0, 8.0)):
        x3[A.find_index(i, i)] *= f
    d_A3 = torch.from_numpy(x3).to("cuda:0")
    dB = torch.from_numpy(rng.standard_normal(16 * n)).to("cuda:0")
    dX = torch.empty(16 * n, device="cuda:0", dtype=torch.float64)
    return n, num, d_Ax, d_Ad, d_A3, dB, dX


def child(case, reps, out):
    import torch

    def median_ms(fn):
        fn()
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()  # synchronous: returns after the library stream is idle
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t)

    n, num, d_Ax, d_Ad, d_A3, dB, dX = setup(case)
    dY = torch.empty_like(dX)
    ad, b, x, y = d_Ad.data_ptr(), dB.data_ptr(), dX.data_ptr(), dY.data_ptr()
    solve = median_ms(lambda: num.solve_device_multi(b, 16, n, x, n))
    mul = median_ms(lambda: num.spmv_device_multi(ad, x, 16, n, y, n))
    note(f"solve {solve:.3f} ms, product {mul:.4f} ms")
    mem0 = num.memory()
    t3 = median_ms(lambda: num.solve_pcg_device_multi(ad, b, 16, n, x, n, tol=0.0, max_iter=3))
    t7 = median_ms(lambda: num.solve_pcg_device_multi(ad, b, 16, n, x, n, tol=0.0, max_iter=7))
    mem1 = num.memory()
    it_ms = (t7 - t3) / 4.0
    note(f"iteration {it_ms:.3f} ms")
    # end to end, conjugate gradients against refinement on the same values
    def end_to_end(ax):
        info = num.solve_pcg_device_multi(ax, b, 16, n, x, n, tol=1e-10)
        pcg_ms = median_ms(lambda: num.solve_pcg_device_multi(ax, b, 16, n, x, n, tol=1e-10))
        pcg = dict(ms=round(pcg_ms, 3), iters=info["iters"].tolist(), states=info["state"].tolist(),
                   relres_true_max=float(info["relres_true"].max()))

        def refined_relres(m):
            r = num.solve_refined_device_multi(ax, b, 16, n, x, n, max_iter=m, residual="fp64")
            # the true relative residual of what refinement returned: a warm start of zero steps
            t = num.solve_pcg_device_multi(ax, b, 16, n, x, n, max_iter=0, use_x0=True)
            return float(t["relres_true"].max()), r

        lo, hi, seen = 0, 1, {}
        while hi <= 64:
            seen[hi] = refined_relres(hi)
            note(f"refinement, at most {hi} increments: relres {seen[hi][0]:.2e}, "
                 f"states {set(seen[hi][1]['state'].tolist())}")
            if seen[hi][0] <= 1e-10 or not seen[hi][1]["iters"].any():  # reached, or no increment was ever applied
                break
            lo, hi = hi, 2 * hi
        if hi <= 64 and seen[hi][0] <= 1e-10:
            while hi - lo > 1:  # the fewest increments that reach 1e-10
                mid = (lo + hi) // 2
                seen[mid] = refined_relres(mid)
                lo, hi = (lo, mid) if seen[mid][0] <= 1e-10 else (mid, hi)
            ms = median_ms(lambda: num.solve_refined_device_multi(ax, b, 16, n, x, n, max_iter=hi, residual="fp64"))
            ref = dict(ms=round(ms, 3), max_iter=hi, iters=seen[hi][1]["iters"].tolist(),
                       states=seen[hi][1]["state"].tolist(), relres_true_max=seen[hi][0])
        else:
            last = max(seen)
            ref = dict(ms=None, max_iter=last, iters=seen[last][1]["iters"].tolist(),
                       states=seen[last][1]["state"].tolist(), relres_true_max=seen[last][0], note="1e-10 not reached")
        return pcg, ref

    pcg, ref = end_to_end(ad)
    pcg3, ref3 = end_to_end(d_A3.data_ptr())
    rec = dict(bench="pcg", case=case, n=n, reps=reps, solve16_ms=round(solve, 3), product16_ms=round(mul, 4),
               pcg_3_steps_ms=round(t3, 3), pcg_7_steps_ms=round(t7, 3), iteration_ms=round(it_ms, 3),
               iteration_over_solve_plus_product=round(it_ms / (solve + mul), 4), dad10_pcg=pcg, dad10_refine=ref,
               rank3_pcg=pcg3, rank3_refine=ref3,
               memory_before=mem0, memory_after=mem1)
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def trace_child(case):
    n, num, d_Ax, d_Ad, d_A3, dB, dX = setup(case)
    for _ in range(2):
        num.solve_pcg_device_multi(d_Ad.data_ptr(), dB.data_ptr(), 16, n, dX.data_ptr(), n, tol=0.0,
                                   max_iter=TRACE_STEPS)
    print(json.dumps(dict(n=n)), flush=True)


def trace(case, outdir):
    d = os.path.join(outdir, f"trace_{case}")
    log = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), "rocprofv3", "--kernel-trace", "--stats",
                          "-f", "csv", "-d", d, "-o", "pcg", "--", sys.executable, os.path.abspath(__file__),
                          "--trace-child", "--case", case], stdout=subprocess.PIPE, text=True)
    if log.returncode != 0:
        raise SystemExit(f"pcg_bench: the traced run of {case} ended with status {log.returncode}")
    n = json.loads([ln for ln in log.stdout.splitlines() if ln.startswith('{"n"')][-1])["n"]
    f = sorted(glob.glob(f"{d}/**/*kernel_stats.csv", recursive=True))[-1]
    rows = list(csv.DictReader(open(f)))
    panel, K, calls = 128.0 * n, TRACE_STEPS, 2
    moved = {"pcg_dot_panel_kernel": calls * (2 * K * 2 + 3) * panel, "pcg_update_kernel": calls * K * 6 * panel,
             "pcg_dir_kernel": calls * ((K - 1) * 4 + 3) * panel}
    total = {k: 0.0 for k in moved}
    kernels = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:14]:
        kernels.append(dict(name=r["Name"][:90], calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                            total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3)))
    for r in rows:
        for k in total:
            if k in r["Name"]:
                total[k] += float(r["TotalDurationNs"])
    rec = dict(bench="pcg_trace", case=case, n=n, steps=K, calls=calls, top_kernels=kernels,
               vector_gbps={k: round(moved[k] / total[k], 1) for k in moved if total[k] > 0},
               vector_total_ms={k: round(total[k] / 1e6, 3) for k in moved})
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(outdir, f"pcg_trace_{case}.jsonl"), "a") as fo:
        fo.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=["1138_bus", "lap128"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "pcg"))
    ap.add_argument("--trace", default=None, help="a case to run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.reps, os.path.join(a.outdir, f"pcg_{a.case[0]}.jsonl"))
        return
    if a.trace_child:
        trace_child(a.case[0])
        return
    if a.trace:
        os.makedirs(a.outdir, exist_ok=True)
        trace(a.trace, a.outdir)
        return
    for case in a.case:  # one child per case, each under its own limit; the first failure ends the run
        rc = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), sys.executable, os.path.abspath(__file__),
                             "--child", "--case", case, "--reps", str(a.reps), "--outdir", a.outdir]).returncode
        if rc != 0:
            raise SystemExit(f"pcg_bench: {case} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
