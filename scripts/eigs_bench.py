#!/usr/bin/env python3
"""Smallest eigenpairs by block shift-invert Lanczos, next to the panel solve on the same handle.

  python scripts/eigs_bench.py [--case 1138_bus lap128] [--reps 5] [--outdir profiles/eigs]
  python scripts/eigs_bench.py --trace lap128        # kernel times, in a run of its own

Cases: lap128 (3D 7-point Laplacian 128^3 in the geometric ND order of bench.py) and 1138_bus
(ND).  Every case runs in a child process of its own under `timeout`, one after the other, and
the first failure ends the run (nothing more is started on the device after a fault or a
hang).  Per case one JSON line; nev = 8, tol = 1e-10, the library's start block, device arrays;
every time the median of --reps synchronous calls after a warm-up:
  * sc_solve_device_multi with 16 columns, and sc_eigs_device: blocks, states, ms, and
    (ms - blocks x panel solve) / blocks, what a step costs beyond its solve;
  * lap128: the eight eigenvalues against the closed form of the Dirichlet grid Laplacian with
    stencil 6 / -1 (refapi.cpp), lambda = 6 - 2 (cos(i h) + cos(j h) + cos(l h)), h = pi / (k + 1),
    after that formula was checked against eigh at 8^3 on the host.
--trace runs two calls under `rocprofv3 --kernel-trace --stats` and prints the split of the
kernel time into panel solve, Gram, block update, the residual's product and sum, and GB/s of
the Gram and update kernels and of pcg_dot over the bytes the algorithm moves (a panel is 128 n
bytes; a Gram launch over nb blocks reads nb + 1 panels, an update over nb blocks reads nb (+ 1
with beta != 0) and writes one, the sum pass reads two panels of nev columns)."""
import argparse
import csv
import glob
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = {"lap128": 1100, "1138_bus": 300}  # seconds per child
NEV, TOL = 8, 1e-10


def note(msg):
    print(f"eigs_bench: {msg}", file=sys.stderr, flush=True)


def grid_spectrum(k, count):
    """The `count` smallest eigenvalues of the k^3 Dirichlet Laplacian with stencil 6 / -1."""
    import numpy as np

    c = 2.0 * np.cos(np.arange(1, k + 1) * math.pi / (k + 1))
    # the smallest sums use the largest cosines: indices below 8 suffice for count <= 64
    m = min(k, 8)
    lam = (6.0 - (c[:m, None, None] + c[None, :m, None] + c[None, None, :m])).reshape(-1)
    return np.sort(lam)[:count]


def check_formula():
    import numpy as np
    import scipy.linalg as sla

    import sparsecholesky_amd as sc

    A = sc.laplacian3d(8, nd=False)
    D = np.zeros((512, 512))
    for j in range(512):
        for q in range(A.p[j], A.p[j + 1]):
            D[A.i[q], j] = D[j, A.i[q]] = A.x[q]
    mu = sla.eigh(D, eigvals_only=True)[:NEV]
    err = float(np.max(np.abs(mu - grid_spectrum(8, NEV)) / mu))
    if err > 1e-13:
        raise SystemExit(f"eigs_bench: the closed form misses eigh at 8^3 by {err:.1e} relative")
    return err


def setup(case):
    import torch

    import sparsecholesky_amd as sc

    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("eigs_bench: no HIP device visible")
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
    return n, num, d_Ax


def child(case, reps, out):
    import numpy as np
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

    formula_err = check_formula() if case == "lap128" else None
    n, num, d_Ax = setup(case)
    dB = torch.from_numpy(np.random.default_rng(1).standard_normal(16 * n)).to("cuda:0")
    dX = torch.empty_like(dB)
    solve = median_ms(lambda: num.solve_device_multi(dB.data_ptr(), 16, n, dX.data_ptr(), n))
    note(f"panel solve {solve:.3f} ms")
    mem0 = num.memory()
    res = {}

    def run():
        res["lam"], res["X"], res["info"] = num.eigsh_device(NEV, tol=TOL, values=d_Ax, return_info=True)

    ms = median_ms(run)
    mem1 = num.memory()
    info, lam = res["info"], res["lam"]
    blocks = int(info["blocks"][0])
    rec = dict(bench="eigs", case=case, n=n, nev=NEV, tol=TOL, reps=reps, solve16_ms=round(solve, 3),
               eigs_ms=round(ms, 3), blocks=blocks, states=info["state"].tolist(),
               step_beyond_solve_ms=round((ms - blocks * solve) / blocks, 3),
               call_over_solves=round(ms / (blocks * solve), 4), lam=lam.tolist(), est_max=float(info["est"].max()),
               resid_max=float(info["resid"].max()), memory_before=mem0, memory_after=mem1)
    if case == "lap128":
        ref = grid_spectrum(128, NEV)
        rec["closed_form_rel_err_max"] = float(np.max(np.abs(lam - ref) / ref))
        rec["closed_form_vs_eigh_at_8"] = formula_err
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def trace_child(case):
    n, num, d_Ax = setup(case)
    for _ in range(2):
        lam, X, info = num.eigsh_device(NEV, tol=TOL, values=d_Ax, return_info=True)
    print(json.dumps(dict(n=n, blocks=int(info["blocks"][0]))), flush=True)


def trace(case, outdir):
    d = os.path.join(outdir, f"trace_{case}")
    log = subprocess.run(["timeout", "-k", "10", str(LIMIT.get(case, 900)), "rocprofv3", "--kernel-trace", "--stats",
                          "-f", "csv", "-d", d, "-o", "eigs", "--", sys.executable, os.path.abspath(__file__),
                          "--trace-child", "--case", case], stdout=subprocess.PIPE, text=True)
    if log.returncode != 0:
        raise SystemExit(f"eigs_bench: the traced run of {case} ended with status {log.returncode}")
    head = json.loads([ln for ln in log.stdout.splitlines() if ln.startswith('{"n"')][-1])
    n, J, calls = head["n"], head["blocks"], 2
    f = sorted(glob.glob(f"{d}/**/*kernel_stats.csv", recursive=True))[-1]
    rows = list(csv.DictReader(open(f)))
    panel, part = 128.0 * n, NEV / 16.0
    orths = 4 * J  # CholQR passes: two per orth, two launches of each kernel per pass, J orths (start + J - 1)
    gram_panels = 2 * orths + sum(2 * (j + 2) + 2 for j in range(J))
    upd_panels = 2 * orths + sum(2 * (j + 3) for j in range(J)) + (J + part) + 3 * part
    moved = {"eigs_gram_kernel": calls * gram_panels * panel, "eigs_update_kernel": calls * upd_panels * panel,
             "pcg_dot_panel_kernel": calls * 2 * part * panel}
    groups = {"gram": ("eigs_gram_kernel", "eigs_gram_final_kernel"), "update": ("eigs_update_kernel",),
              "residual": ("spmv", "pcg_dot", "pcg_final"), "start": ("eigs_start_kernel",)}
    total = {k: 0.0 for k in moved}
    split = {k: 0.0 for k in groups}
    split["solve"] = 0.0
    kernels = []
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"]))[:14]:
        kernels.append(dict(name=r["Name"][:90], calls=int(r["Calls"]), avg_us=round(float(r["AverageNs"]) / 1e3, 2),
                            total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3)))
    for r in rows:
        ns = float(r["TotalDurationNs"])
        for k in total:
            if k in r["Name"]:
                total[k] += ns
        if "solve" in r["Name"] or "gemv" in r["Name"] or "diag" in r["Name"]:
            g = "solve"
        else:
            g = next((g for g, names in groups.items() if any(s in r["Name"] for s in names)), None)
        if g:
            split[g] += ns
    rec = dict(bench="eigs_trace", case=case, n=n, blocks=J, calls=calls, top_kernels=kernels,
               split_ms_per_call={k: round(v / 1e6 / calls, 3) for k, v in split.items()},
               gbps={k: round(moved[k] / total[k], 1) for k in moved if total[k] > 0},
               total_ms={k: round(total[k] / 1e6, 3) for k in moved})
    line = json.dumps(rec)
    print(line, flush=True)
    with open(os.path.join(outdir, f"eigs_trace_{case}.jsonl"), "a") as fo:
        fo.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", nargs="+", default=["1138_bus", "lap128"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "eigs"))
    ap.add_argument("--trace", default=None, help="a case to run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.case[0], a.reps, os.path.join(a.outdir, f"eigs_{a.case[0]}.jsonl"))
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
            raise SystemExit(f"eigs_bench: {case} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
