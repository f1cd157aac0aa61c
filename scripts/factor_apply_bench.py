#!/usr/bin/env python3
"""The factor operators (sc_apply_device / sc_apply_device_multi, sc_logdet) on lap k^3 (ND
order), one handle, next to the full solve of the same run.

  python scripts/factor_apply_bench.py [--k 128] [--reps 11] [--out FILE]

Prints one JSON line: per op (solve_A, solve_L, solve_Lt, mul_L, mul_Lt, P, Pt) the time
of the single-vector entry point and of the 16-column panel entry point, the logdet, and
the ratios the design compares: the two half solves against the full solve, and each
product against the half solve of its direction (same L bytes read, fewer flops, no
inverse on its path).  A single-vector product runs the panel kernels on one column.
Every figure is the median of --reps synchronous calls on device arrays after a warm-up
of the same shape (the calls end in a stream synchronise, so the host clock around them
is the device time plus the launch of one graph)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sparsecholesky_amd as sc  # noqa: E402

OPS = [("solve_A", sc.SC_OP_SOLVE_A), ("solve_L", sc.SC_OP_SOLVE_L), ("solve_Lt", sc.SC_OP_SOLVE_LT),
       ("mul_L", sc.SC_OP_MUL_L), ("mul_Lt", sc.SC_OP_MUL_LT), ("P", sc.SC_OP_PERM), ("Pt", sc.SC_OP_PERM_T)]
NRHS = 16


def timed(fn, reps):
    fn()  # warm-up: first launch of the shape (graph capture, code objects)
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: returns after the library stream is idle
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("factor_apply_bench: no HIP device visible")
    A = sc.laplacian3d(a.k)
    s = sc.Symbolic(A)
    n = A.size()
    num = sc.Numeric(s, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0
    entries = s.stats()["panel_entries"]
    g = torch.Generator(device="cuda:0").manual_seed(1)
    d_B = torch.randn((NRHS, n), dtype=torch.float64, device="cuda:0", generator=g)  # column j = row j
    d_X = torch.empty_like(d_B)
    res = dict(bench="factor_apply", k=a.k, n=n, panel_entries=entries, L_bytes=8 * entries, reps=a.reps, nrhs=NRHS,
               single={}, panel={})
    # the existing entry points of the same run, the yardstick of both families
    res["single"]["sc_solve_device"] = timed(lambda: num.solve_device(d_B.data_ptr(), d_X.data_ptr()), a.reps)
    res["panel"]["sc_solve_device_multi"] = timed(
        lambda: num.solve_device_multi(d_B.data_ptr(), NRHS, n, d_X.data_ptr(), n), a.reps)
    for name, op in OPS:
        res["single"][name] = timed(lambda: num.apply_device(op, d_B.data_ptr(), d_X.data_ptr()), a.reps)
        res["panel"][name] = timed(lambda: num.apply_device_multi(op, d_B.data_ptr(), NRHS, n, d_X.data_ptr(), n),
                                   a.reps)
    t = timed(num.logdet, a.reps)
    res["logdet"] = dict(t, value=num.logdet())
    for fam in ("single", "panel"):
        r = res[fam]
        full = r["sc_solve_device" if fam == "single" else "sc_solve_device_multi"]["ms"]
        r["ratios"] = dict(
            halves_over_full=round((r["solve_L"]["ms"] + r["solve_Lt"]["ms"]) / full, 3),
            mul_L_over_solve_L=round(r["mul_L"]["ms"] / r["solve_L"]["ms"], 3),
            mul_Lt_over_solve_Lt=round(r["mul_Lt"]["ms"] / r["solve_Lt"]["ms"], 3))
        for name in ("solve_L", "solve_Lt", "mul_L", "mul_Lt"):  # one read of L per op and panel
            r[name]["L_read_GBps"] = round(8 * entries / (r[name]["ms"] * 1e-3) / 1e9, 1)
    # the products undo the half solves: a sanity figure, not a test
    for tag, mul, slv in (("L", sc.SC_OP_MUL_L, sc.SC_OP_SOLVE_L), ("Lt", sc.SC_OP_MUL_LT, sc.SC_OP_SOLVE_LT)):
        num.apply_device_multi(mul, d_B.data_ptr(), NRHS, n, d_X.data_ptr(), n)
        num.apply_device_multi(slv, d_X.data_ptr(), NRHS, n, d_X.data_ptr(), n)
        res["rel_round_trip_" + tag] = float((torch.linalg.norm(d_X - d_B) / torch.linalg.norm(d_B)).item())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
