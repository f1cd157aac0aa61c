#!/usr/bin/env python3
"""Single-vector solve against the 16-column panel solve on lap k^3 (ND order), one handle.

  python scripts/solve_multi_bench.py [--k 128] [--reps 11] [--out FILE]

Prints one JSON line: the single-vector time, and for nrhs = 1, 4, 16, 64 the multi
time, the time per right-hand side and the equivalent L-read rate (2 sweeps x 8 bytes x
panel entries over the time per 16-column panel).  Every figure is the median of
--reps synchronous calls on device arrays after a warm-up of the same shape (the calls
end in a stream synchronise, so the host clock around them is the device time plus the
launch of one graph per panel).  16 x the single-vector time of the same run is what 16
solves cost without the panel path."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import sparsecholesky_amd as sc  # noqa: E402

NRHS = (1, 4, 16, 64)


def timed(fn, reps):
    fn()  # warm-up: first launch of the shape (graph capture, code objects)
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: returns after the library stream is idle
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None, help="also append the JSON line to this file")
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10")
    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("solve_multi_bench: no HIP device visible")
    A = sc.laplacian3d(a.k)
    s = sc.Symbolic(A)
    n = A.size()
    num = sc.Numeric(s, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0
    entries = s.stats()["panel_entries"]
    g = torch.Generator(device="cuda:0").manual_seed(1)
    d_B = torch.randn((max(NRHS), n), dtype=torch.float64, device="cuda:0", generator=g)  # column j = row j
    d_X = torch.empty_like(d_B)
    mem0 = num.memory()["total"]
    med, lo, hi = timed(lambda: num.solve_device(d_B.data_ptr(), d_X.data_ptr()), a.reps)
    res = dict(bench="solve_multi", k=a.k, n=n, panel_entries=entries, L_bytes=8 * entries, reps=a.reps,
               single_ms=round(med, 4), single_min_ms=round(lo, 4), single_max_ms=round(hi, 4),
               single_L_read_GBps=round(2 * 8 * entries / (med * 1e-3) / 1e9, 1), multi={})
    for nrhs in NRHS:
        med, lo, hi = timed(lambda: num.solve_device_multi(d_B.data_ptr(), nrhs, n, d_X.data_ptr(), n), a.reps)
        panels = (nrhs + 15) // 16
        res["multi"][str(nrhs)] = dict(ms=round(med, 4), min_ms=round(lo, 4), max_ms=round(hi, 4),
                                       ms_per_rhs=round(med / nrhs, 4),
                                       L_read_GBps=round(2 * 8 * entries / (med / panels * 1e-3) / 1e9, 1))
    res["panel_buffer_bytes"] = num.memory()["total"] - mem0
    res["sixteen_single_ms"] = round(16 * res["single_ms"], 4)
    res["panel16_over_single"] = round(res["multi"]["16"]["ms"] / res["single_ms"], 3)
    res["speedup_16_rhs"] = round(res["sixteen_single_ms"] / res["multi"]["16"]["ms"], 2)
    # the two paths agree to rounding on the first right-hand side
    num.solve_device(d_B.data_ptr(), d_X.data_ptr())
    x1 = d_X[0].clone()
    num.solve_device_multi(d_B.data_ptr(), 16, n, d_X.data_ptr(), n)
    res["rel_diff_single_vs_panel"] = float((torch.linalg.norm(d_X[0] - x1) / torch.linalg.norm(x1)).item())
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
