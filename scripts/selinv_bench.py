#!/usr/bin/env python3
"""Selected inversion (sc_selinv) on lap k^3 (ND order), one handle per size, next to the
factorization of the same run.

  python scripts/selinv_bench.py [--k 64 128] [--reps 5] [--out FILE]

Prints one JSON line per size: the median of --reps synchronous sc_selinv calls after a
warm-up (the first call also allocates the Z panel and builds the task lists; its time is
reported separately), sc_selinv_flops and the TFLOP/s they give, the factorization time of
the same handle, the time split over the kernel classes W, Z_RK, Z_KK and push from HIP
events around every launch of one more (eager, profiled) call, and sc_numeric_memory before
and after the first call.  Validation at scale: for 16 columns k of Z (the first, the
last, 14 seeded at random) the diagonal Z[k, k] and the column below it, read from the Z
panel, against sc_solve_device_multi on the 16 unit vectors; the largest relative
difference max |Z - X| / max |X| over a column's entries is reported."""
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

NRHS = 16


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()  # synchronous: returns after the library stream is idle
    return (time.perf_counter() - t0) * 1e3


def run(k, reps):
    A = sc.laplacian3d(k)
    s = sc.Symbolic(A)
    n = A.size()
    num = sc.Numeric(s, device=0)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    assert num.factor_device(d_Ax.data_ptr(), sync=True) == 0  # warm-up (code objects)
    t_factor = [wall_ms(lambda: num.factor_device(d_Ax.data_ptr(), sync=True)) for _ in range(3)]
    mem0 = num.memory()
    t_first = wall_ms(num.selinv)
    mem1 = num.memory()
    ts = [wall_ms(num.selinv) for _ in range(reps)]
    ms = statistics.median(ts)
    flops = s.selinv_flops()
    num.selinv_times(profile=True)
    t_prof = wall_ms(num.selinv)
    split = num.selinv_times(profile=False)
    # validation: columns of Z against solves with unit vectors (no fill-reducing
    # permutation is in effect: A's order is the export's)
    rng = np.random.default_rng(k)
    cols = [0, n - 1] + sorted(rng.choice(np.arange(1, n - 1), NRHS - 2, replace=False).tolist())
    d_B = torch.zeros((NRHS, n), dtype=torch.float64, device="cuda:0")  # column j = row j
    for c, j in enumerate(cols):
        d_B[c, j] = 1.0
    torch.cuda.synchronize()
    num.solve_device_multi(d_B.data_ptr(), NRHS, n, d_B.data_ptr(), n)
    X = d_B.cpu().numpy()
    worst, worst_diag, entries = 0.0, 0.0, 0
    for c, j in enumerate(cols):
        cp, ri, rx = num.selected_inverse_cols(j, j + 1)
        assert ri[0] == j
        x = X[c, ri]
        worst = max(worst, float(np.abs(rx - x).max() / np.abs(x).max()))
        worst_diag = max(worst_diag, float(abs(rx[0] - x[0]) / abs(x[0])))
        entries += len(ri)
    return dict(bench="selinv", k=k, n=n, reps=reps, panel_entries=s.stats()["panel_entries"],
                factor_ms=round(statistics.median(t_factor), 3), factor_flops=s.stats()["flops_executed"],
                selinv_first_call_ms=round(t_first, 3), selinv_ms=round(ms, 3), selinv_min_ms=round(min(ts), 3),
                selinv_max_ms=round(max(ts), 3), selinv_flops=flops, selinv_tflops=round(flops / (ms * 1e-3) / 1e12, 3),
                flops_over_factor=round(flops / s.stats()["flops_executed"], 3),
                profiled_call_ms=round(t_prof, 3), split_ms={q: round(v, 3) for q, v in split.items()},
                hot_kernel="sel_zrk_kernel (v_mfma_f64_16x16x4_f64)",
                memory_before=mem0, memory_after=mem1, z_panel_bytes=mem0["panel"],
                selinv_extra_bytes=mem1["total"] - mem0["total"],
                validation=dict(columns=cols, entries=entries, worst_rel_diff=worst, worst_rel_diff_diag=worst_diag))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("selinv_bench: no HIP device visible")
    for k in a.k:
        line = json.dumps(run(k, a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
