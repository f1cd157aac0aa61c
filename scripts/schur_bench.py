#!/usr/bin/env python3
"""Schur complement of the middle plane of lap k^3 (natural grid order, ordering = ND, S = the
plane x = k / 2, ns = k^2), next to the unconstrained ND factorization of the same k.

  python scripts/schur_bench.py [--k 64 128] [--reps 5] [--outdir profiles/schur]

Every size runs in a child process of its own under `timeout`, one after the other, and the
first failure ends the run (nothing more is started on the device after a fault or a hang).
Per size one JSON line: factor ms of the Schur handle and of the plain ND handle, gather ms
(sc_schur_factor_device after a new factorization minus the same call on the cached D: both
copy D once), product ms (sc_schur_matrix_device on the cached D) and its TFLOP/s at ns^3 / 3
flops, beside the TFLOP/s sc_debug_bench(which=1) reports for the existing SYRK at M = ns,
K = ns / 2 (by its own count, M (M + 1) K), condense and expand ms of a 16-column device
panel, and the memory of the handle.  Each value is the median of --reps synchronous calls
after a warm-up."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMIT = {64: 300, 128: 900}  # seconds per child


def child(k, reps, out):
    import numpy as np
    import torch

    import sparsecholesky_amd as sc

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: returns after the library stream is idle
        return (time.perf_counter() - t0) * 1e3

    def note(what):
        print(f"schur_bench k={k}: {what}", file=sys.stderr, flush=True)

    def median_ms(fn, before=None):
        fn()
        t = []
        for _ in range(reps):
            if before:
                before()
            t.append(wall_ms(fn))
        return statistics.median(t)

    if sc.lib().sc_device_count() <= 0:
        raise SystemExit("schur_bench: no HIP device visible")
    A = sc.laplacian3d(k, nd=False)
    n = A.size()
    idx = np.nonzero(np.arange(n) % k == k // 2)[0].astype(np.int32)
    ns = len(idx)
    d_Ax = torch.from_numpy(A.x).to("cuda:0")
    t0 = time.perf_counter()
    plain_symb = sc.Symbolic(A, ordering=1)
    t_an_plain = time.perf_counter() - t0
    note(f"plain ND analysis {t_an_plain:.1f} s")
    plain = sc.Numeric(plain_symb, device=0)
    factor_plain = median_ms(lambda: plain.factor_device(d_Ax.data_ptr(), sync=True))
    plain_stats = plain_symb.stats()
    del plain
    torch.cuda.empty_cache()
    t0 = time.perf_counter()
    symb = sc.Symbolic(A, ordering=1, schur=idx)
    t_an = time.perf_counter() - t0
    note(f"plain ND factor {factor_plain:.1f} ms; Schur analysis {t_an:.1f} s")
    num = sc.Numeric(symb, device=0)
    refactor = lambda: num.factor_device(d_Ax.data_ptr(), sync=True)
    factor = median_ms(refactor)
    assert num.status() == 0
    mem0 = num.memory()
    dD = torch.empty(ns * ns, device="cuda:0", dtype=torch.float64)
    dS = torch.empty(ns * ns, device="cuda:0", dtype=torch.float64)
    gather_copy = median_ms(lambda: num.schur_factor_device(dD.data_ptr(), ns), before=refactor)
    copy = median_ms(lambda: num.schur_factor_device(dD.data_ptr(), ns))
    product = median_ms(lambda: num.schur_complement_device(dS.data_ptr(), ns))
    mem1 = num.memory()
    note(f"factor {factor:.1f} ms, gather + copy {gather_copy:.1f} ms, product {product:.1f} ms")
    # validation at scale: S_c is symmetric and S_c x = D (D^T x) for a random x
    x = torch.randn(ns, device="cuda:0", dtype=torch.float64)
    Dm, Sm = dD.view(ns, ns).T, dS.view(ns, ns).T  # column-major buffers
    resid = float((Sm @ x - Dm @ (Dm.T @ x)).norm() / (Sm @ x).norm())
    symmetric = bool(torch.equal(Sm, Sm.T))
    dB = torch.randn(16 * n, device="cuda:0", dtype=torch.float64)
    dG = torch.empty(16 * ns, device="cuda:0", dtype=torch.float64)
    dX = torch.empty(16 * n, device="cuda:0", dtype=torch.float64)
    condense = median_ms(lambda: num.schur_condense_device_multi(dB.data_ptr(), 16, n, dG.data_ptr(), ns))
    dXS = torch.linalg.solve(Sm, dG.view(16, ns).T).T.contiguous()
    expand = median_ms(lambda: num.schur_expand_device_multi(dB.data_ptr(), 16, n, dXS.data_ptr(), ns, dX.data_ptr(), n))
    solve = median_ms(lambda: num.solve_device_multi(dB.data_ptr(), 16, n, dX.data_ptr(), n))
    mem2 = num.memory()
    del dD, dS, Dm, Sm
    torch.cuda.empty_cache()
    tf = ctypes.c_double()
    rc = sc.lib().sc_debug_bench(1, ns, ns // 2, 3, 128, ctypes.byref(tf))
    rec = dict(bench="schur", k=k, n=n, ns=ns, reps=reps, analyze_s=round(t_an, 2), analyze_plain_nd_s=round(t_an_plain, 2),
               nnz_L=symb.nnz_L, nnz_L_plain_nd=plain_symb.nnz_L, flops=symb.flops, flops_plain_nd=plain_symb.flops,
               max_front_m=symb.stats()["max_front_m"], max_front_m_plain_nd=plain_stats["max_front_m"],
               factor_ms=round(factor, 3), factor_plain_nd_ms=round(factor_plain, 3),
               gather_ms=round(gather_copy - copy, 3), gather_and_copy_ms=round(gather_copy, 3), copy_ms=round(copy, 3),
               product_ms=round(product, 3), product_tflops=round(ns ** 3 / 3.0 / (product * 1e-3) / 1e12, 3),
               syrk_tflops_M_ns_K_half=round(tf.value, 3) if rc == 0 else None,
               condense16_ms=round(condense, 3), expand16_ms=round(expand, 3), solve16_ms=round(solve, 3),
               product_check_rel=resid, symmetric=symmetric,
               memory_after_factor=mem0, memory_after_schur=mem1, memory_after_partial_solves=mem2,
               hot_kernel="schur_llt_kernel (v_mfma_f64_16x16x4_f64)")
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles", "schur"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.k[0], a.reps, os.path.join(a.outdir, f"schur_k{a.k[0]}.jsonl"))
        return
    for k in a.k:  # one child per size, each under its own limit; the first failure ends the run
        limit = LIMIT.get(k, 900)
        rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child",
                             "--k", str(k), "--reps", str(a.reps), "--outdir", a.outdir]).returncode
        if rc != 0:
            raise SystemExit(f"schur_bench: k = {k} ended with status {rc}; nothing more is started")


if __name__ == "__main__":
    main()
