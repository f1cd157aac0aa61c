"""bench.py's command line: the plain run's result line, --full, and --dump-outputs
(a fixed sample of the timed factor's columns)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

K = 12  # 1728 columns: several levels, large and small fronts, well under a second per step


def test_dump_columns_fixed_sorted_disjoint():
    for n in (64, 512, K ** 3, 128 ** 3):
        runs = bench.dump_columns(n)
        assert runs == bench.dump_columns(n)
        flat = [c for a, b in runs for c in range(a, b)]
        assert flat == sorted(set(flat)) and 0 <= flat[0] and flat[-1] == n - 1
        assert len(flat) <= 8 * (24 + 96) + 256
    top = [a for a, _ in bench.dump_columns(128 ** 3) if a >= 128 ** 3 - 256 - 8 - 262144]
    assert len(top) >= 24  # the top separators are sampled


def _run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--k", str(K), *args],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_factor(gpu, tmp_path):
    import oracle
    import sparsecholesky_amd as sc

    d = _run_bench("--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert d["unit"] == "GFLOP/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert abs(d["value"] - d["config"]["flops"] / (d["ms_per_step"] * 1e-3) / 1e9) <= 0.01 * d["value"] + 0.01
    # a plain run does not validate, time the solve or run the CPU baseline
    assert d["validation"]["backward_error"] is None and d["solve"] is None and "cpu_baseline" not in d

    arr = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in ("L_columns", "L_colptr", "L_rows", "L_values")}
    assert all(a.dtype == np.float64 for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64e6
    cols = arr["L_columns"].astype(np.int64)
    ptr = arr["L_colptr"].astype(np.int64)
    assert np.array_equal(cols, [c for a, b in bench.dump_columns(K ** 3) for c in range(a, b)])
    assert len(ptr) == len(cols) + 1 and ptr[-1] == len(arr["L_values"]) == len(arr["L_rows"])
    # against the oracle's L: same entries where the oracle has one, (relaxed) zeros elsewhere
    st, Lp, Li, Lx = oracle.chol(sc.laplacian3d(K))
    assert st == 0
    num = den = 0.0
    for t, j in enumerate(cols):
        rows = arr["L_rows"][ptr[t]:ptr[t + 1]].astype(np.int64)
        vals = arr["L_values"][ptr[t]:ptr[t + 1]]
        assert rows[0] == j
        ref = np.zeros(K ** 3)
        ref[Li[Lp[j]:Lp[j + 1]]] = Lx[Lp[j]:Lp[j + 1]]
        got = np.zeros(K ** 3)
        got[rows] = vals
        num += float(((got - ref) ** 2).sum())
        den += float((ref ** 2).sum())
    assert (num / den) ** 0.5 < 1e-12  # the parity bound of tests/test_gpu_parity.py


@pytest.mark.gpu
def test_full_run_validates_and_times_the_rest(gpu):
    d = _run_bench("--steps", "1", "--warmup", "1", "--full", "--cpu-k", "8")
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    assert d["validation"]["backward_error"] < 1e-12
    assert d["solve"]["ms"] > 0 and d["cpu_baseline"]["value"] > 0
