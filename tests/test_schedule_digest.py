"""The launch schedule itself, pinned: digests of what a factorization issues, computed on
the host (Symbolic.schedule_digest, no GPU), against tests/golden/schedule_digests.json.

A digest is a 64-bit hash over every decoded schedule entry (launcher, kernel instance,
stream, hosted rank, task / tile ranges, event, step, flops and bytes) and every task
array a handle uploads, plus counters per call kind.  The parity tests see only the
factor; a reordered launch or a lost event wait shows here.

The golden file was written from the schedule builder as it was before it was split
into ScheduleBuilder (`python tests/test_schedule_digest.py --write` rewrites it: only
for a change that is meant to alter a schedule).
"""
import json
import os
import sys

import numpy as np
import pytest

import sparsecholesky_amd as sc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "schedule_digests.json")

# tests/test_gpu_parity.py: PANEL_OPTS, the dense-1350 option sets of PANEL_CASES, the
# options of test_schedule_variants_bitwise_lap48
PANEL_OPTS = [dict(inner_order=0), dict(inner_order=0, lookahead=0), dict(lookahead=0), dict(asm_tile_min_m=1),
              dict(asm_tile_min_m=300), dict(panel_nb_outer=128, lookahead=0), dict(trsm_split_wg=1),
              dict(trsm_split_wg=1, panel_nb_outer=128), dict(panel_nb_outer=192, inner_order=0),
              dict(syrk_lean_kmax=0), dict(cb_tail_split=0)]
DENSE_OPTS = [{}, dict(panel_nb_outer=128), dict(panel_nb_outer=192, inner_order=0)]
LAP48_OPTS = [dict(trsm_split_wg=0), dict(syrk_lean_kmax=0), dict(cb_tail_split=0), dict(trsm_split_wg=1)]
SPLIT = dict(panel_nb_outer=128, dist_cbb=64, small_front_max=32)  # test_partitioned_split_fronts_emulated


def _single():
    rows = []
    for name in ("bcsstk01", "lap3", "lap4"):
        rows += [(name, dict(tiny_dense=t)) for t in (1, 0)]
    rows += [("1138_bus", {}), ("lap16", {}), ("lap16", dict(small_front_max=0)),
             ("lap16", dict(small_front_max=0, panel_nb_outer=128))]
    for o in PANEL_OPTS:
        rows += [("lap20", o), ("lap20", dict(small_front_max=0, **o)), ("dense1350", o)]
    rows += [("lap20", dict(small_front_max=0)), ("lap20", dict(small_front_max=0, trsm_split_wg=0))]
    for pf in (0, 1):
        rows += [("lap20", dict(small_front_max=0, panel_prefactor=pf, panel_nb_outer=nbo)) for nbo in (64, 128)]
        rows += [("dense1350", dict(panel_prefactor=pf, **o)) for o in DENSE_OPTS]
    rows += [("lap24", {}), ("lap32", {}), ("lap48", {}), ("lap64", {})]
    rows += [("lap48", o) for o in LAP48_OPTS]
    return rows


def _multi():
    """(nranks, matrix, opts) rows of tests/test_dist.py, tests/test_dist_gpu.py and the two
    partition matrices of tests/test_gpu_parity.py, then the defaults at 48^3 and 64^3."""
    rows = [(2, 16, {}), (4, 20, {}), (4, 20, SPLIT), (3, 24, dict(dist_cbb=128)), (4, 20, dict(dist_split=0)),
            (8, 24, dict(panel_nb_outer=128, dist_cbb=64)), (4, 20, dict(panel_nb_outer=128, dist_panel=0)),
            (8, 24, dict(panel_nb_outer=128, dist_cbb=64, dist_asm=0)), (3, 24, dict(dist_cbb=128, dist_asm=0)),
            (4, 24, dict(panel_nb_outer=256, dist_pieces=1)), (4, 24, dict(panel_nb_outer=256, dist_pieces=3))]
    rows += [(2, 32, {}), (4, 32, {}), (2, 20, dict(dist_cbb=64, small_front_max=32)),
             (3, 20, dict(dist_cbb=64, dist_early=0)), (3, 20, dict(panel_nb_outer=128, dist_cbb=128)),
             (4, 20, dict(panel_nb_outer=128, dist_cbb=64, dist_split=0))]
    for n, o in [(2, {}), (3, {}), (4, {}), (8, {}), (4, dict(dist_panel=0)), (3, dict(dist_split=0)),
                 (8, dict(dist_split=0)), (4, dict(lookahead=0, inner_order=0)), (4, dict(dist_asm=0)),
                 (8, dict(dist_asm=0)), (3, dict(dist_panel=0, dist_asm=0)), (4, dict(dist_pieces=1)),
                 (8, dict(dist_pieces=8))]:
        rows.append((n, 20, dict(SPLIT, **o)))
    for n, o in [(2, {}), (4, {}), (8, {}), (8, dict(dist_asm=0)), (4, dict(dist_asm=0)), (4, dict(dist_pieces=1)),
                 (8, dict(dist_pieces=16)), (2, dict(dist_local_pieces=0)), (4, dict(dist_local_pieces=0)),
                 (4, dict(dist_pieces=3))]:
        rows.append((n, 48, o))
    rows += [(n, 64, {}) for n in (2, 4, 8)]
    out = []
    for r in rows:
        if r not in out:
            out.append(r)
    return [(n, "lap%d" % k, o) for n, k, o in out]


def _key(name, opts):
    return name + "".join(",%s=%s" % kv for kv in sorted(opts.items()))


def _groups():
    """{symbolic key: (matrix, opts, [(nranks, rank, emulate)])}: one analysis per group."""
    g = {}
    for name, o in _single():
        g.setdefault(_key(name, o), (name, o, []))[2].append((1, 0, 0))
    for n, name, o in _multi():
        modes = g.setdefault(_key(name, o), (name, o, []))[2]
        modes += [(n, 0, 1), (n, 0, 2)] + [(n, r, 0) for r in range(n)]
    # the bench and projection configuration, every rank in one process
    g.setdefault("lap128", ("lap128", {}, []))[2].append((8, 0, 1))
    return g


GROUPS = _groups()
_matrices = {}


def matrix(name):
    if name not in _matrices:
        if name.startswith("lap"):
            A = sc.laplacian3d(int(name[3:]))
        elif name == "dense1350":  # one dense front: the analysis reads the pattern only
            n = 1350
            p = np.cumsum(np.arange(n + 1, dtype=np.int64))
            i = np.concatenate([np.arange(j + 1, dtype=np.int32) for j in range(n)])
            A = sc.csc_matrix(n, n, p, i, np.ones(len(i)))
        else:
            A = sc.load_matrix_market_to_csc(os.path.join(HERE, "golden", name + ".mtx"))
        _matrices[name] = A
    return _matrices[name]


def flat(d):
    return [d["hash"]] + list(d["calls"].values()) + [d[c] for c in ("tail_split", "pf", "comm_steps", "events",
                                                                     "msgs", "gsegs")]


def group_digests(key):
    name, opts, modes = GROUPS[key]
    s = sc.Symbolic(matrix(name), **opts)
    return {"%s|n%d,r%d,e%d" % ((key,) + m): flat(s.schedule_digest(*m)) for m in modes}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_lists_exactly_the_cases(golden):
    want = {"%s|n%d,r%d,e%d" % ((k,) + m) for k, (_, _, modes) in GROUPS.items() for m in modes}
    assert set(golden) == want


@pytest.mark.parametrize("key", sorted(GROUPS))
def test_schedule_digest_matches_golden(golden, key):
    got = group_digests(key)
    bad = {c: (v, golden.get(c)) for c, v in got.items() if golden.get(c) != v}
    assert not bad, bad


def test_every_emission_path_is_hit(golden):
    # every decoded call kind and every counter is non-zero in some pinned case
    names = list(sc.CALL_KINDS) + ["tail_split", "pf", "comm_steps", "events", "msgs", "gsegs"]
    total = np.sum([v[1:] for v in golden.values()], axis=0)
    assert len(total) == len(names)
    assert not [n for n, t in zip(names, total) if t <= 0]


@pytest.mark.parametrize("key,mode", [("1138_bus", (1, 0, 0)), ("lap20,small_front_max=0", (1, 0, 0)),
                                      (_key("lap20", SPLIT), (4, 0, 1)), (_key("lap20", SPLIT), (4, 2, 0))])
def test_digest_is_deterministic(key, mode):
    name, opts, _ = GROUPS[key]
    s = sc.Symbolic(matrix(name), **opts)
    assert s.schedule_digest(*mode) == s.schedule_digest(*mode)
    assert sc.Symbolic(matrix(name), **opts).schedule_digest(*mode) == s.schedule_digest(*mode)


@pytest.mark.parametrize("name,base,mode,opt,a,b", [
    ("lap20", dict(small_front_max=0, panel_nb_outer=128), (1, 0, 0), "lookahead", 0, 1),  # several slabs
    ("lap20", dict(small_front_max=0), (1, 0, 0), "inner_order", 0, 1),
    ("lap20", dict(small_front_max=0), (1, 0, 0), "trsm_split_wg", 0, 1),
    ("lap48", {}, (1, 0, 0), "cb_tail_split", 0, 1),
    ("lap24", dict(panel_nb_outer=256), (4, 0, 1), "dist_pieces", 1, 3),
    ("lap20", SPLIT, (4, 0, 1), "dist_asm", 0, 1),
    ("lap20", SPLIT, (4, 1, 0), "dist_asm", 0, 1),
])
def test_digest_differs_where_the_schedule_must(name, base, mode, opt, a, b):
    da, db = (sc.Symbolic(matrix(name), **dict(base, **{opt: v})).schedule_digest(*mode) for v in (a, b))
    assert da["hash"] != db["hash"]


if __name__ == "__main__":
    assert sys.argv[1:] == ["--write"], "usage: test_schedule_digest.py --write"
    out = {}
    for k in sorted(GROUPS):
        out.update(group_digests(k))
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(c), json.dumps(out[c])) for c in sorted(out)) + "\n}\n")
    print("wrote %d digests" % len(out))
