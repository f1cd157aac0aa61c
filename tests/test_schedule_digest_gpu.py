"""Ties the host-only schedule digests (tests/test_schedule_digest.py) to the product
path: a live handle's digest, hashed at creation from what it uploads with the pointers
rebased by the real pool bases, equals the digest planned on the host with no device."""
import os

import pytest

import sparsecholesky_amd as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case,opts,nranks", [
    ("bcsstk01", {}, 1), ("1138_bus", {}, 1), ("lap16", {}, 1),
    ("lap20", dict(panel_nb_outer=128, dist_cbb=64, small_front_max=32), 4)])
def test_live_digest_equals_host_digest(gpu, case, opts, nranks):
    A = (sc.laplacian3d(int(case[3:])) if case.startswith("lap") else
         sc.load_matrix_market_to_csc(os.path.join(GOLDEN, case + ".mtx")))
    s = sc.Symbolic(A, **opts)
    num = sc.Numeric(s, nranks=nranks, virtual=nranks > 1)
    live = num.schedule_digest()
    assert sum(live["calls"].values()) > 0
    assert live == s.schedule_digest(nranks, 0, 1 if nranks > 1 else 0)
    assert num.factor(A.x) == 0  # the hashed schedule is the one that runs
