"""Host tests of the prescribed-tree catalogue (tests/zoo.py): the generator against the
analysis, every case against the code path it is named for (read off the host schedule digest
and the supernode partition), multi-rank plans, the oracle against the long-double factor, and
the expected status of inputs with two failing pivots; for the big_ cases the SYRK kernel
instance every case and tag reaches (Symbolic.syrk_launches), and the argument checks of the
kernel debug hooks.  No GPU."""
import numpy as np
import pytest

import oracle
import sparsecholesky_amd as sc
import zoo

TINY_PR_LDS, TINY_MAX_LDS, CHAIN_MAXF = 2048, 12288, 256  # kernels.hpp


def _partition(symb):
    """The analysis' supernodes as {first natural column: (w, m, parent's first natural column or -1)}."""
    sn = symb.supernodes()
    _, post = symb.etree()
    first = [int(post[sn["start"][s]]) for s in range(len(sn["w"]))]
    out = {}
    for s in range(len(sn["w"])):
        cols = post[sn["start"][s]:sn["start"][s + 1]]
        assert np.array_equal(cols, np.arange(first[s], first[s] + len(cols))), "a front's columns are contiguous"
        p = int(sn["parent"][s])
        out[first[s]] = (int(sn["w"][s]), int(sn["m"][s]), first[p] if p >= 0 else -1)
    return out


def _children(sn):
    par = sn["parent"]
    return np.bincount(par[par >= 0], minlength=len(par))


def _pairs(sn):
    mb = (sn["m"] - sn["w"]).astype(np.int64)[sn["parent"] >= 0]
    return int((mb * (mb + 1) // 2).sum())


def _lds(sn):
    m, mb = sn["m"].astype(np.int64), (sn["m"] - sn["w"]).astype(np.int64)
    return int((m * (m + 1) // 2 + mb * (mb + 1) // 2).sum())


def _max_small_on_a_level(sn, small_front_max=128):
    lev = sn["level"]
    return max(int(np.sum((lev == L) & (sn["m"] <= small_front_max))) for L in range(int(lev.max()) + 1))


# ---- 1. the generator against the analysis ----
@pytest.mark.parametrize("name", zoo.NAMES)
def test_partition_at_relax0_is_the_spec(name):
    c = zoo.case(name)
    st = c.st
    symb = sc.Symbolic(c.A, relax=0)
    want = {int(st.start[f]): (int(st.w[f]), int(st.m[f]), int(st.start[st.parent[f]]) if st.parent[f] >= 0 else -1)
            for f in range(len(st.w))}
    assert _partition(symb) == want
    nnz = sum(int(m) - j for m, w in zip(st.m, st.w) for j in range(int(w)))
    assert symb.nnz_L == nnz == st.nnz_L
    Lp, Li = st.pattern()
    oLp, oLi, _ = oracle.schol(c.A)
    assert np.array_equal(oLp, Lp) and np.array_equal(oLi, Li)
    pLp, pLi = symb.pattern()
    assert np.array_equal(pLp, Lp) and np.array_equal(pLi, Li)


@pytest.mark.parametrize("name", ["tiny_hbm_pairs", "chain300_edges", "forest"])
def test_llt_values_keep_the_partition(name):
    # A = L0 L0^T has no accidental zeros on the pattern: same analysis as the dd values
    a, b = zoo.case(name, "dd").A, zoo.case(name, "llt").A
    assert np.array_equal(a.p, b.p) and np.array_equal(a.i, b.i)
    assert np.all(b.x != 0.0)
    D = zoo.case(name, "llt").dense()
    assert np.linalg.cond(D) < 1e4


# ---- 2. every case reaches the path it is named for ----
def _calls(name, **kw):
    symb = sc.Symbolic(zoo.case(name).A, **kw)
    return symb, symb.supernodes(), symb.schedule_digest()["calls"]


@pytest.mark.parametrize("kw", [dict(relax=0), {}], ids=["relax0", "default"])
def test_tiny_hbm_pairs_reads_pairs_from_hbm(kw):
    symb, sn, calls = _calls("tiny_hbm_pairs", **kw)
    assert symb.n > 64 and calls["tiny_tree"] == 1 and calls["front_small"] == 0
    print(f"tiny_hbm_pairs {kw}: {_pairs(sn)} pairs, LDS {_lds(sn)} doubles, {len(sn['w'])} fronts")
    assert _pairs(sn) > TINY_PR_LDS
    assert _lds(sn) <= TINY_MAX_LDS


def test_tiny_limits_from_both_sides():
    symb, sn, calls = _calls("tiny_16_m64", relax=0)
    assert len(sn["w"]) == 16 and sn["m"].max() == 64 and calls["tiny_tree"] == 1
    assert _pairs(sn) > TINY_PR_LDS
    symb, sn, calls = _calls("tiny_17", relax=0)
    assert len(sn["w"]) == 17 and sn["m"].max() == 64
    assert calls["tiny_tree"] == 0 and calls["front_small"] >= 1
    symb, sn, calls = _calls("tiny_m65", relax=0)
    assert len(sn["w"]) == 16 and sn["m"].max() == 65
    assert calls["tiny_tree"] == 0 and calls["front_small"] >= 1
    symb, sn, calls = _calls("tiny_lds_under", relax=0)
    assert len(sn["w"]) <= 16 and sn["m"].max() <= 64
    assert TINY_MAX_LDS - 64 < _lds(sn) <= TINY_MAX_LDS and calls["tiny_tree"] == 1
    symb, sn, calls = _calls("tiny_lds_over", relax=0)
    assert len(sn["w"]) <= 16 and sn["m"].max() <= 64
    assert TINY_MAX_LDS < _lds(sn) < TINY_MAX_LDS + 64
    assert calls["tiny_tree"] == 0 and calls["front_small"] >= 1


def test_chains():
    symb, sn, calls = _calls("chain300_edges", relax=0)
    assert len(sn["w"]) == 301 and _children(sn).max() == 1
    assert CHAIN_MAXF < 300 <= 2 * CHAIN_MAXF
    assert calls["chain"] == 2  # the contribution block of front 255 crosses from one launch to the next
    m = set(sn["m"][:300].tolist())
    assert {31, 32, 33, 63, 64, 65, 87, 88, 89, 95, 96, 97, 127, 128} <= m  # every LDS bucket edge
    # the chain's last front hands its rows to the large root, past its pivots' first block
    st = zoo.case("chain300_edges").st
    assert st.m[300] > 128 and (st.rows[299][st.w[299]:] - st.start[300]).max() == 139
    symb, sn, calls = _calls("chain_into_large_tail", relax=0)
    assert calls["chain"] == 1 and len(sn["w"]) == 6
    st = zoo.case("chain_into_large_tail").st
    rel = st.rows[4][st.w[4]:] - st.start[5]  # positions in the parent's front: beyond 8 bits
    assert (rel >= 256).sum() == 39 and st.m[5] == 300


@pytest.mark.parametrize("kw", [dict(relax=0), {}], ids=["relax0", "default"])
def test_fan_in(kw):
    symb, sn, calls = _calls("star300_large_root", **kw)
    root = int(np.argmax(_children(sn)))
    assert _children(sn)[root] >= 300 and sn["m"][root] > 128
    assert _max_small_on_a_level(sn) > 256 and calls["front_small"] >= 2  # bucketed launches
    symb, sn, calls = _calls("star100_small_root", **kw)
    root = int(np.argmax(_children(sn)))
    assert _children(sn)[root] >= 99 and sn["m"][root] <= 128
    symb, sn, calls = _calls("fanin300_mid_cb", **kw)
    mid = int(np.argmax(_children(sn)))
    assert _children(sn)[mid] >= 300 and sn["m"][mid] > 128 and sn["m"][mid] > sn["w"][mid]
    assert sn["parent"][mid] >= 0 and calls["syrk_cb"] >= 1
    assert symb.schedule_digest()["gsegs"] > 0  # the fan-in parent's CB is gathered from its 300 children


def test_block_edges_and_forest():
    for name in ("edges_a", "edges_b"):
        symb, sn, calls = _calls(name, relax=0)
        assert calls["syrk_cb"] >= 1 and calls["trsm_partial"] >= 1
    symb, sn, calls = _calls("edges_a", relax=0)
    assert sorted(zip(sn["w"].tolist(), (sn["m"] - sn["w"]).tolist())) == sorted(
        [(63, 1), (64, 64), (65, 63), (1, 128), (1, 129), (200, 0)])
    for kw in (dict(relax=0), {}):
        symb, sn, calls = _calls("forest", **kw)
        roots = np.flatnonzero(sn["parent"] < 0)
        assert len(roots) == 8  # roots of every class: isolated columns, small, large with mb = 0
        assert (sn["m"][roots] > 128).sum() == 2 and (sn["w"][roots] == 1).sum() == 3
    symb, sn, calls = _calls("forest", relax=0)
    assert sorted(sn["w"][sn["parent"] < 0].tolist()) == [1, 1, 1, 2, 3, 6, 130, 150]
    assert calls["chain"] >= 1 and calls["front_small"] >= 1 and calls["syrk_cb"] >= 1
    st = zoo.case("forest").st
    assert st.w[0] == 1 and st.w[-1] == 1 and st.parent[-1] < 0  # isolated columns first and last


# ---- 2b. the big_ cases: which SYRK instance each case and tag reaches ----
def _launches(name, tag):
    """(symbolic, {(kind, bt, lean, epi, pf, gather): [tile counts]}, calls) of a case's host schedule under a tag."""
    symb = sc.Symbolic(zoo.case(name).A, **zoo.OPTS[tag])
    inst = {}
    for l in symb.syrk_launches():
        inst.setdefault((l["kind"], l["bt"], l["lean"], l["epi"], l["pf"], l["gather"]), []).append(l["tiles"])
        assert l["tail"] == 0  # see test_big_cases_cover_every_syrk_instance
    return symb, inst, symb.schedule_digest()["calls"]


CB128_G1, CB128_G0 = ("cb", 128, 0, 1, 0, 1), ("cb", 128, 0, 0, 0, 1)  # 128-tile gather: short K (epi 1), deep K
CB64L_G1 = ("cb", 64, 1, 1, 0, 1)                                      # lean 64-tile gather


def test_big_gather_cases_reach_their_cb_instance():
    _, inst, _ = _launches("big_gather_k40", "relax0")
    assert inst[CB128_G1] == [6]  # the parent's 300-row CB: 2 x 128 + 44, partial edge tiles
    _, inst, _ = _launches("big_gather_k100", "relax0")
    assert CB64L_G1 in inst and not any(k[0] == "cb" and k[1] == 128 for k in inst)  # 64 < K <= 128: lean although wide
    symb, inst, calls = _launches("big_gather_k200", "relax0")
    assert CB128_G0 in inst and ("panel", 128, 0, 1, 0, 0) in inst
    assert calls["asm_tiled"] >= 1 and calls["trsm_pre"] >= 1 and calls["trsm_partial"] >= 1 and calls["trsm_fused"] >= 1
    assert sorted(symb.supernodes()["m"].tolist())[-3:] == [642, 677, 713]  # above ASM_TILE_MIN_M and 2 x TRSM_ROWS
    _, inst, calls = _launches("big_gather_k200", "nbo128")
    assert ("panel", 128, 0, 0, 0, 0) in inst and ("panel", 64, 1, 0, 0, 0) in inst  # the lookahead stream's instances
    assert calls["record"] >= 1 and calls["wait"] >= 1
    _, inst, _ = _launches("big_gather_k200", "nbo192")
    assert ("panel", 64, 0, 0, 0, 0) in inst  # K = 192: past the lean instance, on the lookahead stream
    symb, inst, _ = _launches("big_nested_gather", "relax0")
    assert int(symb.supernodes()["level"].max()) == 3  # four levels: a gather reads a CB a gather wrote
    assert CB128_G1 in inst and CB64L_G1 in inst
    symb, inst, _ = _launches("big_fanin40_tile128", "relax0")
    assert inst[CB128_G1] == [6]
    assert symb.schedule_digest()["gsegs"] > 40 * 3  # many children in every block of the parent's CB


@pytest.mark.parametrize("tag", ["relax0", "default"])
def test_big_cb_edge_cases_pick_the_tile_per_launch(tag):
    # the parent's mb x mb CB: 255 stays on 64-tiles, 256 is three 128-tiles, 257 six (the
    # last row and column of them one wide); the parent survives the default amalgamation
    want = {"big_cb255": None, "big_cb256": [3], "big_cb257": [6]}
    for name, tiles in want.items():
        symb, inst, _ = _launches(name, tag)
        mb = int(name[-3:])
        assert (40, 40 + mb) in zip(symb.supernodes()["w"].tolist(), symb.supernodes()["m"].tolist())
        assert inst.get(CB128_G1) == tiles, (name, inst)
        assert ("cb", 64, 0, 1, 0, 1) in inst  # the children's CBs, and at 255 the parent's


def test_big_cases_that_survive_the_default_amalgamation():
    whole = []
    for name in zoo.BIG_FRONTS:
        a, b = (_partition(sc.Symbolic(zoo.case(name).A, **kw)) for kw in (dict(relax=0), {}))
        if a == b:
            whole.append(name)
    # elsewhere the parent, the front before the root, merges into the root
    assert whole == ["big_cb255", "big_cb256", "big_cb257"]
    assert tuple(n for n in zoo.SURVIVE_RELAX if n in zoo.BIG_FRONTS) == tuple(whole)


@pytest.mark.parametrize("name", zoo.BIG_FRONTS)
def test_big_tags_change_what_they_are_named_for(name):
    _, inst, calls = _launches(name, "tile128")
    assert all(k[1] == 128 and k[2] == 0 and k[4] == 0 for k in inst)  # every SYRK on 128-tiles, no pre-factor
    assert calls["trsm_pre"] == 0 and calls["trsm_fused"] >= 1           # so every TRSM is fused
    _, inst0, calls0 = _launches(name, "relax0")
    _, _, calls = _launches(name, "trsm_split")
    assert calls["potrf"] > calls0["potrf"] and calls["trsm_pre"] > calls0["trsm_pre"]
    _, inst, calls = _launches(name, "nbo128")
    assert calls["record"] >= 1 and any(k[0] == "panel" and k[3] == 0 for k in inst)  # lookahead-stream updates
    _, inst, calls = _launches(name, "nbo128_rl")
    assert calls["record"] == 0 and not any(k[4] for k in inst) and calls["trsm_pre"] == 0
    _, inst, calls = _launches(name, "tiled_nogather")
    assert calls["asm_tiled"] >= 1 and calls["asm_cols"] == 0 and not any(k[5] for k in inst)
    _, _, calls = _launches(name, "allfronts")
    assert calls["front_small"] == 0


def test_big_cases_cover_every_syrk_instance():
    # over the big_ cases and their tags: every (kind, tile, lean, epi) the schedule's rules
    # allow, CB launches with and without the gather.  The rules (push_syrk_launch) exclude:
    # lean CB launches with epi = 0 (lean needs K <= 128, epi = 0 needs K >= 192) and
    # pre-factoring panel launches with epi = 0 (pf forces epi = 1, plain 64-tiles).
    # tail = 1 (the re-cut last round of a deep-K CB launch) needs more than 512 tiles of
    # 128: no small case reaches it, lap48 (tests/test_gpu_parity.py) remains its only cover.
    seen = set()
    for name in zoo.BIG_FRONTS:
        for tag in zoo.tags(name):
            seen |= set(_launches(name, tag)[1])
    want = set()
    for g in (0, 1):
        want |= {("cb", 64, 0, 0, 0, g), ("cb", 64, 0, 1, 0, g), ("cb", 64, 1, 1, 0, g), ("cb", 128, 0, 0, 0, g),
                 ("cb", 128, 0, 1, 0, g)}
    for epi in (0, 1):
        want |= {("panel", 64, 0, epi, 0, 0), ("panel", 64, 1, epi, 0, 0), ("panel", 128, 0, epi, 0, 0)}
    want.add(("panel", 64, 0, 1, 1, 0))
    assert want <= seen, sorted(want - seen)
    assert ("cb", 64, 1, 0, 0, 0) not in seen and ("cb", 64, 1, 0, 0, 1) not in seen
    assert not any(k[4] and not k[3] for k in seen)


def test_syrk_launches_agree_with_the_digest():
    for name, tag in (("big_gather_k200", "nbo128"), ("forest", "default"), ("tiny_17", "relax0")):
        symb = sc.Symbolic(zoo.case(name).A, **zoo.OPTS[tag])
        d, ls = symb.schedule_digest(), symb.syrk_launches()
        assert sum(l["kind"] == "panel" for l in ls) == d["calls"]["syrk_panel"]
        assert sum(l["kind"] == "cb" for l in ls) == d["calls"]["syrk_cb"]
        assert sum(l["pf"] for l in ls) == d["pf"] and sum(l["tail"] for l in ls) == d["tail_split"]
        assert all(l["tiles"] >= 1 and l["bt"] in (64, 128) for l in ls)
        assert symb.schedule_digest() == d  # listing the launches leaves the digest alone
    symb = sc.Symbolic(zoo.case("big_gather_k200").A, relax=0)
    assert len(symb.syrk_launches(2, 0, 1)) >= 1 and len(symb.syrk_launches(2, 1, 0)) >= 0


# ---- 2c. the debug hooks refuse inconsistent arguments before any device call ----
def test_kernel_hooks_refuse_bad_arguments():
    import ctypes

    L = sc.lib()
    ERR = -1  # SC_ERR_ARG
    p = ctypes.c_void_p(4096)  # never dereferenced: every call below is refused on its arguments
    ok = dict(ldc=70, lda=70, M=65, N=64, K=7, bt=64, lean=0, tag=0, epi=0)

    def syrk(**kw):
        a = dict(ok, **kw)
        return L.sc_debug_syrk_ex(a.get("C", p), a["ldc"], a.get("A", p), a["lda"], a["M"], a["N"], a["K"], a["bt"],
                                  a["lean"], a["tag"], a["epi"])

    for bad in (dict(C=None), dict(A=None), dict(M=0), dict(N=0), dict(K=0), dict(N=66), dict(lda=64), dict(ldc=64),
                dict(bt=32), dict(bt=0), dict(bt=256), dict(bt=128, lean=1), dict(lean=2), dict(lean=-1), dict(tag=2),
                dict(tag=-1), dict(epi=2), dict(epi=-1), dict(lda=1 << 22), dict(ldc=1 << 22)):
        assert syrk(**bad) == ERR, bad
    assert L.sc_debug_syrk(p, 64, p, 70, 65, 64, 7) == ERR  # the old hook goes through the new one

    info = ctypes.c_int32(-7)

    def panel(m=200, w=130, k0=0, mode=1, F=p, inf=ctypes.byref(info)):
        return L.sc_debug_panel(F, m, w, k0, mode, inf)

    for bad in (dict(F=None), dict(inf=None), dict(m=0), dict(w=0), dict(w=201), dict(k0=-64), dict(k0=32), dict(k0=192),
                dict(mode=-1), dict(mode=4), dict(k0=128, mode=1), dict(k0=128, mode=2), dict(k0=64, mode=3),
                dict(k0=0, mode=3), dict(m=(1 << 22) + 1, w=64)):
        assert panel(**bad) == ERR, bad
    assert info.value == -7  # untouched

    symb = sc.Symbolic(zoo.case("tiny_17").A)
    out = np.zeros(8, dtype=np.int64)
    ptr = out.ctypes.data_as(ctypes.c_void_p)
    for args in ((None, 1, 0, 0, ptr, 8), (symb.h, 0, 0, 0, ptr, 8), (symb.h, 2, 2, 0, ptr, 8), (symb.h, 1, -1, 0, ptr, 8),
                 (symb.h, 1, 0, 3, ptr, 8), (symb.h, 1, 0, 0, ptr, -1), (symb.h, 1, 0, 0, None, 8)):
        assert L.sc_debug_schedule_syrk(*args) == ERR, args


# ---- 3. multi-rank plans on the host ----
@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("name", ["forest", "fanin300_mid_cb", "big_gather_k200"])
def test_multi_rank_plans_build(name, nranks):
    for kw in (dict(relax=0), {}):
        symb = sc.Symbolic(zoo.case(name).A, **kw)
        info = symb.dist_plan_info(nranks)
        assert len(info["gsize"]) == symb.stats()["n_supernodes"] and info["gsize"].min() >= 1
        own, work = symb.owner_map(nranks)
        assert own.min() >= 0 and own.max() < nranks
        d = symb.schedule_digest(nranks, 0, 1)
        assert sum(d["calls"].values()) > 0


# ---- 4. the oracle against long double ----
@pytest.mark.parametrize("mode", zoo.MODES)
@pytest.mark.parametrize("name", zoo.NAMES)
def test_oracle_per_front_error(name, mode):
    c = zoo.case(name, mode)
    st, Lp, Li, Lx = oracle.chol(c.A)
    assert st == 0 and np.array_equal(Lp, c.ref.Lp) and np.array_equal(Li, c.ref.Li)
    e = c.ref.front_errors(Lx)
    print(f"{name} {mode}: oracle worst per-front error E = {e.max():.3e} (front {int(e.argmax())} of {len(e)})")
    # a broken reference must not widen the GPU tests' bar of 16 E unnoticed
    assert e.max() < 1e-14


def test_long_double_references_are_consistent():
    c = zoo.case("forest", "llt")
    ref = c.ref
    n = c.n
    D = c.dense().astype(zoo.LD)
    assert np.abs(ref.L @ ref.L.T - D).max() < 1e-17 * np.abs(D).max() * n
    B = np.random.default_rng(0).standard_normal((n, 3))
    X = ref.solve(B)
    assert np.abs(D @ X - B).max() < 1e-16 * n
    assert np.abs(ref.mul_L(ref.solve_L(B)) - B).max() < 1e-16 * n
    assert np.abs(ref.mul_Lt(ref.solve_Lt(B)) - B).max() < 1e-16 * n
    assert np.abs(ref.solve(B[:, 0]) - X[:, 0]).max() == 0
    sign, ld = np.linalg.slogdet(c.dense())
    assert sign > 0 and abs(float(ref.logdet) - ld) < 1e-12 * abs(ld)


# ---- 5. two bad pivots: the expected status ----
def _independent(parent, a, b):
    for x, y in ((a, b), (b, a)):
        while x >= 0 and x != y:
            x = int(parent[x])
        if x == y:
            return False
    return True


@pytest.mark.parametrize("name", list(zoo.DOUBLE_FAILURES))
def test_two_bad_pivots_expected_status(name):
    A, (a, b) = zoo.double_failure(name)
    assert a < b
    st, _, _, _ = oracle.chol(zoo.with_bad_pivots(A, (a, b)))
    assert st == a + 1  # the reference: the first failing column in natural order
    for kw in (dict(relax=0), {}):
        symb = sc.Symbolic(A, **kw)
        parent, post = symb.etree()
        assert _independent(parent, a, b)
        ipost = np.empty_like(post)
        ipost[post] = np.arange(len(post))
        # the factorization meets b first: a status taken from the smallest internal index is b + 1
        assert ipost[a] > ipost[b], (name, kw)


@pytest.mark.parametrize("name", list(zoo.SINGLE_FAILURES))
def test_one_bad_pivot_expected_status(name):
    A, j = zoo.single_failure(name)
    st, _, _, _ = oracle.chol(zoo.with_bad_pivots(A, (j,)))
    assert st == j + 1
