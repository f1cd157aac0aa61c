"""The numpy model of the gradient entry points (tests/grad_cases.py) pinned by complex-step
differentiation, deliberately wrong models shown to fail the same check, and the host-only
parts of the feature: sc_value_entries and the exported symbols.  No GPU.

Bar: worst relative deviation <= 64 u cond_2(A) (grad_cases' docstring), per input."""
import ctypes

import numpy as np
import pytest

import grad_cases as gc
import sparsecholesky_amd as sc

ENTRY = ("sc_value_entries", "sc_pattern_outer_host", "sc_pattern_outer_device", "sc_pattern_dot_host",
         "sc_pattern_dot_device", "sc_logdet_grad_host", "sc_logdet_grad_device", "sc_solve_grad_host",
         "sc_solve_grad_device")


def _bar(name):
    return 64 * gc.U * gc.cond2(name)


@pytest.mark.parametrize("name", gc.NAMES)
def test_logdet_model_against_complex_step(name):
    A = gc.matrix(name)
    g = gc.logdet_grad(A.size(), A.p, A.i, A.x)
    worst = gc.check_logdet_model(name, g)
    print(f"{name}: logdet, worst relative deviation {worst:.2e} (bar {_bar(name):.2e}, cond {gc.cond2(name):.2e})")
    assert worst <= _bar(name)


@pytest.mark.parametrize("name", gc.NAMES)
def test_solve_model_against_complex_step(name):
    A = gc.matrix(name)
    _, X, Xbar = gc.solve_data(name)
    _, g = gc.solve_grad(A.size(), A.p, A.i, A.x, Xbar, X)
    worst = gc.check_solve_model(name, g)
    print(f"{name}: solve, worst relative deviation {worst:.2e} (bar {_bar(name):.2e})")
    assert worst <= _bar(name)


def test_the_bar_of_1138_bus_is_what_the_issue_states():
    assert 5e-8 < _bar("1138_bus") < 7e-8


def test_six_has_what_it_is_for():
    Ap, Ai, _ = gc.six()
    rows, cols, eff = gc.classify(6, Ap, Ai)
    assert (rows > cols).sum() == 2 and not eff[rows > cols].any()
    assert eff.sum() == len(eff) - 2 - 3  # two below the diagonal, three superseded duplicates
    assert np.linalg.eigvalsh(gc.dense(6, Ap, Ai, gc.six()[2])).min() > 0


# ---- deliberately wrong models must fail the same checks ----
def test_factor_one_off_the_diagonal_fails():
    A = gc.matrix("six")
    g = gc.logdet_grad(6, A.p, A.i, A.x, off_factor=1.0)
    assert gc.check_logdet_model("six", g) > 0.4  # half of every off-diagonal derivative is missing


def test_derivative_on_an_ignored_duplicate_fails():
    A = gc.matrix("six")
    g = gc.logdet_grad(6, A.p, A.i, A.x, ignored=1.0)
    assert gc.check_logdet_model("six", g) > _bar("six")
    assert gc.check_logdet_model("six", g) == 1.0


def test_one_sided_outer_product_fails():
    A = gc.matrix("six")
    _, X, Xbar = gc.solve_data("six")
    _, g = gc.solve_grad(6, A.p, A.i, A.x, Xbar, X, one_sided=True)
    assert gc.check_solve_model("six", g) > 1e-3


# ---- the host-only entry point and the symbols ----
ORDERINGS = (0, 1, 2)


@pytest.mark.parametrize("name", gc.NAMES)
@pytest.mark.parametrize("ordering", ORDERINGS)
def test_value_entries_is_the_models_classification(name, ordering):
    A = gc.matrix(name)
    symb = sc.Symbolic(A, ordering=ordering)
    rows, cols, eff = symb.value_entries()
    mr, mc, me = gc.classify(A.size(), A.p, A.i)
    assert len(rows) == len(A.x)
    assert np.array_equal(rows, mr) and np.array_equal(cols, mc) and np.array_equal(eff, me)
    # consistent with the product's structure: the effective slots are exactly the set of its sp
    _, _, sp = symb.spmv_structure()
    assert np.array_equal(np.unique(sp), np.flatnonzero(eff))


def test_value_entries_of_a_schur_analysis():
    A = gc.matrix("six")
    symb = sc.Symbolic(A, schur=[4, 1])
    rows, cols, eff = symb.value_entries()
    mr, mc, me = gc.classify(6, A.p, A.i)
    assert np.array_equal(rows, mr) and np.array_equal(cols, mc) and np.array_equal(eff, me)


def test_value_entries_null_arrays_and_null_handle():
    A = gc.matrix("six")
    symb = sc.Symbolic(A)
    L = sc.lib()
    assert L.sc_value_entries(symb.h, None, None, None) == len(A.x)
    eff = np.full(len(A.x), -7, dtype=np.int32)
    assert L.sc_value_entries(symb.h, None, None, eff.ctypes.data_as(ctypes.c_void_p)) == len(A.x)
    assert np.array_equal(eff.astype(bool), gc.classify(6, A.p, A.i)[2])
    assert L.sc_value_entries(None, None, None, None) == -1
    assert b"sc_value_entries" in L.sc_last_error()


def test_symbols_and_methods_exist():
    so = ctypes.CDLL(sc.LIB_PATH)
    for name in ENTRY:
        assert name in sc.exported_symbols() and hasattr(so, name), name
    for meth in ("logdet_grad", "pattern_outer", "pattern_dot", "solve_grad", "logdet_grad_device",
                 "pattern_outer_device", "pattern_dot_device", "solve_grad_device"):
        assert callable(getattr(sc.Numeric, meth))
    assert callable(sc.Symbolic.value_entries)
    assert sc.lib().sc_version() == 121


def test_the_package_imports_without_torch_and_the_torch_layer_is_a_module_of_its_own():
    # the test is about a fresh interpreter in which torch cannot be imported
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparsecholesky_amd as sc\n"
            "sc.lib()\n"
            "assert 'sparsecholesky_amd.autograd' not in sys.modules\n"
            "assert callable(sc.Numeric.logdet_grad)\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)
    assert os.path.exists(os.path.join(root, "sparsecholesky_amd", "autograd.py"))
