"""CPU-side checks of fold-in: the numpy model of tests/foldin_model.py against the oracle's forward (the gradient of the full objective
vanishes at the solved rows), the model's own fp64 spread on exactly the GPU test's inputs, and the declared surface."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests import foldin_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(line):
    """printed (pytest -s) and, with FMX_FOLDIN_REPORT set to a path, appended to that file (profiles/foldin.txt quotes such a run)"""
    print(line)
    path = os.environ.get("FMX_FOLDIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _oracle_raw(inp, k, w0, w, v, k0=1, k1=1):
    P = oracle.params(task=oracle.REGRESSION, k=k, k0=bool(k0), k1=bool(k1))
    return oracle.predict_batch(P, oracle.Matrix(inp["rp"], inp["col"], inp["val"], inp["p"]), w0, w, v.ravel())


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", M.KS)
@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
def test_gradient_of_the_full_objective_vanishes_at_the_solved_rows(loss, k, valued):
    inp = M.inputs(valued)
    ids = inp["ids"]
    w0, w, v = M.model_params(inp["p"], k)
    y = M.targets(valued, k, loss)
    theta, rows, status = M.fold_in(inp["rp"], inp["col"], inp["val"], y, ids, w0, w, v, 0.1, 0.1, loss=loss)
    assert np.array_equal(rows, inp["sizes"]) and not status.any()
    assert np.all(theta[list(inp["sizes"]).index(0)] == 0)          # no rows, positive lambdas: theta = 0 falls out of the solve
    w2, v2 = w.copy(), v.copy()
    w2[ids] = theta[:, 0]
    v2[:, ids] = theta[:, 1:].T
    g = M.gradient(inp["rp"], inp["col"], inp["val"], y, ids, theta, _oracle_raw(inp, k, w0, w2, v2), w0, w, v, 0.1, 0.1, loss=loss)
    _record(f"fold-in model {loss} k={k} valued={valued}: gradient {g:.3g}")
    assert g <= 1e-10


@pytest.mark.parametrize("form", [dict(k0=0), dict(k1=0), dict(lw=0.03, lv=0.7)])
def test_gradient_with_keep_flags_and_unequal_lambdas(form):
    inp = M.inputs(True)
    ids, k = inp["ids"], 16
    w0, w, v = M.model_params(inp["p"], k)
    y = M.targets(True, k, M.SQUARED)
    lw, lv, k0, k1 = form.get("lw", 0.1), form.get("lv", 0.1), form.get("k0", 1), form.get("k1", 1)
    theta, _, status = M.fold_in(inp["rp"], inp["col"], inp["val"], y, ids, w0, w, v, lw, lv, k0, k1)
    assert not status.any() and (k1 or np.all(theta[:, 0] == 0))
    w2, v2 = w.copy(), v.copy()
    w2[ids] = theta[:, 0]
    v2[:, ids] = theta[:, 1:].T
    g = M.gradient(inp["rp"], inp["col"], inp["val"], y, ids, theta, _oracle_raw(inp, k, w0, w2, v2, k0, k1), w0, w, v, lw, lv, k0, k1)
    assert g <= 1e-10


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", M.KS)
@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
def test_spread_of_the_fp64_model(loss, k, valued):
    """the float64 model on permuted rows against the longdouble model, relative to a feature's max |theta|: what the GPU test's bar of 1e-11
    presupposes (<= 1e-13)"""
    s = M.spread(valued, k, loss)
    _record(f"fold-in model {loss} k={k} valued={valued}: fp64 spread {s:.3g}")
    assert s <= 1e-13


def test_first_newton_step_is_the_first_of_eight():
    inp = M.inputs(True)
    w0, w, v = M.model_params(inp["p"], 16)
    y = M.targets(True, 16, M.LOGISTIC)
    rows, grp, b, z = M.rows_of(inp["rp"], inp["col"], inp["val"], inp["ids"], w0, w, v, 1, 1, np.float64)
    R = np.flatnonzero(grp == 7)
    steps = []
    M.solve_group(z[R], b[R], y[rows[R]], 0.1, 0.1, 1, M.LOGISTIC, 8, np.float64, steps)
    one = M.solve_group(z[R], b[R], y[rows[R]], 0.1, 0.1, 1, M.LOGISTIC, 1, np.float64)
    assert len(steps) == 8 and np.array_equal(steps[0], one) and np.max(np.abs(steps[7] - steps[6])) < 1e-9 * np.max(np.abs(steps[7]))


def test_failed_pivot_and_two_fold_entries():
    inp = M.inputs(False)
    w0, w, v = M.model_params(inp["p"], 16)
    y = M.targets(False, 16, M.SQUARED)
    theta, rows, status = M.fold_in(inp["rp"], inp["col"], inp["val"], y, inp["ids"], w0, w, v, 0.0, 0.0)
    sizes = list(inp["sizes"])
    assert status[sizes.index(0)] == 1 and status[sizes.index(1)] == 1 and np.all(np.isnan(theta[sizes.index(0)]))
    assert status[sizes.index(257)] == 0 and status[sizes.index(5000)] == 0
    col = inp["col"].copy()
    four = np.flatnonzero(np.diff(inp["rp"]) == 4)[0]
    col[inp["rp"][four]] = inp["ids"][2]                          # its item entry becomes a second fold entry
    with pytest.raises(ValueError):
        M.fold_in(inp["rp"], col, inp["val"], y, inp["ids"], w0, w, v, 0.1, 0.1)


def test_surface_is_declared_bound_and_refuses_null_handles():
    from fmwr_amd import _lib as L
    import fmwr_amd
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert re.search(r"\bint fmx_fold_in\(fmx_engine\* e, const fmx_matrix\* m, const uint32_t\* ids, int64_t n_ids,", header)
    assert "fmx_fold_in" in L.SYMBOLS and "fmx_debug_foldin_slab" in L.TEST_HOOKS
    assert "fmx_debug_foldin_slab" not in header
    assert callable(fmwr_amd.fm_fold_in) and hasattr(fmwr_amd.engine.Engine, "fold_in")
    ids = np.zeros(1, np.uint32)
    assert L.lib().fmx_fold_in(None, None, ids.ctypes.data_as(C.c_void_p), 1, 0.1, 0.1, 8, 0, None, None, None, None) == L.ERR_INVALID
    with pytest.raises(TypeError):
        fmwr_amd.fm_fold_in({"class": "other"}, None, [0])
    src = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fm_foldin.hip")).read()
    assert re.search(r"FI_CHUNK = (\d+);", src).group(1) == str(M.ROW_CHUNK)   # the test's group sizes straddle the kernel's row chunk
