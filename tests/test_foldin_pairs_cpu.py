"""CPU-side checks of the pairwise fold-in: the numpy model of tests/foldin_pairs_model.py against the oracle's forward (the gradient of the
full pairwise objective vanishes at the solved rows), the model's own fp64 spread on exactly the GPU test's inputs, the exact zero of a new
user's w, the declared surface, and the cold-start numbers the end-to-end GPU test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests import foldin_model as M
from tests import foldin_pairs_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(line):
    """printed (pytest -s) and, with FMX_FOLDIN_REPORT set to a path, appended to that file (profiles/foldin_pairs.txt quotes such a run)"""
    print(line)
    path = os.environ.get("FMX_FOLDIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _oracle_raw(inp, k, w0, w, v):
    par = oracle.params(task=oracle.REGRESSION, k=k)
    return oracle.predict_batch(par, oracle.Matrix(inp["rp"], inp["col"], inp["val"], inp["p"]), w0, w, v.ravel())


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", [0, 2, 16, 64])
def test_gradient_of_the_pairwise_objective_vanishes_at_the_solved_rows(k, valued):
    inp = P.inputs(valued, k)
    ids = inp["ids"]
    w0, w, v = M.model_params(inp["p"], k)
    lam = P.case_lambda(k, valued)
    theta, pairs, status = P.fold_in_pairs(inp["rp"], inp["col"], inp["val"], ids, w, v, lam, lam)
    assert np.array_equal(pairs, inp["sizes"]) and not status.any()
    assert np.all(theta[list(inp["sizes"]).index(0)] == 0)          # no pairs, positive lambdas: theta = 0 falls out of the solve
    w2, v2 = w.copy(), v.copy()
    w2[ids] = theta[:, 0]
    v2[:, ids] = theta[:, 1:].T
    g = P.gradient(inp["rp"], inp["col"], inp["val"], ids, theta, _oracle_raw(inp, k, w0, w2, v2), w, v, lam, lam)
    _record(f"pair fold-in model k={k} valued={valued} lambda={lam}: gradient {g:.3g}")
    assert g <= 1e-10


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", P.KS)
def test_spread_of_the_fp64_model(k, valued):
    """the float64 model on permuted pairs against the longdouble model, relative to a feature's max |theta|: what the GPU test's bar of
    1e-11 presupposes (<= 1e-13), for every (k, valued) case of the GPU test under foldin_pairs_model.case_lambda"""
    s = P.spread(valued, k)
    _record(f"pair fold-in model k={k} valued={valued} lambda={P.case_lambda(k, valued)}: fp64 spread {s:.3g}")
    assert s <= 1e-13


def test_every_form_of_pair_is_present_and_groups_alternate():
    for valued in (False, True):
        inp = P.inputs(valued, 16)
        forms, grp = inp["forms"], inp["pair_group"]
        assert set(forms) == ({"V", "P", "N", "-"} if valued else {"U", "P", "N", "-"}) and np.sum(forms == "-") == 100
        for g in range(len(inp["sizes"])):
            assert set(forms[grp == g]) <= ({"V", "U"} if P.user_like(g) else {"P", "N"})
        big = np.flatnonzero(inp["sizes"] >= 63)
        assert all(set(forms[grp == g]) == {"P", "N"} for g in big if not P.user_like(g))   # item-like groups mix both orientations


def test_w_of_a_new_user_is_exactly_zero_and_needs_a_positive_lambda_w():
    k = 16
    inp = P.inputs(False, k)
    _, w, v = M.model_params(inp["p"], k)
    users = np.array([g for g in range(len(inp["sizes"])) if P.user_like(g)])
    theta, pairs, status = P.fold_in_pairs(inp["rp"], inp["col"], inp["val"], inp["ids"], w, v, 0.1, 0.1)
    assert not status.any() and np.all(theta[users, 0] == 0.0)
    assert np.any(theta[np.setdiff1d(np.arange(len(inp["sizes"])), users), 0] != 0.0)
    theta, pairs, status = P.fold_in_pairs(inp["rp"], inp["col"], inp["val"], inp["ids"], w, v, 0.0, 0.1)
    assert np.all(status[users] == 1) and np.all(np.isnan(theta[users]))                   # the first pivot is exactly 0
    theta, pairs, status = P.fold_in_pairs(inp["rp"], inp["col"], inp["val"], inp["ids"], w, v, 0.0, 0.1, k1=0)
    assert not status.any() and np.all(theta[:, 0] == 0.0)                                   # keep_w1 = 0: w_u is not a variable


def test_pairs_of_two_groups_and_rows_of_two_entries_are_refused():
    inp = P.inputs(False, 2)
    _, w, v = M.model_params(inp["p"], 2)
    col = inp["col"].copy()
    t = int(np.flatnonzero(inp["forms"] == "U")[0])
    a = inp["rp"][2 * t]
    at = a + int(np.flatnonzero(col[a:inp["rp"][2 * t + 1]] >= P.N_ITEMS + P.N_SIDE)[0])
    col[at] = inp["ids"][1] if col[at] != inp["ids"][1] else inp["ids"][3]
    with pytest.raises(ValueError, match="different fold features"):
        P.fold_in_pairs(inp["rp"], col, inp["val"], inp["ids"], w, v, 0.1, 0.1)
    col = inp["col"].copy()
    a = inp["rp"][2 * t]
    col[a:a + 4] = np.where(col[a:a + 4] < P.N_ITEMS, inp["ids"][5], col[a:a + 4])   # its item entry becomes a second fold entry
    with pytest.raises(ValueError, match="more than one entry"):
        P.fold_in_pairs(inp["rp"], col, inp["val"], inp["ids"], w, v, 0.1, 0.1)


def test_surface_is_declared_bound_and_refuses_null_handles():
    from fmwr_amd import _lib as L
    import fmwr_amd
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    assert re.search(r"\bint fmx_fold_in_pairs\(fmx_engine\* e, const fmx_matrix\* m, const uint32_t\* ids, int64_t n_ids,", header)
    assert "lambda_w > 0 OR keep_w1 = 0" in header
    assert "fmx_fold_in_pairs" in L.SYMBOLS
    assert callable(fmwr_amd.fm_fold_in_rank) and hasattr(fmwr_amd.engine.Engine, "fold_in_pairs")
    ids = np.zeros(1, np.uint32)
    assert L.lib().fmx_fold_in_pairs(None, None, ids.ctypes.data_as(C.c_void_p), 1, 0.1, 0.1, 8, 0, None, None, None, None) == L.ERR_INVALID
    with pytest.raises(TypeError):
        fmwr_amd.fm_fold_in_rank({"class": "other"}, None, None, None, [0])


@pytest.mark.parametrize("seed", range(5))
def test_cold_start_fold_in_lifts_the_held_out_auc(seed):
    """The planted problem of the end-to-end GPU test, all in the numpy model: held-out AUC (training positives excluded) of 40 new users
    with zero rows against the same users folded in from 12 positives x 4 sampled negatives, lambda = 0.1, eight steps."""
    cs = P.cold_start(seed)
    rp, col, val = P.cold_start_pairs(cs, seed)
    ids = np.arange(P.CS_ITEMS, cs["p"], dtype=np.uint32)
    theta, pairs, status = P.fold_in_pairs(rp, col, val, ids, cs["w"], cs["v"], 0.1, 0.1)
    assert not status.any() and np.all(pairs == P.CS_TRAIN * P.CS_NEG) and np.all(theta[:, 0] == 0.0)
    w2, v2 = cs["w"].copy(), cs["v"].copy()
    v2[:, ids] = theta[:, 1:].T
    before, after = P.cold_start_auc(cs, cs["w"], cs["v"]), P.cold_start_auc(cs, w2, v2)
    _record(f"pair fold-in cold start seed={seed}: held-out AUC unfolded {before:.3f}, folded {after:.3f}")
    assert after >= before + 0.10
