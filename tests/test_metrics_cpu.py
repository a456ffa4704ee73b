"""CPU-side checks of the pointwise-metrics surface (fmx_metrics / fmx_metrics_device, fmwr_amd.fm_metrics): the numpy model of the definition
(tests/metrics_model.py) against a brute-force loop over all (positive, negative) pairs and against the identities of the AUC; why the call
exists (the reference's AUC scores an inverted ranking as perfect); the declared surface; the argument checks, which run before any device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import oracle
from tests import metrics_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_metrics", "fmx_metrics_device")


def _cmp2(a, b):
    """2 [a > b] + [a == b] under the ranking order, written out case by case: NaN below every number and equal to NaN, -0 == +0"""
    an, bn = math.isnan(a), math.isnan(b)
    if an or bn:
        return 1 if (an and bn) else (0 if an else 2)
    return 2 if a > b else (1 if a == b else 0)


def _brute_pairs2(z, y):
    return sum(_cmp2(float(z[i]), float(z[j])) for i in range(len(z)) if y[i] > 0 for j in range(len(z)) if not y[j] > 0)


def test_model_matches_the_double_loop_on_heavy_ties_and_edge_scores():
    rng = np.random.default_rng(5)
    n, G = 200, 7
    z = rng.choice([-1.5, -0.25, 0.5, 0.75, 2.0], n)
    z[rng.choice(n, 40, replace=False)] = rng.choice([0.0, -0.0, np.inf, -np.inf, np.nan], 40)
    assert all(np.any(mm.bits(z) == b) for b in mm.bits([0.0, -0.0, np.inf, -np.inf])) and np.isnan(z).any()
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    g = rng.integers(0, G, n)
    p = 1.0 / (1.0 + np.exp(-z))
    count, value, _ = mm.metrics(z, p, y, g, G, True, mm.LINK_LOGISTIC)
    for q in range(G):
        rows = np.flatnonzero(g == q)
        P = int((y[rows] > 0).sum())
        ref = _brute_pairs2(z[rows], y[rows])
        assert count[q][:3] == [len(rows), P, ref]
        assert 0 <= ref <= 2 * P * (len(rows) - P)
        assert 0 < P < len(rows)
        assert value[q][0] == ref / 2 / (P * (len(rows) - P))   # halving is exact: one rounding either way
        assert count[q][3] == sum(1 for r in rows if not math.isnan(p[r]) and ((p[r] >= 0.5) == (y[r] > 0)))
    pooled = mm.metrics(z, p, y, None, 1, True, mm.LINK_LOGISTIC)[0][0]
    assert pooled[2] == _brute_pairs2(z, y) and pooled[0] == n


def test_auc_of_negated_scores_is_one_minus_auc():
    """tie-free, NaN-free: every pair flips, pairs2(-z) = 2 P N - pairs2(z).  With P N = 256 both quotients and the subtraction are exact in
    fp64, so the identity of the AUCs holds in every bit (for a general P N the two sides may differ by one rounding)."""
    rng = np.random.default_rng(11)
    z = rng.permutation(32).astype(np.float64) - 15.5
    pos = np.arange(32) < 16
    rng.shuffle(pos)
    a, b = mm.pairs2(z, pos), mm.pairs2(-z, pos)
    assert a + b == 2 * 256 and 0 < a < 512
    assert mm.auc_from(b, 16, 16) == 1.0 - mm.auc_from(a, 16, 16)


def test_pairs_are_invariant_under_increasing_maps():
    rng = np.random.default_rng(12)
    z = np.round(rng.normal(0, 1, 300), 1)   # ties
    pos = rng.random(300) < 0.3
    ref = mm.pairs2(z, pos)
    for f in (lambda t: 3.0 * t + 1.0, np.exp, lambda t: t ** 3, lambda t: 1.0 / (1.0 + np.exp(-t))):
        assert mm.pairs2(f(z), pos) == ref


def test_all_equal_scores_give_p_times_n():
    pos = np.arange(50) % 3 == 0
    for s in (0.25, 0.0, np.nan, np.inf):
        assert mm.pairs2(np.full(50, s), pos) == int(pos.sum()) * int((~pos).sum())
    assert mm.pairs2(np.where(np.arange(50) % 2 == 0, 0.0, -0.0), pos) == int(pos.sum()) * int((~pos).sum())   # -0 == +0


def test_inverted_ranking_scores_zero_here_and_one_in_the_reference():
    """the reason for this call: the reference's AUC (core/Evaluation.h, reproduced by the oracle and by fmx_evaluate) returns max(a, 1 - a)"""
    y = np.where(np.arange(40) < 15, 1.0, -1.0)
    z = np.where(y > 0, -1.0, 1.0) + np.linspace(-0.2, 0.2, 40)   # every positive below every negative
    p = 1.0 / (1.0 + np.exp(-z))
    _, value, _ = mm.metrics(z, p, y, None, 1, True, mm.LINK_LOGISTIC)
    assert value[0][0] == 0.0
    assert oracle.evaluate(oracle.CLASSIFICATION, oracle.AUC, p, y) == 1.0
    _, value, _ = mm.metrics(-z, 1.0 - p, y, None, 1, True, mm.LINK_LOGISTIC)
    assert value[0][0] == 1.0


def test_planted_gauc_is_one_half_under_a_high_pooled_auc():
    z, y, user = mm.planted_gauc(np.random.default_rng(3))
    p = 1.0 / (1.0 + np.exp(-z))
    count, value, _ = mm.metrics(z, p, y, user, 40, True, mm.LINK_LOGISTIC)
    assert np.all(value[:, 0] == 0.5)
    rows = np.array([c[0] for c in count], np.float64)
    assert math.fsum(value[:, 0] * rows) / rows.sum() == 0.5
    pooled = mm.metrics(z, p, y, None, 1, True, mm.LINK_LOGISTIC)[1][0][0]
    assert pooled > 0.75
    assert abs(pooled - mm.rank_sum_auc(z, y > 0)) < 1e-12


def test_regression_values_and_empty_groups():
    rng = np.random.default_rng(8)
    p, y = rng.normal(0, 1, 30), rng.normal(0, 1, 30).astype(np.float32).astype(np.float64)
    count, value, ab = mm.metrics(p, p, y, np.repeat([0, 2], 15), 3, False, mm.LINK_NONE)
    assert count[1] == [0, 0, 0, 0] and np.isnan(value[1]).all()
    assert count[0] == [15, 0, 0, 0]
    d = p[:15] - y[:15]
    tol = 15 * 2.0 ** -53 * float(np.sum(d * d) + np.sum(np.abs(d)))   # numpy's own mean: a plain sum of 15 terms
    assert abs(value[0][0] - np.mean(d * d)) <= tol and abs(value[0][2] - np.mean(np.abs(d))) <= tol and abs(value[0][3] - np.mean(d)) <= tol
    assert ab[0][2] == math.fsum(np.abs(d))


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_metrics_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_metrics_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_metrics_limits")
    assert "fmx_debug_metrics_limits" not in text   # the hook stays out of the public header
    for name, value in (("VALUES", 6), ("COUNTS", 4), ("AUC", 0), ("LOGLOSS", 1), ("ACCURACY", 2), ("BRIER", 3), ("MEAN_PRED", 4), ("MEAN_LABEL", 5),
                        ("MSE", 0), ("RMSE", 1), ("MAE", 2), ("MEAN_ERR", 3), ("ROWS", 0), ("POSITIVES", 1), ("PAIRS2", 2), ("CORRECT", 3)):
        assert re.search(r"#define\s+FMX_MET_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(L, "MET_" + name) == value
    assert len(mm.CLS_NAMES) == len(mm.REG_NAMES) == L.MET_VALUES
    assert "fmx_metrics" in text[text.index("int fmx_evaluate(") - 600:text.index("int fmx_evaluate(")]   # fmx_evaluate points here
    import fmwr_amd as fm
    assert callable(fm.fm_metrics)
    for method in ("metrics", "metrics_device"):
        assert callable(getattr(fm.Engine, method))


def test_metrics_without_an_engine_are_an_error_not_a_computation():
    L = _lib()
    out = np.full(12, 7.0)
    cnt = np.full(8, 7, np.int64)
    po, pc = out.ctypes.data_as(C.c_void_p), cnt.ctypes.data_as(C.c_void_p)
    assert L.lib().fmx_metrics(None, None, None, 1, L.LINK_LOGISTIC, po, pc) == L.ERR_INVALID
    assert L.lib().fmx_last_error().decode()
    assert L.lib().fmx_metrics_device(None, None, 0, 1, None, 1, L.LINK_LOGISTIC, po, pc) == L.ERR_INVALID
    assert np.all(out == 7.0) and np.all(cnt == 7)  # nothing written


def _fit(p, task="CLASSIFICATION", k=3):
    """a fitted-model object as fm_train returns it, without training (the checks below never reach a device)"""
    import fmwr_amd as fm
    rng = np.random.default_rng(0)
    ctl = {"model": fm.model_control(task, **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    return {"Model": {"w0": 0.1, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"], "solver.control": ctl["solver"],
                      "track.control": ctl["track"]},
            "Scales": {"mean": None, "std": None, "target.range": (-1.0, 1.0)}}


def _data(n, p, seed, labels="01"):
    import fmwr_amd as fm
    y = None if labels is None else (np.arange(n) % 2).astype(np.float64) if labels == "01" else np.asarray(labels, np.float64)
    return fm.fm_matrix(np.random.default_rng(seed).random((n, p)), y)


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    monkeypatch.setattr(api, "_engine_for", lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api, "_device_matrix", lambda *a, **k: pytest.fail("a device was touched"))


def test_fm_metrics_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_metrics(_fit(6), np.ones((4, 6)), normalize=False)
    rank = _fit(6)
    rank["Model"]["model.control"] = dict(rank["Model"]["model.control"], task="RANK")
    with pytest.raises(ValueError, match="CLASSIFICATION and REGRESSION"):
        fm.fm_metrics(rank, _data(4, 6, 1), normalize=False)
    with pytest.raises(ValueError, match="no labels"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1, labels=None), normalize=False)
    d = _data(4, 6, 1)
    d.features["value"][2] = np.nan
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_metrics(_fit(6), d, normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_metrics(_fit(6), _data(4, 7, 1), normalize=False)
    with pytest.raises(ValueError, match="normalize"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1), normalize=True)
    with pytest.raises(ValueError, match="one integer group id per row"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1), groups=[0, 1, 2], normalize=False)
    with pytest.raises(ValueError, match="one integer group id per row"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1), groups=np.zeros(4), normalize=False)
    with pytest.raises(ValueError, match="two levels"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1, labels=[0, 1, 2, 1]), normalize=False)
    with pytest.raises(ValueError, match=r"c\(0, 1\) or c\(-1, 1\)"):
        fm.fm_metrics(_fit(6), _data(4, 6, 1, labels=[1, 2, 2, 1]), normalize=False)
