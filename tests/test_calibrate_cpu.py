"""The calibration calls without a GPU: the numpy model (tests/calibrate_model.py) against brute force -- the bins by a Python-integer loop, the
pooling by the min-max formula in fractions, the Platt fit in fp64 under permuted orders against long double --, the planted problem, and the
declared surface with its refusals."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import calibrate_model as cm

GPU_AB_BAR = 1e-11   # tests/test_gpu_calibrate.py holds (a, b) to this share of max(|a|, |b|) of the long double model


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


def _edge_rows(rng, n=200, G=7):
    pool = np.array([-np.inf, -2.0, -0.0, 0.0, 0.5, 0.5, 1.25, np.inf, np.nan, 3.0])
    z = rng.choice(pool, n)
    g = rng.integers(0, G, n)
    g[g == 5] = 4                      # group 5 stays empty
    z[g == 6] = np.nan                 # group 6 holds NaN rows only
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
    with np.errstate(all="ignore"):
        p = 1.0 / (1.0 + np.exp(-z))
    return z, p, y, g


def _key_less(a, b):
    """a < b under the ranking order's key, in plain Python"""
    a, b = (0.0 if a == 0 else a), (0.0 if b == 0 else b)
    return a < b


@pytest.mark.parametrize("B", [1, 2, 10, 64, 1024])
def test_bins_against_a_brute_force_loop(B):
    rng = np.random.default_rng(B)
    z, p, y, g = _edge_rows(rng)
    G = 7
    for binning in (cm.BINS_WIDTH, cm.BINS_MASS):
        t = cm.table(z, p, y, g, G, B, binning)
        for q in range(G):
            rows = [r for r in range(len(z)) if g[r] == q]
            valid = [r for r in rows if not math.isnan(z[r])]
            assert t["nan_rows"][q] == len(rows) - len(valid) and t["s"][q] == len(valid)
            s = len(valid)
            count = [[0, 0] for _ in range(B)]
            for r in valid:
                if binning == cm.BINS_WIDTH:
                    b = min(B - 1, int(math.floor(float(p[r]) * float(B))))
                else:
                    head = sum(1 for r2 in valid if _key_less(float(z[r2]), float(z[r])))   # the rows strictly below = the run's first position
                    b = head * B // s
                assert t["bin"][r] == b, (binning, q, r)
                count[b][0] += 1
                count[b][1] += int(y[r] > 0)
            assert t["count"][q] == count
            for b in range(B):
                sel = [r for r in valid if t["bin"][r] == b]
                if not sel:
                    assert math.isnan(t["lo_z"][q, b]) and math.isnan(t["hi_z"][q, b])
                    continue
                assert min(z[sel]) == t["lo_z"][q, b] and max(z[sel]) == t["hi_z"][q, b]
                if 0.0 in z[sel] and any(math.copysign(1, v) < 0 and v == 0 for v in z[sel]):   # both zeros: -0 is the smaller
                    if t["lo_z"][q, b] == 0:
                        assert math.copysign(1, t["lo_z"][q, b]) < 0
                    if t["hi_z"][q, b] == 0:
                        assert math.copysign(1, t["hi_z"][q, b]) > 0
        assert t["count"][5] == [[0, 0]] * B and t["s"][6] == 0 and t["nan_rows"][6] > 0


def test_mass_bin_properties():
    rng = np.random.default_rng(3)
    for s, B in ((1, 1), (7, 3), (40, 10), (40, 64), (200, 10), (200, 1024), (33, 33)):
        z = rng.choice(np.concatenate([rng.normal(0, 1, 12), [-0.0, 0.0, np.inf, -np.inf]]), s)
        b = cm.mass_bins(z, B)
        k = cm.order_key(z)
        assert b.min() >= 0 and b.max() < B
        for key in np.unique(k):
            assert len(set(b[k == key])) == 1                    # equal scores share a bin
        order = np.argsort(k, kind="stable")
        assert np.all(np.diff(b[order]) >= 0)                    # non-decreasing in z
        if B >= s:
            first = [b[k == key][0] for key in np.unique(k)]
            assert len(set(first)) == len(first)                 # every run has a bin of its own
    assert cm.mass_bins(np.array([-0.0, 0.0, 1.0]), 3).tolist() == [0, 0, 2]


def _minmax_isotonic(pos, rows):
    """the isotonic regression of the bins' rates under the weights `rows`, by the min-max formula in exact fractions: fit_i = max over a <= i
    of min over c >= i of mean(a .. c)"""
    n = len(pos)
    fit = []
    for i in range(n):
        best = None
        for a in range(i + 1):
            low = min(Fraction(sum(pos[a:c + 1]), sum(rows[a:c + 1])) for c in range(i, n))
            best = low if best is None or low > best else best
        fit.append(best)
    return fit


def test_pooling_against_the_min_max_formula():
    rng = np.random.default_rng(11)
    for trial in range(60):
        B = int(rng.integers(1, 14))
        rows = rng.integers(0, 6, B)
        if trial % 7 == 0:
            rows[:] = 0
        pos = np.array([rng.integers(0, r + 1) for r in rows])
        lo = np.arange(B, dtype=np.float64) + 0.5
        ns, thr, val = cm.pav([[int(r), int(p)] for r, p in zip(rows, pos)], lo)
        nz = [b for b in range(B) if rows[b] > 0]
        fit = _minmax_isotonic([int(pos[b]) for b in nz], [int(rows[b]) for b in nz]) if nz else []
        assert ns == len(set(fit))
        assert np.isnan(thr[ns:]).all() and np.isnan(val[ns:]).all()
        if ns:
            assert thr[0] == -math.inf
            assert all(val[t] < val[t + 1] for t in range(ns - 1))     # block values rise strictly
            assert all(thr[t] < thr[t + 1] for t in range(ns - 1))
        for i, b in enumerate(nz):                                      # the step that bin b's rows fall into holds the bin's fitted value
            step = int(np.searchsorted(thr[:ns], lo[b], "right")) - 1
            assert val[step] == float(fit[i].numerator) / float(fit[i].denominator)


def test_platt_model_orders_against_long_double():
    rng = np.random.default_rng(5)
    worst = 0.0
    for name, w, cols, y, lam in cm.platt_cases():
        z = w[cols]
        ref = cm.platt(z, y, lam, 8)
        assert ref[3] == 0 and ref[2] == len(z), name
        scale = max(abs(float(ref[0])), abs(float(ref[1])))
        for trial in range(4):
            order = None if trial == 0 else rng.permutation(len(z))
            a, b, rows, status = cm.platt(z, y, lam, 8, np.float64, order)
            assert status == 0
            spread = max(abs(float(a) - float(ref[0])), abs(float(b) - float(ref[1]))) / scale
            worst = max(worst, spread)
            assert spread <= GPU_AB_BAR / 10, (name, trial, spread)
    print("largest spread of the fp64 model against long double:", worst)
    a, _, _, status = cm.platt(np.linspace(-6.0, 8.0, 40), np.ones(40), 0.1, 8)
    assert status == 0 and abs(float(a)) > 100    # a one-class group: status 0, and the undamped steps have run away
    assert cm.platt(np.array([np.inf, np.nan]), np.ones(2), 0.0, 3)[2:] == (0, 1)
    a, b, rows, status = cm.platt(np.array([np.nan]), np.ones(1), 0.1, 3)
    assert (float(a), float(b), rows, status) == (1.0, 0.0, 0, 0)


def _ece10(z, p, y):
    t = cm.table(z, p, y, None, 1, 10, cm.BINS_WIDTH)
    return cm.ece_mce(t["count"][0], t["sum_p"][0])[0]


def test_planted_problem_platt_isotonic_and_prior_correction():
    from fmwr_amd import api
    rng = np.random.default_rng(1)
    z, y = cm.planted(rng)
    fit_rows, test_rows = np.arange(0, 5000, 2), np.arange(1, 5000, 2)
    p0 = cm.apply_map(None, z, p_link=1.0 / (1.0 + np.exp(-z)))
    before = _ece10(z[test_rows], p0[test_rows], y[test_rows])
    a, b, _, status = cm.platt(z[fit_rows], y[fit_rows], 0.1, 8, np.float64)
    assert status == 0 and abs(float(a) - 0.5) < 0.15 and abs(float(b) + 0.5) < 0.2
    p1 = cm.apply_map({"kind": "platt", "ab": [[float(a), float(b)]]}, z)
    after = _ece10(z[test_rows], p1[test_rows], y[test_rows])
    print("ECE at 10 width bins:", before, "->", after, "(Platt)")
    assert before > 0.08 and after < before / 2
    t = cm.table(z[fit_rows], p0[fit_rows], y[fit_rows], None, 1, 64, cm.BINS_MASS)
    ns, thr, val = cm.pav(t["count"][0], t["lo_z"][0])
    p2 = cm.apply_map({"kind": "steps", "n_steps": [ns], "thr": thr[None], "val": val[None]}, z)
    iso = _ece10(z[test_rows], p2[test_rows], y[test_rows])
    print("... ->", iso, "(isotonic, 64 bins)")
    assert iso < before
    # a model that is right on a set whose negatives were kept with probability r is right on the full set after the correction
    r = 0.1
    zt = rng.normal(-3.0, 1.0, 40000)
    yf = rng.random(40000) < 1.0 / (1.0 + np.exp(-zt))
    cal = api.fm_prior_correction(r)
    assert cal["map"]["ab"].tolist() == [[1.0, math.log(r)]] and cal["groups"] is None
    pc = cm.apply_map(cal["map"], zt - math.log(r))
    assert abs(pc.mean() - yf.mean()) < 4 * math.sqrt(yf.mean() / 40000)
    assert abs((1.0 / (1.0 + np.exp(-(zt - math.log(r))))).mean() - yf.mean()) > 0.1     # ... and is far off before it
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            api.fm_prior_correction(bad)


CALLS = ["fmx_predict_calibrated", "fmx_predict_calibrated_device", "fmx_reliability", "fmx_reliability_device", "fmx_calibrate_platt",
         "fmx_calibrate_platt_device", "fmx_calibrate_isotonic", "fmx_calibrate_isotonic_device"]


def test_declared_surface_and_null_engine_calls():
    L = _lib()
    lib = L.lib()
    assert set(CALLS) <= set(L.SYMBOLS) and "fmx_debug_calibrate_limits" in L.TEST_HOOKS and "fmx_debug_calibrate_limits" not in L.SYMBOLS
    for s in CALLS + ["fmx_debug_calibrate_limits"]:
        assert hasattr(lib, s), s
    assert C.sizeof(L.Calibrator) == 56
    assert (L.CAL_NONE, L.CAL_PLATT, L.CAL_STEPS, L.BINS_WIDTH, L.BINS_MASS, L.CAL_VALUES) == (0, 1, 2, 0, 1, 4)
    out = np.full(4, 7.0)
    o = out.ctypes.data_as(C.c_void_p)
    assert lib.fmx_predict_calibrated(None, None, None, 1, None, L.LINK_LOGISTIC, o) == L.ERR_INVALID
    assert lib.fmx_predict_calibrated_device(None, None, 0, 0, None, 1, None, L.LINK_LOGISTIC, o) == L.ERR_INVALID
    assert lib.fmx_reliability(None, None, None, 1, 10, L.BINS_WIDTH, None, L.LINK_LOGISTIC, o, o, o, o, o, o) == L.ERR_INVALID
    assert lib.fmx_reliability_device(None, None, 0, 0, None, 1, 10, L.BINS_WIDTH, None, L.LINK_LOGISTIC, o, o, o, o, o, o) == L.ERR_INVALID
    assert lib.fmx_calibrate_platt(None, None, None, 1, 0.1, 8, o, o, o) == L.ERR_INVALID
    assert lib.fmx_calibrate_platt_device(None, None, 0, 0, None, 1, 0.1, 8, o, o, o) == L.ERR_INVALID
    assert lib.fmx_calibrate_isotonic(None, None, None, 1, 10, o, o, o) == L.ERR_INVALID
    assert lib.fmx_calibrate_isotonic_device(None, None, 0, 0, None, 1, 10, o, o, o) == L.ERR_INVALID
    assert lib.fmx_last_error() and (out == 7.0).all()
    assert lib.fmx_debug_calibrate_limits(16) == L.OK and lib.fmx_debug_calibrate_limits(0) == L.OK


def test_python_refusals_before_any_device():
    import scipy.sparse as sp

    import fmwr_amd
    from fmwr_amd import api, engine
    for name in ("fm_reliability", "fm_calibrate", "fm_prior_correction", "fm_predict_calibrated"):
        assert hasattr(fmwr_amd, name)
    for name in ("reliability", "calibrate_platt", "calibrate_isotonic", "predict_calibrated"):
        assert hasattr(engine.Engine, name) and hasattr(engine.Engine, name + "_device")
    data = api.fm_matrix(sp.csr_matrix(np.eye(4)), labels=[0, 1, 1, 0])
    nolab = api.fm_matrix(sp.csr_matrix(np.eye(4)))

    def model(task, p=4):
        return {"class": "FM", "Model": {"model.control": {"task": task}, "solver.control": {"solver": {"solver": "SGD"}}, "track.control": None,
                                         "w0": 0.0, "w": np.zeros(p), "v": np.zeros((2, p))}, "Scales": {"mean": None, "std": None, "target.range": None}}
    fm = model("CLASSIFICATION")
    cal = api.fm_prior_correction(0.5)
    with pytest.raises(TypeError):
        api.fm_reliability({"class": "other"}, data)
    with pytest.raises(TypeError):
        api.fm_reliability(fm, np.eye(4))
    with pytest.raises(TypeError):
        api.fm_reliability(fm, data, calibration={"ab": 1})
    with pytest.raises(TypeError):
        api.fm_predict_calibrated(fm, data, None)
    with pytest.raises(ValueError, match="binning"):
        api.fm_reliability(fm, data, binning="quantile")
    with pytest.raises(ValueError, match="bins"):
        api.fm_reliability(fm, data, bins=0)
    with pytest.raises(ValueError, match="bins"):
        api.fm_calibrate(fm, data, method="isotonic", bins=2000)
    with pytest.raises(ValueError, match="method"):
        api.fm_calibrate(fm, data, method="beta")
    with pytest.raises(ValueError, match="l2"):
        api.fm_calibrate(fm, data, l2=float("nan"))
    with pytest.raises(ValueError, match="newton_steps"):
        api.fm_calibrate(fm, data, newton_steps=0)
    with pytest.raises(ValueError, match="CLASSIFICATION"):
        api.fm_calibrate(model("REGRESSION"), data)
    with pytest.raises(ValueError, match="CLASSIFICATION"):
        api.fm_reliability(model("RANK"), data)
    with pytest.raises(ValueError, match="no labels"):
        api.fm_reliability(fm, nolab)
    with pytest.raises(ValueError, match="features"):
        api.fm_calibrate(model("CLASSIFICATION", 5), data)
    with pytest.raises(ValueError, match="normalize"):
        api.fm_reliability(fm, data, normalize=True)
    with pytest.raises(ValueError, match="groups"):
        api.fm_reliability(fm, data, groups=[0, 1, 2], normalize=False)
    with pytest.raises(ValueError, match="groups"):
        api.fm_reliability(fm, data, groups=np.array([0.5, 1, 2, 3]), normalize=False)
    per_group = dict(cal, groups=np.array([3, 8]), map={"kind": "platt", "ab": np.array([[1.0, 0.0], [1.0, 0.0]])})
    with pytest.raises(ValueError, match="groups is needed"):
        api.fm_predict_calibrated(fm, data, per_group, normalize=False)
    with pytest.raises(ValueError, match="not fitted"):
        api.fm_predict_calibrated(fm, data, per_group, groups=np.array([3, 8, 9, 3]), normalize=False)
