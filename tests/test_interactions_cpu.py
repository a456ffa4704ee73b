"""CPU-side checks of the interaction surface (fmx_interactions / fmx_interactions_device / fmx_interactions_summary, fmwr_amd.fm_interactions):
the numpy model of the definition (tests/interactions_model.py) against a brute-force loop and against the identities that tie the pair
values to the contributions and the forward; the declared surface; the argument checks, which run before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from tests import interactions_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_interactions", "fmx_interactions_device", "fmx_interactions_summary")


def _rows(lens, p, rng):
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, p, int(rp[-1])).astype(np.uint32)
    val = rng.normal(0, 1, int(rp[-1])).astype(np.float32)
    return rp, col, val


def _tables(rng, k, p, fp32):
    v = rng.normal(0, 0.4, (k, p))
    return v.astype(np.float32).astype(np.float64) if fp32 else v


@pytest.mark.parametrize("fp32", [True, False])
def test_model_against_a_brute_force_double_loop(fp32):
    rng = np.random.default_rng(3 + fp32)
    p, k = 40, 5
    v = _tables(rng, k, p, fp32)
    rp, col, val = _rows(rng.integers(0, 9, 200), p, rng)
    for r in range(200):
        c, x = col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]
        a, b, I = im.pair_values(v, c, x)
        ref = im.brute_pairs(v, c, x)
        assert [(int(i), int(j)) for i, j in zip(a, b)] == [(i, j) for i, j, _ in ref]
        assert np.array_equal(im.bits(I), im.bits([t for _, _, t in ref]))


def test_order_is_by_magnitude_then_position_with_nan_last():
    a = np.array([0, 0, 0, 1, 1, 2])
    b = np.array([1, 2, 3, 2, 3, 3])
    val = np.array([-2.0, np.nan, 0.0, 2.0, -0.0, 3.0])
    o = im.order(a, b, val)
    assert [(int(a[i]), int(b[i])) for i in o] == [(2, 3), (0, 1), (1, 2), (0, 3), (1, 3), (0, 2)]


def _closed_form(w, v, rp, col, val, k1):
    """phi of every entry (fm_contrib's closed form), its linear part, and each entry's row max |phi|"""
    x = val.astype(np.float64)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    T = v.T[col] * x[:, None]
    S = np.zeros((len(rp) - 1, v.shape[0]))
    np.add.at(S, row, T)
    lin = k1 * x * w[col]
    phi = lin + 0.5 * (T * (S[row] - T)).sum(1)
    rmax = np.zeros(len(rp) - 1)
    np.maximum.at(rmax, row, np.abs(phi))
    return phi, lin, rmax[row]


@pytest.mark.parametrize("k0,k1", [(1, 1), (0, 1), (1, 0)])
def test_identities_against_the_closed_form_and_the_forward(k0, k1):
    rng = np.random.default_rng(11)
    p, k = 60, 7
    w0, w, v = 0.3, rng.normal(0, 0.5, p), _tables(rng, k, p, True)
    rp, col, val = _rows(rng.integers(0, 12, 120), p, rng)
    phi, lin, rmax = _closed_form(w, v, rp, col, val, k1)
    P = oracle.params(task=oracle.REGRESSION, k=k, k0=bool(k0), k1=bool(k1))
    yhat = oracle.predict_batch(P, oracle.Matrix(rp, col, val, p), w0, w, v.ravel())
    for r in range(len(rp) - 1):
        a, b, I = im.pair_values(v, col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]])
        m = rp[r + 1] - rp[r]
        per = np.zeros(m)
        np.add.at(per, a, I)
        np.add.at(per, b, I)
        sl = slice(rp[r], rp[r + 1])
        assert np.all(np.abs(per - 2 * (phi[sl] - lin[sl])) <= 2 * 1e-12 * (1 + rmax[sl])), r
        got = k0 * w0 + lin[sl].sum() + I.sum()
        assert abs(got - yhat[r]) <= 1e-10 * (1 + abs(yhat[r])), r


def test_prefix_property_and_k_zero():
    rng = np.random.default_rng(5)
    p = 30
    rp, col, val = _rows([0, 1, 2, 5, 9, 12], p, rng)
    v = _tables(rng, 4, p, True)
    big = im.top_m(v, rp, col, val, 64)
    for m_top in (1, 2, 7, 63):
        sa, sb, sv = im.top_m(v, rp, col, val, m_top)
        assert np.array_equal(sa, big[0][:, :m_top]) and np.array_equal(sb, big[1][:, :m_top])
        assert np.array_equal(im.bits(sv), im.bits(big[2][:, :m_top]))
    assert np.all(big[0][:2] == -1) and np.all(big[1][:2] == -1) and np.all(np.isnan(big[2][:2]))   # rows of 0 and 1 entries have no pair
    assert np.all(big[0][4, 36:] == -1) and big[0][4, 35] >= 0    # 9 entries: 36 pairs
    assert np.all(big[0][5] >= 0)                                  # 12 entries: 66 pairs, every slot taken
    a, b, val0 = im.top_m(np.zeros((0, p)), rp, col, val, 3)
    assert np.array_equal(im.bits(val0[3]), im.bits([0.0, 0.0, 0.0]))   # +0.0, in (a, b) order
    assert a[3].tolist() == [0, 0, 0] and b[3].tolist() == [1, 2, 3]


def test_planted_interaction_is_found():
    p, groups, v, rp, col, val = im.planted(np.random.default_rng(2))
    a, b, _ = im.top_m(v, rp, col, val, 1)
    assert np.all(a[:, 0] == 1) and np.all(b[:, 0] == 4)
    s = im.summary(v, rp, col, val, groups, 6)
    iu = np.triu_indices(6)
    best = np.argmax(s["abs_sum"][iu])
    assert (iu[0][best], iu[1][best]) == (1, 4)
    assert np.array_equal(s["abs_sum"], s["abs_sum"].T) and np.array_equal(s["count"], s["count"].T)
    assert np.all(s["count"][~np.eye(6, dtype=bool)] == 300) and np.all(np.diag(s["count"]) == 0)


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_interaction_entry_points_are_declared_and_exported():
    L = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_interactions_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_interactions_limits")
    import fmwr_amd as fm
    assert callable(fm.fm_interactions)
    for method in ("interactions", "interactions_device", "interactions_summary"):
        assert callable(getattr(fm.Engine, method))


def test_interactions_without_an_engine_are_an_error_not_a_computation():
    L = _lib()
    out = np.full(4, 7.0)
    idx = np.full(4, 7, np.int64)
    po, pi = out.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)
    assert L.lib().fmx_interactions(None, None, 2, pi, pi, po) == L.ERR_INVALID
    assert L.lib().fmx_last_error().decode()
    assert L.lib().fmx_interactions_device(None, None, 0, 1, 2, pi, pi, po) == L.ERR_INVALID
    assert L.lib().fmx_interactions_summary(None, None, None, 2, po, po, pi) == L.ERR_INVALID
    assert np.all(out == 7.0) and np.all(idx == 7)  # nothing written


def _fit(p, k=3):
    """a fitted-model object as fm_train returns it, without training (the checks below never reach a device)"""
    import fmwr_amd as fm
    rng = np.random.default_rng(0)
    ctl = {"model": fm.model_control("CLASSIFICATION", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    return {"Model": {"w0": 0.1, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"], "solver.control": ctl["solver"],
                      "track.control": ctl["track"]},
            "Scales": {"mean": None, "std": None, "target.range": (-1.0, 1.0)}}


def _data(n, p, seed):
    import fmwr_amd as fm
    return fm.fm_matrix(np.random.default_rng(seed).random((n, p)))


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    monkeypatch.setattr(api, "_engine_for", lambda *a, **k: pytest.fail("a device was touched"))


def test_fm_interactions_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_interactions(_fit(6), np.ones((3, 6)), normalize=False)
    d = _data(3, 6, 1)
    d.features["value"][2] = np.nan
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_interactions(_fit(6), d, normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_interactions(_fit(6), _data(3, 7, 1), normalize=False)
    with pytest.raises(ValueError, match="normalize"):
        fm.fm_interactions(_fit(6), _data(3, 6, 1), normalize=True)
    for top in (0, 65):
        with pytest.raises(ValueError, match="top must be in 1..64"):
            fm.fm_interactions(_fit(6), _data(3, 6, 1), top=top, normalize=False)
    with pytest.raises(ValueError, match="one integer group id per feature"):
        fm.fm_interactions(_fit(6), _data(3, 6, 1), groups=[0, 1, 2], normalize=False)
    with pytest.raises(ValueError, match="one integer group id per feature"):
        fm.fm_interactions(_fit(6), _data(3, 6, 1), groups=np.zeros(6), normalize=False)
    with pytest.raises(ValueError, match=">= 0"):
        fm.fm_interactions(_fit(6), _data(3, 6, 1), groups=[0, 1, -1, 0, 1, 2], normalize=False)
    with pytest.raises(ValueError, match="at most 64 groups"):
        fm.fm_interactions(_fit(6), _data(3, 6, 1), groups=[0, 1, 64, 0, 1, 2], normalize=False)
