"""CPU-side checks of the top-K recommendation surface (fmx_topk / fmx_topk_device, fmwr_amd.fm_recommend): declared, exported,
and its argument checks run before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_topk_entry_points_are_declared_and_exported():
    L = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    for name in ("fmx_topk", "fmx_topk_device"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)


def test_topk_without_an_engine_is_an_error_not_a_computation():
    L = _lib()
    idx = np.full(4, 7, np.int64)
    score = np.full(4, 7.0)
    st = L.lib().fmx_topk(None, None, None, None, C.c_int32(4), C.c_int(L.LINK_NONE), idx.ctypes.data_as(C.c_void_p), score.ctypes.data_as(C.c_void_p))
    assert st == L.ERR_INVALID
    assert L.lib().fmx_last_error().decode()
    assert np.all(idx == 7) and np.all(score == 7.0)  # nothing written
    st = L.lib().fmx_topk_device(None, None, C.c_int64(0), C.c_int64(1), None, None, C.c_int32(4), C.c_int(L.LINK_NONE), None, None)
    assert st == L.ERR_INVALID


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


@pytest.mark.parametrize("top_k", [0, -3, 1025, 5000])
def test_fm_recommend_rejects_top_k_out_of_range(monkeypatch, top_k):
    import fmwr_amd as fm
    from fmwr_amd import api
    monkeypatch.setattr(api, "_engine_for", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="top_k"):
        fm.fm_recommend(_fit(6), _data(3, 6, 1), _data(5, 6, 2), top_k=top_k, normalize=False)


def test_fm_recommend_rejects_a_feature_count_mismatch(monkeypatch):
    import fmwr_amd as fm
    from fmwr_amd import api
    monkeypatch.setattr(api, "_engine_for", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_recommend(_fit(6), _data(3, 6, 1), _data(5, 7, 2), top_k=2, normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_recommend(_fit(6), _data(3, 5, 1), _data(5, 6, 2), top_k=2, normalize=False)


def test_fm_recommend_rejects_a_bad_exclusion(monkeypatch):
    import fmwr_amd as fm
    from fmwr_amd import api
    monkeypatch.setattr(api, "_engine_for", lambda *a, **k: pytest.fail("a device was touched"))
    with pytest.raises(ValueError, match="exclude"):
        fm.fm_recommend(_fit(6), _data(3, 6, 1), _data(5, 6, 2), top_k=2, exclude=[[0], [1]], normalize=False)   # 2 lists for 3 contexts
    with pytest.raises(ValueError, match="exclude"):
        fm.fm_recommend(_fit(6), _data(3, 6, 1), _data(5, 6, 2), top_k=2, exclude=[[0], [5], []], normalize=False)   # item 5 of 5
    with pytest.raises(ValueError, match="exclude"):
        fm.fm_recommend(_fit(6), _data(3, 6, 1), _data(5, 6, 2), top_k=2, exclude=sp.csr_matrix((3, 4)), normalize=False)
