"""CPU-side checks of the contribution surface (fmx_contrib / fmx_contrib_device / fmx_contrib_summary, fmwr_amd.fm_explain): declared,
exported, and its argument checks run before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_contrib", "fmx_contrib_device", "fmx_contrib_summary")


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_contrib_entry_points_are_declared_and_exported():
    L = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)


def test_contrib_without_an_engine_is_an_error_not_a_computation():
    L = _lib()
    out = np.full(4, 7.0)
    cnt = np.full(4, 7, np.int64)
    ptr = out.ctypes.data_as(C.c_void_p)
    assert L.lib().fmx_contrib(None, None, ptr) == L.ERR_INVALID
    assert L.lib().fmx_last_error().decode()
    assert L.lib().fmx_contrib_device(None, None, C.c_int64(0), C.c_int64(1), ptr) == L.ERR_INVALID
    assert L.lib().fmx_contrib_summary(None, None, ptr, ptr, cnt.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID
    assert np.all(out == 7.0) and np.all(cnt == 7)  # nothing written


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


def test_fm_explain_rejects_a_wrong_type(no_device):
    import fmwr_amd as fm
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_explain(_fit(6), np.ones((3, 6)), normalize=False)


def test_fm_explain_rejects_nans(no_device):
    import fmwr_amd as fm
    d = _data(3, 6, 1)
    d.features["value"][2] = np.nan
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_explain(_fit(6), d, normalize=False)


def test_fm_explain_rejects_a_feature_count_mismatch(no_device):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_explain(_fit(6), _data(3, 7, 1), normalize=False)


def test_fm_explain_rejects_normalize_without_scales(no_device):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="normalize"):
        fm.fm_explain(_fit(6), _data(3, 6, 1), normalize=True)
