"""CPU-side checks of the held-out ranking surface (fmx_heldout_rank / fmx_heldout_rank_device / fmx_heldout_metrics,
fmwr_amd.fm_recommend_metrics): declared, exported, and its argument checks run before any device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_heldout_rank", "fmx_heldout_rank_device", "fmx_heldout_metrics")


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_heldout_entry_points_are_declared_and_exported():
    L = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_heldout_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_heldout_limits")
    import fmwr_amd
    assert callable(fmwr_amd.fm_recommend_metrics)


def test_heldout_without_an_engine_is_an_error_not_a_computation():
    L = _lib()
    rank = np.full(4, 7, np.int64)
    score = np.full(4, 7.0)
    st = L.lib().fmx_heldout_rank(None, None, None, None, None, rank.ctypes.data_as(C.c_void_p), score.ctypes.data_as(C.c_void_p))
    assert st == L.ERR_INVALID
    assert L.lib().fmx_last_error().decode()
    assert np.all(rank == 7) and np.all(score == 7.0)  # nothing written
    st = L.lib().fmx_heldout_rank_device(None, None, C.c_int64(0), C.c_int64(1), None, None, None, None, None)
    assert st == L.ERR_INVALID
    ks = np.array([10], np.int32)
    out = np.full(6, 7.0)
    counted = np.full(2, 7, np.int64)
    st = L.lib().fmx_heldout_metrics(None, None, None, None, None, ks.ctypes.data_as(C.c_void_p), C.c_int32(1), out.ctypes.data_as(C.c_void_p), None,
                                     counted.ctypes.data_as(C.c_void_p))
    assert st == L.ERR_INVALID
    assert np.all(out == 7.0) and np.all(counted == 7)


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
    monkeypatch.setattr(api, "_device_matrix", lambda *a, **k: pytest.fail("a device was touched"))


HELD = [[0], [1, 2], [4]]


@pytest.mark.parametrize("k", [0, -3, 2.5, True, [], [10, 0], list(range(1, 34)), "10"])
def test_fm_recommend_metrics_rejects_a_bad_k(no_device, k):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="k"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), HELD, k=k, normalize=False)


def test_fm_recommend_metrics_rejects_shape_mismatches(no_device):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 7, 2), HELD, normalize=False)
    with pytest.raises(ValueError, match="heldout"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), [[0], [1]], normalize=False)  # 2 lists for 3 contexts
    with pytest.raises(ValueError, match="heldout"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), [[0], [5], []], normalize=False)  # item 5 of 5
    with pytest.raises(ValueError, match="heldout"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), sp.csr_matrix((3, 4)), normalize=False)
    with pytest.raises(ValueError, match="exclude"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), HELD, exclude=[[0], [1]], normalize=False)


def test_fm_recommend_metrics_rejects_non_matrix_inputs(no_device):
    import fmwr_amd as fm
    with pytest.raises(TypeError, match="newdata"):
        fm.fm_recommend_metrics(_fit(6), np.zeros((3, 6)), _data(5, 6, 2), HELD, normalize=False)
    with pytest.raises(TypeError, match="items"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), "items", HELD, normalize=False)
    with pytest.raises(TypeError, match="heldout"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), None, normalize=False)


def test_fm_recommend_metrics_rejects_an_overlap_and_an_empty_heldout(no_device):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="both in heldout and in exclude"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), HELD, exclude=[[3], [2], []], normalize=False)
    with pytest.raises(ValueError, match="no item"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), [[], [], []], normalize=False)
    with pytest.raises(ValueError, match="normalize"):
        fm.fm_recommend_metrics(_fit(6), _data(3, 6, 1), _data(5, 6, 2), HELD, normalize=True)
