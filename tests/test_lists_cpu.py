"""CPU-side checks of the candidate-list surface (fmx_rank_lists / fmx_topk_lists / fmx_project, fmwr_amd.fm_rerank / fm_embed): declared,
exported, its argument checks run before any device is touched, and the numpy model the GPU tests measure against is itself right."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from tests import lists_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_rank_lists", "fmx_rank_lists_device", "fmx_topk_lists", "fmx_topk_lists_device", "fmx_project", "fmx_project_device")


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_list_entry_points_are_declared_and_exported():
    L = _lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fmx.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    hooks = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fmwr_amd", "csrc", "fmx_test_hooks.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fmx_debug_lists_limits\s*\(", hooks)
    assert "fmx_debug_lists_limits" in L.TEST_HOOKS and "fmx_debug_lists_limits" not in L.SYMBOLS
    assert hasattr(L.lib(), "fmx_debug_lists_limits")


def test_list_calls_without_an_engine_are_errors_not_computations():
    L = _lib()
    lib = L.lib()
    score = np.full(4, 7.0)
    pos = np.full(4, 7, np.int64)
    ps, pp = score.ctypes.data_as(C.c_void_p), pos.ctypes.data_as(C.c_void_p)
    none, r0, r1 = None, C.c_int64(0), C.c_int64(1)
    calls = [lambda: lib.fmx_rank_lists(none, none, none, none, C.c_int(L.LINK_NONE), ps, pp),
             lambda: lib.fmx_rank_lists_device(none, none, r0, r1, none, none, C.c_int(L.LINK_NONE), ps, pp),
             lambda: lib.fmx_topk_lists(none, none, none, none, C.c_int32(4), C.c_int(L.LINK_NONE), pp, ps),
             lambda: lib.fmx_topk_lists_device(none, none, r0, r1, none, none, C.c_int32(4), C.c_int(L.LINK_NONE), pp, ps),
             lambda: lib.fmx_project(none, none, C.c_int32(1), ps, ps),
             lambda: lib.fmx_project_device(none, none, r0, r1, C.c_int32(0), ps, ps)]
    for call in calls:
        assert call() == L.ERR_INVALID
        assert lib.fmx_last_error().decode()
        assert np.all(score == 7.0) and np.all(pos == 7)   # nothing written


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


ALL = [[0, 1], [2], []]


@pytest.mark.parametrize("top_k", [0, -3, 1025, 5000])
def test_fm_rerank_rejects_top_k_out_of_range(no_device, top_k):
    import fmwr_amd as fm
    with pytest.raises(ValueError, match="top_k"):
        fm.fm_rerank(_fit(6), _data(3, 6, 1), _data(5, 6, 2), ALL, top_k=top_k, normalize=False)


@pytest.mark.parametrize("top_k", [2.5, True, "3"])
def test_fm_rerank_rejects_a_top_k_that_is_not_an_integer(no_device, top_k):
    import fmwr_amd as fm
    with pytest.raises((ValueError, TypeError), match="top_k|int"):
        fm.fm_rerank(_fit(6), _data(3, 6, 1), _data(5, 6, 2), ALL, top_k=top_k, normalize=False)


def test_fm_rerank_and_fm_embed_reject_bad_matrices(no_device):
    import fmwr_amd as fm
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_rerank(_fit(6), np.zeros((3, 6)), _data(5, 6, 2), ALL, normalize=False)
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_rerank(_fit(6), _data(3, 6, 1), sp.csr_matrix((5, 6)), ALL, normalize=False)
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_embed(_fit(6), np.zeros((3, 6)), normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_rerank(_fit(6), _data(3, 6, 1), _data(5, 7, 2), ALL, normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_rerank(_fit(6), _data(3, 5, 1), _data(5, 6, 2), ALL, normalize=False)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_embed(_fit(6), _data(3, 5, 1), normalize=False)
    bad = _data(3, 6, 1)
    bad.features["value"][2] = np.nan
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_rerank(_fit(6), bad, _data(5, 6, 2), ALL, normalize=False)
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_rerank(_fit(6), _data(3, 6, 1), bad, [[0], [1], [2]], normalize=False)
    with pytest.raises(ValueError, match="NAs"):
        fm.fm_embed(_fit(6), bad, normalize=False)
    with pytest.raises(ValueError, match="normalize"):
        fm.fm_embed(_fit(6), _data(3, 6, 1), normalize=True)   # the model holds no scales


def test_fm_rerank_rejects_bad_candidates(no_device):
    import fmwr_amd as fm
    args = (_fit(6), _data(3, 6, 1), _data(5, 6, 2))
    with pytest.raises(ValueError, match="candidates"):
        fm.fm_rerank(*args, [[0], [1]], normalize=False)            # 2 lists for 3 contexts
    with pytest.raises(ValueError, match="candidates"):
        fm.fm_rerank(*args, [[0], [5], []], normalize=False)        # item 5 of 5
    with pytest.raises(ValueError, match="candidates"):
        fm.fm_rerank(*args, [[0], [-1], []], normalize=False)
    with pytest.raises(ValueError, match="candidates"):
        fm.fm_rerank(*args, sp.csr_matrix((3, 4)), normalize=False)  # the wrong shape
    with pytest.raises(ValueError, match="candidates"):
        fm.fm_rerank(*args, sp.csr_matrix((2, 5)), normalize=False)
    with pytest.raises(TypeError, match="candidates"):
        fm.fm_rerank(*args, None, normalize=False)


@pytest.mark.parametrize("seed", range(6))
def test_the_numpy_model_equals_the_definition(seed):
    """positions and top-K of the model against a double loop over the definition, on inputs with duplicates, exact ties, +-0 and NaN"""
    rng = np.random.default_rng(seed)
    ni = 40
    scores = rng.normal(0, 1, ni).round(1)                      # rounding makes exact ties
    scores[rng.choice(ni, 6, replace=False)] = np.nan
    scores[rng.choice(ni, 4, replace=False)] = 0.0
    scores[rng.choice(ni, 4, replace=False)] = -0.0
    scores[rng.choice(ni, 2, replace=False)] = np.inf
    scores[rng.choice(ni, 2, replace=False)] = -np.inf
    assert np.isnan(scores).any() and np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    for n in (0, 1, 7, 40, 90):
        items = rng.integers(0, ni, n) if n != 40 else rng.permutation(ni)
        pos = lists_model.positions(scores, items)
        assert np.array_equal(pos, lists_model.positions_brute(scores, [int(j) for j in items]))
        distinct = len(set(items.tolist()))
        assert sorted(set(pos.tolist())) == list(range(distinct))   # the positions of the distinct candidates are 0 .. distinct - 1
        for K in (1, 5, 64):
            idx, sc = lists_model.topk(scores, items, K)
            for t in range(K):
                if t < distinct:
                    assert pos[list(items).index(idx[t])] == t
                    assert np.array_equal(sc[t:t + 1], scores[idx[t]:idx[t] + 1], equal_nan=True)
                    assert np.signbit(sc[t]) == np.signbit(scores[idx[t]])
                else:
                    assert idx[t] == -1 and np.isnan(sc[t])
    # NaN below -inf, +0 and -0 one score ordered by the index
    s = np.array([np.nan, -np.inf, -0.0, 0.0, 1.0])
    assert lists_model.ordered(s, [0, 1, 2, 3, 4]).tolist() == [4, 2, 3, 1, 0]
