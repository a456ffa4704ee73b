"""CPU-side checks of the RANK task's surface (FMX_TASK_RANKING, fmx_matrix_pairs, the pair metrics, fmwr_amd.fm_train_rank /
fm_rank_evaluate): declared, exported, and every argument check runs before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "fmx.h")).read()


def test_rank_constants_and_sampler_are_declared_and_exported():
    L = _lib()
    h = _header()
    assert re.search(r"#define FMX_TASK_RANKING 30\b", h)
    assert re.search(r"#define FMX_EVAL_PAIR_ACC 666\b", h) and re.search(r"#define FMX_EVAL_BPR 777\b", h)
    assert (L.TASK_RANKING, L.EVAL_PAIR_ACC, L.EVAL_BPR) == (30, 666, 777)
    # the new metric ids clash with none of the reference's (util/Macros.h:24-29)
    assert len({L.EVAL_LL, L.EVAL_AUC, L.EVAL_ACC, L.EVAL_RMSE, L.EVAL_MSE, L.EVAL_MAE, L.EVAL_PAIR_ACC, L.EVAL_BPR}) == 8
    body = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+fmx_matrix_pairs\s*\(", body)
    assert "fmx_matrix_pairs" in L.SYMBOLS
    assert hasattr(L.lib(), "fmx_matrix_pairs")
    import fmwr_amd
    from fmwr_amd import Matrix
    assert callable(fmwr_amd.fm_train_rank) and callable(fmwr_amd.fm_rank_evaluate) and callable(Matrix.pairs)


def test_sampler_without_matrices_is_an_error_not_a_computation():
    L = _lib()
    out = C.c_void_p(12345)
    assert L.lib().fmx_matrix_pairs(None, None, None, C.c_int32(1), C.c_uint64(0), C.c_int64(0), C.byref(out)) == L.ERR_INVALID
    assert out.value is None  # cleared, nothing made
    assert L.lib().fmx_last_error().decode()
    assert L.lib().fmx_matrix_pairs(None, None, None, C.c_int32(1), C.c_uint64(0), C.c_int64(0), None) == L.ERR_INVALID


def test_rank_engine_refuses_unsupported_configurations_before_a_device():
    """fmx_engine_create checks task / mode / solver / parities before it selects a device: these fail the same way with or without one."""
    L = _lib()
    base = dict(task=L.TASK_RANKING, solver=L.SOLVER_SGD, mode=L.MODE_MINIBATCH, batch_rows=64, num_factor=4)
    bad = [dict(mode=L.MODE_SEQUENTIAL), dict(solver=L.SOLVER_ALS), dict(solver=L.SOLVER_MCMC), dict(solver=L.SOLVER_TDAP), dict(batch_rows=63),
           dict(tile_rows=31)]
    for change in bad:
        cfg = L.default_config()
        for k, v in {**base, **change}.items():
            setattr(cfg, k, v)
        h = C.c_void_p(777)
        assert L.lib().fmx_engine_create(C.byref(cfg), C.c_uint64(10), C.byref(h)) == L.ERR_INVALID, change
        assert h.value is None
        msg = L.lib().fmx_last_error().decode()
        assert "RANKING" in msg, (change, msg)


def _ctx_items(n_ctx=6, n_items=5, pc=3, pi=2, seed=0):
    import fmwr_amd as fm
    rng = np.random.default_rng(seed)
    p = pc + pi
    ctx = np.zeros((n_ctx, p)); ctx[:, :pc] = rng.random((n_ctx, pc))
    it = np.zeros((n_items, p)); it[:, pc:] = rng.random((n_items, pi)) + 0.1
    return fm.fm_matrix(ctx), fm.fm_matrix(it)


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api, engine
    fail = lambda *a, **k: pytest.fail("a device was touched")  # noqa: E731
    monkeypatch.setattr(api, "_engine_for", fail)
    monkeypatch.setattr(api, "Engine", fail)
    monkeypatch.setattr(api, "_device_matrix", fail)
    monkeypatch.setattr(engine.Matrix, "from_csr", classmethod(fail))
    monkeypatch.setattr(engine.Matrix, "pairs", classmethod(fail))


def test_fm_train_rank_argument_checks(no_device):
    import scipy.sparse as sp

    import fmwr_amd as fm
    ctx, items = _ctx_items()
    pos = [[0], [1, 1], [], [4, 2], [3], [0, 1]]
    with pytest.raises(ValueError, match="task RANK"):
        fm.fm_train_rank(ctx, items, pos, control=[fm.model_control("CLASSIFICATION")])
    with pytest.raises(ValueError, match="SGD or FTRL"):
        fm.fm_train_rank(ctx, items, pos, control=[fm.model_control("RANK"), fm.solver_control(solver=fm.TDAP_solver())])
    with pytest.raises(ValueError, match="SGD or FTRL"):
        fm.fm_train_rank(ctx, items, pos, control=[fm.model_control("RANK"), fm.solver_control(max_iter=5, solver=fm.ALS_solver())])
    with pytest.raises(ValueError, match="mode"):
        fm.fm_train_rank(ctx, items, pos, mode="sequential")
    with pytest.raises(ValueError, match="even"):
        fm.fm_train_rank(ctx, items, pos, batch_rows=101)
    for kw in (dict(n_neg=0), dict(epochs=-1), dict(n_neg=1.5), dict(batch_rows=0)):
        with pytest.raises(ValueError):
            fm.fm_train_rank(ctx, items, pos, **kw)
    with pytest.raises(ValueError, match="outside"):
        fm.fm_train_rank(ctx, items, [[0], [5], [], [], [], []])
    with pytest.raises(ValueError, match="one index array per row"):
        fm.fm_train_rank(ctx, items, pos[:3])
    with pytest.raises(ValueError, match="must be 6 x 5"):
        fm.fm_train_rank(ctx, items, sp.csr_matrix((6, 4)))
    with pytest.raises(ValueError, match="every item"):  # duplicates count once, and 5 distinct positives of 5 items leave nothing to draw
        fm.fm_train_rank(ctx, items, [[0], [0, 1, 2, 3, 4, 4], [], [], [], []])
    with pytest.raises(ValueError, match="tracker"):
        fm.fm_train_rank(ctx, items, pos, control=[fm.track_control(step_size=10)])
    with pytest.raises(TypeError):
        fm.fm_train_rank(ctx, np.zeros((5, 5)), pos)
    _, wide = _ctx_items(6, 5, pc=3, pi=3)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_train_rank(ctx, wide, pos)


def _rank_fit(p, k=3):
    import fmwr_amd as fm
    rng = np.random.default_rng(0)
    ctl = {"model": fm.model_control("RANK", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    return {"class": "FM", "Model": {"w0": 0.0, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"],
                                     "solver.control": ctl["solver"], "track.control": ctl["track"]},
            "Scales": {"mean": None, "std": None, "model.vars": [f"V{j + 1}" for j in range(p)], "target.range": (-1.0, 1.0)}}


def test_rank_models_refuse_update_and_pointwise_training(no_device):
    import fmwr_amd as fm
    ctx, items = _ctx_items()
    data = fm.fm_matrix(np.ones((4, 5)), labels=np.array([1, -1, 1, -1.0]))
    with pytest.raises(ValueError, match="fm_update"):
        fm.fm_update(_rank_fit(5), data)
    with pytest.raises(ValueError, match="fm_train_rank"):
        fm.fm_train(data, normalize=False, control=[fm.model_control("RANK")])
    with pytest.raises(ValueError, match="n_neg"):
        fm.fm_rank_evaluate(_rank_fit(5), ctx, items, [[0]] * 6, n_neg=0)
    with pytest.raises(ValueError, match="number of input's features"):
        fm.fm_rank_evaluate(_rank_fit(7), ctx, items, [[0]] * 6)
    with pytest.raises(TypeError):
        fm.fm_rank_evaluate({"class": "lm"}, ctx, items, [[0]] * 6)
