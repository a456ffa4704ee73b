"""CPU-side checks of the hard-negative sampler's surface (fmx_matrix_pairs_hard, Matrix.pairs_hard, fm_train_rank(n_candidates=...)):
declared, exported, NULL arguments refused, and fm_train_rank's check of n_candidates runs before a device is touched."""
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


def test_hard_sampler_is_declared_listed_and_exported():
    L = _lib()
    h = open(os.path.join(ROOT, "include", "fmx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+fmx_matrix_pairs_hard\s*\(\s*fmx_engine\s*\*\s*e\s*,\s*const fmx_matrix\s*\*\s*context\s*,\s*const fmx_matrix\s*\*\s*items\s*,"
                     r"\s*const fmx_matrix\s*\*\s*positives\s*,\s*int32_t\s+n_neg\s*,\s*int32_t\s+n_cand\s*,\s*uint64_t\s+seed\s*,\s*int64_t\s+epoch\s*,"
                     r"\s*fmx_matrix\s*\*\*\s*out\s*\)", body)
    assert "fmx_matrix_pairs_hard" in L.SYMBOLS
    assert hasattr(L.lib(), "fmx_matrix_pairs_hard")
    assert "fmx_debug_pairs_hard_chunk" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_pairs_hard_chunk")
    from fmwr_amd import Matrix
    assert callable(Matrix.pairs_hard)


def test_null_arguments_are_refused_and_clear_out():
    L = _lib()
    lib = L.lib()
    for n_cand in (1, 8, 0, 65):
        out = C.c_void_p(12345)
        assert lib.fmx_matrix_pairs_hard(None, None, None, None, 1, n_cand, 0, 0, C.byref(out)) == L.ERR_INVALID
        assert out.value is None  # cleared, nothing made
        assert lib.fmx_last_error().decode()
    assert lib.fmx_matrix_pairs_hard(None, None, None, None, 1, 8, 0, 0, None) == L.ERR_INVALID
    assert lib.fmx_last_error().decode()


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
    monkeypatch.setattr(engine.Matrix, "pairs_hard", classmethod(fail))


def test_fm_train_rank_checks_n_candidates_before_a_device(no_device):
    import fmwr_amd as fm
    ctx, items = _ctx_items()
    pos = [[0], [1, 1], [], [4, 2], [3], [0, 1]]
    for bad in (0, 65, 2.5, True, False, -1, "8", None):
        with pytest.raises(ValueError, match="n_candidates"):
            fm.fm_train_rank(ctx, items, pos, n_candidates=bad)
