"""fmx_fold_in / Engine.fold_in / fm_fold_in: the rows of new features solved against the frozen model.  The yardstick
is tests/foldin_model.py in np.longdouble; the bar is the project's fp64 bar 1e-11 relative to a feature's max |theta|, provided the fp64
model's own spread on the same inputs (permuted rows against longdouble; asserted in tests/test_foldin_cpu.py) is <= 1e-13, and 100 x that
spread otherwise."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from tests import foldin_model as M

pytestmark = pytest.mark.gpu

KINDS = ["mb32", "mb32_wir", "mb64", "seq64"]


def _record(line):
    """every measured figure is printed (pytest -s) and, with FMX_FOLDIN_REPORT set to a path, appended to that file: profiles/foldin.txt quotes such a run"""
    print(line)
    path = os.environ.get("FMX_FOLDIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _engine(kind, p, k, monkeypatch, loss=M.SQUARED, k0=1, k1=1, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    common = dict(num_factor=k, task=L.TASK_REGRESSION if loss == M.SQUARED else L.TASK_CLASSIFICATION, keep_w0=k0, keep_w1=k1, **kw)
    if kind == "seq64":
        return engine.Engine(p, mode=L.MODE_SEQUENTIAL, **common)
    return engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), **common)


def _matrix(inp, y):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], inp["p"], y)


def _theta(w, v):
    return np.concatenate([w[:, None], v.T], axis=1)


def _bar(valued, k, loss, n_newton=8):
    s = M.spread(valued, k, loss, n_newton)
    return 1e-11 if s <= 1e-13 else 100 * s


def _case(kind, k, valued, loss, monkeypatch, lw=0.1, lv=0.1, k0=1, k1=1, n_newton=8):
    inp = M.inputs(valued)
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch, loss, k0, k1)
    e.set_params(w0, w, v)
    gw, gv, rows, status = e.fold_in(_matrix(inp, M.targets(valued, k, loss)), inp["ids"], lw, lv, newton_steps=n_newton)
    ref, rrows, rstatus = M.reference(valued, k, loss, lw, lv, k0, k1, n_newton)
    assert np.array_equal(rows, rrows) and np.array_equal(rows, inp["sizes"])
    assert np.array_equal(status, rstatus) and not status.any()
    err = M.rel_err(_theta(gw, gv), ref)
    _record(f"fold-in {loss} {kind} k={k} valued={valued} lw={lw} lv={lv} k0={k0} k1={k1} newton={n_newton}: error {err:.3g}")
    if not k1:
        assert np.all(gw == 0)
    return err


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", M.KS)
@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
def test_parity_fp32_tables(loss, k, valued, monkeypatch):
    assert _case("mb32", k, valued, loss, monkeypatch) <= _bar(valued, k, loss)


@pytest.mark.parametrize("kind,k", [("mb64", 17), ("seq64", 16), ("seq64", 33), ("mb32_wir", 16), ("mb32_wir", 2)])
@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
def test_parity_table_and_layout_forms(loss, kind, k, monkeypatch):
    if kind == "mb32_wir":
        assert _engine(kind, 300, k, monkeypatch).w_in_row()
    assert _case(kind, k, True, loss, monkeypatch) <= _bar(True, k, loss)


@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
@pytest.mark.parametrize("form", ["no_w0", "no_w1", "lambdas"])
def test_parity_keep_flags_and_unequal_lambdas(loss, form, monkeypatch):
    kw = {"no_w0": dict(k0=0), "no_w1": dict(k1=0), "lambdas": dict(lw=0.03, lv=0.7)}[form]
    for kind in ("mb32", "seq64"):
        assert _case(kind, 16, True, loss, monkeypatch, **kw) <= _bar(True, 16, loss)


@pytest.mark.parametrize("k", [16, 33])
def test_first_newton_step(k, monkeypatch):
    assert _case("mb32", k, True, M.LOGISTIC, monkeypatch, n_newton=1) <= _bar(True, k, M.LOGISTIC, 1)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
@pytest.mark.parametrize("loss", [M.SQUARED, M.LOGISTIC])
def test_bits_do_not_depend_on_company_order_call_or_current_rows(kind, loss, monkeypatch):
    from fmwr_amd import _lib as L
    k = 17
    inp = M.inputs(True)
    ids = inp["ids"]
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch, loss)
    e.set_params(w0, w, v)
    m = _matrix(inp, M.targets(True, k, loss))
    full = e.fold_in(m, ids, 0.1, 0.1)
    assert _same(full, e.fold_in(m, ids, 0.1, 0.1))                       # a second call
    perm = np.random.default_rng(3).permutation(len(ids))
    got = e.fold_in(m, ids[perm], 0.1, 0.1)                               # ids permuted
    assert _same((full[0][perm], full[1][:, perm], full[2][perm], full[3][perm]), got)
    for g in (0, 1, 5, 8, len(ids) - 1, len(ids) - 2):                    # alone: the other fold columns are then ordinary features of rows that are ignored
        one = e.fold_in(m, ids[g:g + 1], 0.1, 0.1)
        assert _same((full[0][g:g + 1], full[1][:, g:g + 1], full[2][g:g + 1], full[3][g:g + 1]), one), g
    sub = np.array([len(ids) - 1, 3, 9])
    assert _same((full[0][sub], full[1][:, sub], full[2][sub], full[3][sub]), e.fold_in(m, ids[sub], 0.1, 0.1))
    L.check(L.lib().fmx_debug_foldin_slab(C.c_int64(700), C.c_int64(3)))  # the next call: slabs of at most 700 rows and 3 groups
    assert _same(full, e.fold_in(m, ids, 0.1, 0.1))
    # the fold features' current rows never enter: large values, then NaN
    before = e.get_params()
    e.set_rows(ids, np.full(len(ids), 1e30), np.full((k, len(ids)), -3e28))
    assert _same(full, e.fold_in(m, ids, 0.1, 0.1))
    e.set_rows(ids, np.full(len(ids), np.nan), np.full((k, len(ids)), np.nan))
    assert _same(full, e.fold_in(m, ids, 0.1, 0.1))
    e.set_rows(ids, before[1][ids], before[2][:, ids])
    after = e.get_params()                                                # apply = 0 modifies nothing
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])


@pytest.mark.parametrize("kind", ["mb32", "mb32_wir", "mb64"])
def test_apply_writes_the_rows_as_set_rows_and_nothing_else(kind, tmp_path, monkeypatch):
    from fmwr_amd import _lib as L
    k = 16
    inp = M.inputs(True)
    ids = inp["ids"]
    y = M.targets(True, k, M.SQUARED)
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch, solver=L.SOLVER_FTRL, l1_w1=1e-3, l1_v=1e-4, l2_w1=1e-2, l2_v=1e-2)
    e.set_params(w0, w, v)
    m = _matrix(inp, y)
    e.train(m, 1024)                                                      # optimiser tables that are not all zero
    e.sync()
    p0 = e.get_params()
    e.save(tmp_path / "before.ckpt")
    dry = e.fold_in(m, ids, 0.1, 0.1, apply=False)
    p1 = e.get_params()
    assert p1[0] == p0[0] and p1[1].tobytes() == p0[1].tobytes() and p1[2].tobytes() == p0[2].tobytes()
    got = e.fold_in(m, ids, 0.1, 0.1, apply=True)
    assert _same(dry, got)
    rw, rv = e.get_rows(ids)
    state = np.float32 if kind != "mb64" else np.float64
    assert np.array_equal(rw, got[0].astype(state).astype(np.float64)) and np.array_equal(rv, got[1].astype(state).astype(np.float64))
    p2 = e.get_params()
    others = np.setdiff1d(np.arange(inp["p"]), ids)
    assert p2[0] == p0[0] and np.array_equal(p2[1][others], p0[1][others]) and np.array_equal(p2[2][:, others], p0[2][:, others])
    e.set_rows(ids, p0[1][ids], p0[2][:, ids])                            # the fold rows back: the checkpoint (parameters, scalars, optimiser
    e.save(tmp_path / "after.ckpt")                                       # tables) is then the one from before, byte for byte
    assert (tmp_path / "after.ckpt").read_bytes() == (tmp_path / "before.ckpt").read_bytes()


def test_multi_gpu_engine_reads_and_writes_its_primary_replica(monkeypatch):
    """(that the other replicas follow is fmx_set_rows' own contract, which apply goes through, and its tests')"""
    k = 16
    inp = M.inputs(True)
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine("mb32", inp["p"], k, monkeypatch, n_gpus=2, gpus_share_device=1)
    e.set_params(w0, w, v)
    gw, gv, rows, status = e.fold_in(_matrix(inp, M.targets(True, k, M.SQUARED)), inp["ids"], 0.1, 0.1, apply=True)
    assert M.rel_err(_theta(gw, gv), M.reference(True, k, M.SQUARED)[0]) <= _bar(True, k, M.SQUARED)
    rw, rv = e.get_rows(inp["ids"])
    assert np.array_equal(rw, gw.astype(np.float32).astype(np.float64)) and np.array_equal(rv, gv.astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
@pytest.mark.parametrize("k", [16, 64])
def test_recovery_of_a_planted_row(kind, k, monkeypatch):
    """Noise-free targets from the engine's own row of u, lambda = 0, groups of >= 257 rows: theta returns that row.  The targets are
    float32 (the matrix's label type), so the problem handed over is the planted one only to about 6e-8: the bar is max(1e-11, 100 x the
    error of the fp64 model on the same input, which the longdouble model confirms to be the input's and not the arithmetic's)."""
    inp = M.inputs(True)
    big = np.flatnonzero(inp["sizes"] >= 257)
    ids = inp["ids"][big]
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch)
    e.set_params(w0, w, v)
    planted = _theta(w[ids], v[:, ids])
    import oracle
    P = oracle.params(task=oracle.REGRESSION, k=k)
    y = oracle.predict_batch(P, oracle.Matrix(inp["rp"], inp["col"], inp["val"], inp["p"]), w0, w, v.ravel()).astype(np.float32)
    t64 = M.fold_in(inp["rp"], inp["col"], inp["val"], y, ids, w0, w, v, 0.0, 0.0, dtype=np.float64)[0]
    tld = M.fold_in(inp["rp"], inp["col"], inp["val"], y, ids, w0, w, v, 0.0, 0.0, dtype=np.longdouble)[0]
    model_err = max(M.rel_err(t64, planted), M.rel_err(tld, planted))
    gw, gv, rows, status = e.fold_in(_matrix(inp, y), ids, 0.0, 0.0)
    err = M.rel_err(_theta(gw, gv), planted)
    # ... and the tight check of the lambda = 0 path: the GPU against the longdouble model on the SAME float32 targets, under the parity rule
    # (1e-11 provided the fp64 model's own error against longdouble here is <= 1e-13, 100 x that error otherwise)
    model_spread = M.rel_err(t64, tld)
    parity = M.rel_err(_theta(gw, gv), tld)
    _record(f"fold-in recovery {kind} k={k}: model error {model_err:.3g}, GPU error {err:.3g}; against longdouble on the same targets: fp64 model "
            f"{model_spread:.3g}, GPU {parity:.3g}")
    assert not status.any() and np.array_equal(rows, inp["sizes"][big])
    assert err <= max(1e-11, 100 * model_err)
    assert parity <= (1e-11 if model_spread <= 1e-13 else 100 * model_spread)


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
def test_status_of_an_unsolvable_group(kind, monkeypatch):
    """lambda = 0 and fewer than k + 1 rows: no row at all gives H = 0, and one one-hot row gives H = z z' with z_0 = 1, whose first
    elimination step leaves round(z_i z_c) - round(z_i z_c) = 0 exactly: a pivot that is not positive in any arithmetic"""
    k = 16
    inp = M.inputs(False)
    sizes = list(inp["sizes"])
    pick = np.array([sizes.index(1), sizes.index(257), sizes.index(0), sizes.index(1000)])
    ids = inp["ids"][pick]
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch)
    e.set_params(w0, w, v)
    before = e.get_rows(ids)
    gw, gv, rows, status = e.fold_in(_matrix(inp, M.targets(False, k, M.SQUARED)), ids, 0.0, 0.0, apply=True)
    assert list(status) == [1, 0, 1, 0] and list(rows) == [1, 257, 0, 1000]
    assert np.all(np.isnan(gw[[0, 2]])) and np.all(np.isnan(gv[:, [0, 2]])) and np.all(np.isfinite(gw[[1, 3]])) and np.all(np.isfinite(gv[:, [1, 3]]))
    after = e.get_rows(ids)
    assert np.array_equal(after[0][[0, 2]], before[0][[0, 2]]) and np.array_equal(after[1][:, [0, 2]], before[1][:, [0, 2]])
    state = np.float32 if kind == "mb32" else np.float64
    assert np.array_equal(after[0][[1, 3]], gw[[1, 3]].astype(state).astype(np.float64))
    assert np.array_equal(after[1][:, [1, 3]], gv[:, [1, 3]].astype(state).astype(np.float64))
    # a feature without rows and positive lambdas: theta = 0, solved
    gw, gv, rows, status = e.fold_in(_matrix(inp, M.targets(False, k, M.SQUARED)), ids[2:3], 0.1, 0.1)
    assert status[0] == 0 and rows[0] == 0 and gw[0] == 0 and np.all(gv == 0)


def test_refusals_touch_nothing(monkeypatch):
    from fmwr_amd import _lib as L, engine
    k = 8
    inp = M.inputs(True)
    p, ids = inp["p"], inp["ids"]
    w0, w, v = M.model_params(p, k)
    y = M.targets(True, k, M.LOGISTIC)
    reg = _engine("mb32", p, k, monkeypatch)
    cls = _engine("mb32", p, k, monkeypatch, M.LOGISTIC)
    rank = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, num_factor=k, task=L.TASK_RANKING)
    wide = _engine("seq64", p, 65, monkeypatch)
    for e in (reg, cls, rank):
        e.set_params(w0, w, v)
    m = _matrix(inp, y)
    unlabelled = _matrix(inp, None)
    other_p = engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], p + 1, y)
    # a row with two fold features; a row with the same fold column stored twice
    rp2 = np.concatenate([inp["rp"], [inp["rp"][-1] + 3]])
    two = engine.Matrix.from_csr(rp2, np.concatenate([inp["col"], [5, ids[3], ids[4]]]).astype(np.uint32), np.concatenate([inp["val"], [1, 1, 1]]).astype(np.float32), p,
                                 np.concatenate([y, [1]]).astype(np.float32))
    twice = engine.Matrix.from_csr(rp2, np.concatenate([inp["col"], [5, ids[3], ids[3]]]).astype(np.uint32), np.concatenate([inp["val"], [1, 1, 1]]).astype(np.float32), p,
                                   np.concatenate([y, [1]]).astype(np.float32))
    ybad = y.copy()
    ybad[np.flatnonzero(np.diff(inp["rp"]) == 4)[7]] = 0.5                 # a participating row
    bad_label = _matrix(inp, ybad)
    yok = y.copy()
    yok[np.flatnonzero(np.diff(inp["rp"]) == 3)] = 0.25                    # rows without a fold feature may carry any label
    fine_label = _matrix(inp, yok)

    def refused(e, mat, idl, lw=0.1, lv=0.1, newton=8, apply=1):
        idl = np.ascontiguousarray(idl, np.uint32)
        n = len(idl)
        ow = np.full(max(n, 1), 7.0); ov = np.full(max(n * max(e.k, 1), 1), 7.0)
        orows = np.full(max(n, 1), 7, np.int64); ost = np.full(max(n, 1), 7, np.int32)
        params = e.get_params()
        st = L.lib().fmx_fold_in(e.h, mat.h, idl.ctypes.data_as(C.c_void_p), n, lw, lv, newton, apply, ow.ctypes.data_as(C.c_void_p), ov.ctypes.data_as(C.c_void_p),
                                 orows.ctypes.data_as(C.c_void_p), ost.ctypes.data_as(C.c_void_p))
        after = e.get_params()
        untouched = (np.all(ow == 7) and np.all(ov == 7) and np.all(orows == 7) and np.all(ost == 7) and after[0] == params[0]
                     and after[1].tobytes() == params[1].tobytes() and after[2].tobytes() == params[2].tobytes())
        return st, untouched

    cases = {
        "no labels": (reg, unlabelled, ids), "p mismatch": (reg, other_p, ids), "id >= p": (reg, m, [ids[0], p]), "id twice": (reg, m, [ids[0], ids[1], ids[0]]),
        "negative lambda_w": (reg, m, ids, -0.1, 0.1), "negative lambda_v": (reg, m, ids, 0.1, -1e-300), "NaN lambda_w": (reg, m, ids, np.nan, 0.1),
        "NaN lambda_v": (reg, m, ids, 0.1, np.nan), "RANKING engine": (rank, m, ids), "more than 64 factors": (wide, m, ids),
        "n_newton < 1": (cls, m, ids, 0.1, 0.1, 0), "label other than +-1": (cls, bad_label, ids), "two fold features in a row": (reg, two, ids),
        "one fold column twice in a row": (reg, twice, ids), "two fold features in a row (classification)": (cls, two, ids),
    }
    for name, args in cases.items():
        st, untouched = refused(*args)
        assert st == L.ERR_INVALID and untouched, name
    for e_h, m_h in ((None, m.h), (reg.h, None)):
        assert L.lib().fmx_fold_in(e_h, m_h, ids.ctypes.data_as(C.c_void_p), len(ids), 0.1, 0.1, 8, 0, None, None, None, None) == L.ERR_INVALID
    # not refusals: no ids (nothing written), a label off +-1 in a row that does not take part, the offending row's columns not folded, REGRESSION with n_newton = 0
    st, untouched = refused(reg, m, [])
    assert st == L.OK and untouched
    assert not cls.fold_in(fine_label, ids, 0.1, 0.1)[3].any()
    assert not reg.fold_in(two, ids[:3], 0.1, 0.1)[3].any()
    assert not reg.fold_in(m, ids, 0.1, 0.1, newton_steps=0)[3].any()
    if L.lib().fmx_device_count is not None:
        cnt = C.c_int32()
        L.check(L.lib().fmx_device_count(C.byref(cnt)))
        if cnt.value > 1:                                                  # a matrix on another device
            far = engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], p, y, device=1)
            st, untouched = refused(reg, far, ids)
            assert st == L.ERR_INVALID and untouched


def _planted_users(seed=0):
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    n_users, n_new, n_items, k, per = 160, 40, 50, 4, 30
    bu, bi = rng.normal(0, 1.0, n_users), rng.normal(0, 0.5, n_items)
    pu, qi = rng.normal(0, 0.6, (n_users, k)), rng.normal(0, 0.6, (n_items, k))
    users = np.repeat(np.arange(n_users), per)
    items = np.concatenate([rng.choice(n_items, per, replace=False) for _ in range(n_users)])
    y = 3.0 + bu[users] + bi[items] + np.einsum("ij,ij->i", pu[users], qi[items]) + rng.normal(0, 0.05, len(users))
    n = len(users)
    X = sp.csr_matrix((np.ones(2 * n), (np.repeat(np.arange(n), 2), np.stack([users, n_users + items], 1).ravel())), shape=(n, n_users + n_items))
    new = np.arange(n_users - n_new, n_users)
    is_new = users >= n_users - n_new
    half = (np.arange(n) % 2 == 0)
    return X, y, new, ~is_new, is_new & half, is_new & ~half, k


def test_fm_fold_in_end_to_end():
    import copy
    import fmwr_amd as fm
    X, y, new, old_rows, fold_rows, test_rows, k = _planted_users()
    ctl = [fm.model_control("REGRESSION", **{"factor.number": k}), fm.solver_control(max_iter=20, solver=fm.ALS_solver(update_v=True))]
    fit = fm.fm_train(fm.fm_matrix(X[old_rows], y[old_rows]), normalize=False, control=ctl, seed=5)   # the 40 users' columns hold nothing
    keep = copy.deepcopy(fit)
    folded = fm.fm_fold_in(fit, fm.fm_matrix(X[fold_rows], y[fold_rows]), list(new), l2_w=0.1, l2_v=0.1)
    assert folded is not fit
    for a, b in ((fit["Model"]["w"], keep["Model"]["w"]), (fit["Model"]["v"], keep["Model"]["v"])):
        assert np.array_equal(a, b)                                                                    # the input object is untouched
    assert "fold.in" not in fit and fit["Model"]["w0"] == keep["Model"]["w0"]
    info = folded["fold.in"]
    assert info["features"] == [f"V{j + 1}" for j in new] and np.array_equal(info["rows"], np.full(len(new), 15)) and not info["status"].any()
    others = np.setdiff1d(np.arange(X.shape[1]), new)
    assert np.array_equal(folded["Model"]["w"][others], fit["Model"]["w"][others]) and np.array_equal(folded["Model"]["v"][:, others], fit["Model"]["v"][:, others])
    assert np.all(fit["Model"]["w"][new] == 0) and np.any(folded["Model"]["w"][new] != 0)
    test = fm.fm_matrix(X[test_rows])
    rmse = lambda f: float(np.sqrt(np.mean((fm.predict(f, test, normalize=False) - y[test_rows]) ** 2)))
    r0, r1 = rmse(fit), rmse(folded)
    _record(f"fm_fold_in: held-out RMSE unfolded {r0:.4f}, folded {r1:.4f}")
    assert r1 < r0
    by_name = fm.fm_fold_in(fit, fm.fm_matrix(X[fold_rows], y[fold_rows]), [f"V{j + 1}" for j in new])
    assert np.array_equal(by_name["Model"]["w"], folded["Model"]["w"]) and np.array_equal(by_name["Model"]["v"], folded["Model"]["v"])
    # status 1 keeps the old row and warns: lambda = 0 and a user without rows
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        part = fm.fm_fold_in(fit, fm.fm_matrix(X[old_rows][:50], y[old_rows][:50]), [int(new[0])], l2_w=0.0, l2_v=0.0)
    assert part["fold.in"]["status"][0] == 1 and part["Model"]["w"][new[0]] == fit["Model"]["w"][new[0]] and any("could not be solved" in str(r.message) for r in rec)
    # data whose columns are not the model's (another order would fold the wrong column)
    with pytest.raises(ValueError):
        fm.fm_fold_in(fit, fm.fm_matrix(X[fold_rows], y[fold_rows], feature_names=[f"V{j + 1}" for j in range(X.shape[1])][::-1]), list(new))
    # refusals: RANK models, and CLASSIFICATION models that predict through the probit link
    rank = copy.deepcopy(fit)
    rank["Model"]["model.control"] = fm.model_control("RANK", **{"factor.number": k})
    with pytest.raises(ValueError):
        fm.fm_fold_in(rank, fm.fm_matrix(X[fold_rows], y[fold_rows]), list(new))
    ycls = np.where(y > 3, 1.0, 0.0)
    for solver in (fm.ALS_solver(), fm.MCMC_solver()):
        probit = copy.deepcopy(fit)
        probit["Model"]["model.control"] = fm.model_control("CLASSIFICATION", **{"factor.number": k})
        probit["Model"]["solver.control"] = fm.solver_control(max_iter=5, solver=solver)
        with pytest.raises(ValueError):
            fm.fm_fold_in(probit, fm.fm_matrix(X[fold_rows], ycls[fold_rows]), list(new))
    logit = copy.deepcopy(fit)
    logit["Model"]["model.control"] = fm.model_control("CLASSIFICATION", **{"factor.number": k})
    logit["Model"]["solver.control"] = fm.solver_control(max_iter=5, solver=fm.SGD_solver())
    out = fm.fm_fold_in(logit, fm.fm_matrix(X[fold_rows], ycls[fold_rows]), list(new))               # labels 0 / 1 are mapped as fm_train maps them
    assert not out["fold.in"]["status"].any()
