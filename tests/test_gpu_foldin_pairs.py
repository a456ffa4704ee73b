"""fmx_fold_in_pairs / Engine.fold_in_pairs / fm_fold_in_rank: the rows of new users and items of a RANKING model solved against the frozen
model from preference pairs.  The yardstick is tests/foldin_pairs_model.py in np.longdouble; the bar is the project's
fp64 bar 1e-11 relative to a feature's max |theta|, which presupposes the fp64 model's own spread on the same inputs to be <= 1e-13
(asserted in tests/test_foldin_pairs_cpu.py)."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from tests import foldin_model as M
from tests import foldin_pairs_model as P

pytestmark = pytest.mark.gpu

KINDS = ["mb32", "mb32_wir", "mb64"]
BAR = 1e-11


def _record(line):
    """every measured figure is printed (pytest -s) and, with FMX_FOLDIN_REPORT set to a path, appended to that file: profiles/foldin_pairs.txt quotes such a run"""
    print(line)
    path = os.environ.get("FMX_FOLDIN_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _engine(kind, p, k, monkeypatch, k1=1, task=None, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    return engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), num_factor=k,
                         task=L.TASK_RANKING if task is None else task, keep_w1=k1, **kw)


def _matrix(inp, y=None):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], inp["p"], y)


def _theta(w, v):
    return np.concatenate([w[:, None], v.T], axis=1)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _bits(a, b):
    """the same BIT PATTERNS (a -0.0 is not a +0.0, a NaN is itself)"""
    return all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() for x, y in zip(a, b))


def _case(kind, k, valued, monkeypatch, lw=None, lv=None, k1=1, n_newton=8):
    inp = P.inputs(valued, k)
    w0, w, v = M.model_params(inp["p"], k)
    lam = P.case_lambda(k, valued)
    lw, lv = lam if lw is None else lw, lam if lv is None else lv
    e = _engine(kind, inp["p"], k, monkeypatch, k1)
    if kind == "mb32_wir":
        assert e.w_in_row()
    e.set_params(w0, w, v)
    gw, gv, pairs, status = e.fold_in_pairs(_matrix(inp), inp["ids"], lw, lv, newton_steps=n_newton)
    ref, rpairs, rstatus = P.reference(valued, k, lw, lv, k1, n_newton)
    assert np.array_equal(pairs, rpairs) and np.array_equal(pairs, inp["sizes"])          # out_pairs: exact
    assert np.array_equal(status, rstatus) and not status.any()
    err = M.rel_err(_theta(gw, gv), ref)
    _record(f"pair fold-in {kind} k={k} valued={valued} lw={lw} lv={lv} k1={k1} newton={n_newton}: error {err:.3g}")
    if not k1:
        assert np.all(gw == 0)
    return err


@pytest.mark.parametrize("valued", [False, True])
@pytest.mark.parametrize("k", P.KS)
def test_parity_fp32_tables(k, valued, monkeypatch):
    assert _case("mb32", k, valued, monkeypatch) <= BAR


@pytest.mark.parametrize("kind,k,valued", [("mb64", 0, True), ("mb64", 17, True), ("mb64", 33, False), ("mb64", 64, True), ("mb32_wir", 16, True),
                                           ("mb32_wir", 2, False), ("mb32_wir", 16, False), ("mb32_wir", 2, True)])
def test_parity_table_and_layout_forms(kind, k, valued, monkeypatch):
    assert _case(kind, k, valued, monkeypatch) <= BAR


@pytest.mark.parametrize("form", ["no_w1", "lambdas"])
def test_parity_keep_w1_and_unequal_lambdas(form, monkeypatch):
    kw = {"no_w1": dict(k1=0), "lambdas": dict(lw=0.03, lv=0.7)}[form]
    for kind in ("mb32", "mb64"):
        assert _case(kind, 16, True, monkeypatch, **kw) <= BAR


@pytest.mark.parametrize("k", [16, 33])
def test_first_newton_step(k, monkeypatch):
    assert _case("mb32", k, True, monkeypatch, n_newton=1) <= BAR


# ------------------------------------------------------------------------------------------------ guarantee 5: consistency with fmx_fold_in

def _pairs_of_rows(inp, first):
    """the pair matrix whose pair t holds row t of the row matrix `inp` as its row 2t (first[t]) or 2t + 1, the other row empty"""
    lens = np.diff(inp["rp"])
    plens = np.zeros(2 * len(lens), np.int64)
    plens[2 * np.arange(len(lens)) + np.where(first, 0, 1)] = lens
    return {"rp": np.concatenate([[0], np.cumsum(plens)]).astype(np.int64), "col": inp["col"], "val": inp["val"], "p": inp["p"]}


@pytest.mark.parametrize("kind", ["mb32", "mb64"])
@pytest.mark.parametrize("k", [2, 16, 64])
@pytest.mark.parametrize("orientation", ["preferred", "other", "mixed"])
def test_pairs_with_an_empty_row_are_fmx_fold_in_bit_for_bit(orientation, k, kind, monkeypatch):
    """rows 2t + 1 empty <-> the rows 2t with labels +1; rows 2t empty <-> the rows 2t + 1 with labels -1; and both in one matrix (the
    planted labels of the row tests): the same bits as fmx_fold_in on a CLASSIFICATION engine with the same tables and keep_w0 = 0"""
    from fmwr_amd import _lib as L
    inp = M.inputs(True)
    w0, w, v = M.model_params(inp["p"], k)
    y = {"preferred": np.ones(inp["n"], np.float32), "other": -np.ones(inp["n"], np.float32), "mixed": M.targets(True, k, M.LOGISTIC)}[orientation]
    cls = _engine(kind, inp["p"], k, monkeypatch, task=L.TASK_CLASSIFICATION, keep_w0=0)
    rank = _engine(kind, inp["p"], k, monkeypatch)
    for e in (cls, rank):
        e.set_params(w0, w, v)
    lam = 1.0   # (one-sided labels are a separable problem: a strong ridge keeps eight undamped steps finite; the comparison is of bits either way)
    rows = cls.fold_in(_matrix(inp, y), inp["ids"], lam, lam)
    pairs = rank.fold_in_pairs(_matrix(_pairs_of_rows(inp, y > 0)), inp["ids"], lam, lam)
    assert not rows[3].any() and np.all(np.isfinite(rows[0])) and np.array_equal(rows[2], inp["sizes"])
    assert _bits(rows, pairs)


# ------------------------------------------------------------------------------------------------ guarantees 2 and 3

@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_bits_do_not_depend_on_company_order_call_slab_current_rows_or_w0(kind, monkeypatch):
    from fmwr_amd import _lib as L
    k = 17
    inp = P.inputs(True, k)
    ids = inp["ids"]
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch)
    e.set_params(w0, w, v)
    m = _matrix(inp)
    full = e.fold_in_pairs(m, ids, 0.1, 0.1)
    assert not full[3].any()
    assert _bits(full, e.fold_in_pairs(m, ids, 0.1, 0.1))                 # a second call
    perm = np.random.default_rng(3).permutation(len(ids))
    got = e.fold_in_pairs(m, ids[perm], 0.1, 0.1)                         # ids permuted
    assert _bits((full[0][perm], full[1][:, perm], full[2][perm], full[3][perm]), got)
    for g in range(len(ids)):                                             # each group alone: the other fold columns are then ordinary features of pairs that are ignored
        one = e.fold_in_pairs(m, ids[g:g + 1], 0.1, 0.1)
        assert _bits((full[0][g:g + 1], full[1][:, g:g + 1], full[2][g:g + 1], full[3][g:g + 1]), one), g
    sub = np.array([len(ids) - 1, 3, 9])
    assert _bits((full[0][sub], full[1][:, sub], full[2][sub], full[3][sub]), e.fold_in_pairs(m, ids[sub], 0.1, 0.1))
    L.check(L.lib().fmx_debug_foldin_slab(C.c_int64(700), C.c_int64(3)))  # the next call: slabs of at most 700 pairs and 3 groups
    assert _bits(full, e.fold_in_pairs(m, ids, 0.1, 0.1))
    # the fold features' current rows never enter: large values, then NaN
    before = e.get_params()
    e.set_rows(ids, np.full(len(ids), 1e30), np.full((k, len(ids)), -3e28))
    assert _bits(full, e.fold_in_pairs(m, ids, 0.1, 0.1))
    e.set_rows(ids, np.full(len(ids), np.nan), np.full((k, len(ids)), np.nan))
    assert _bits(full, e.fold_in_pairs(m, ids, 0.1, 0.1))
    e.set_rows(ids, before[1][ids], before[2][:, ids])
    after = e.get_params()                                                # apply = 0 modifies nothing
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    for other_w0 in (w0 + 1.5, 1e300, np.nan):                            # w0 cancels in every pair and is never read
        e.set_params(other_w0, w, v)
        assert _bits(full, e.fold_in_pairs(m, ids, 0.1, 0.1))


# ------------------------------------------------------------------------------------------------ apply

@pytest.mark.parametrize("kind", KINDS)
def test_apply_writes_the_rows_as_set_rows_and_nothing_else(kind, tmp_path, monkeypatch):
    from fmwr_amd import _lib as L
    k = 16
    inp = P.inputs(True, k)
    ids = inp["ids"]
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch, solver=L.SOLVER_FTRL, l1_w1=1e-3, l1_v=1e-4, l2_w1=1e-2, l2_v=1e-2)
    e.set_params(0.0, w, v)
    m = _matrix(inp, np.ones(inp["n"], np.float32))
    e.train(m, 1024)                                                      # optimiser tables that are not all zero
    e.sync()
    p0 = e.get_params()
    e.save(tmp_path / "before.ckpt")
    dry = e.fold_in_pairs(m, ids, 0.1, 0.1, apply=False)
    p1 = e.get_params()
    assert p1[0] == p0[0] and p1[1].tobytes() == p0[1].tobytes() and p1[2].tobytes() == p0[2].tobytes()
    got = e.fold_in_pairs(m, ids, 0.1, 0.1, apply=True)
    assert _bits(dry, got) and not got[3].any()
    rw, rv = e.get_rows(ids)
    state = np.float32 if kind != "mb64" else np.float64
    assert np.array_equal(rw, got[0].astype(state).astype(np.float64)) and np.array_equal(rv, got[1].astype(state).astype(np.float64))
    p2 = e.get_params()
    others = np.setdiff1d(np.arange(inp["p"]), ids)
    assert p2[0] == p0[0] and np.array_equal(p2[1][others], p0[1][others]) and np.array_equal(p2[2][:, others], p0[2][:, others])
    e.set_rows(ids, p0[1][ids], p0[2][:, ids])                            # the fold rows back: the checkpoint (parameters, scalars, optimiser
    e.save(tmp_path / "after.ckpt")                                       # tables) is then the one from before, byte for byte
    assert (tmp_path / "after.ckpt").read_bytes() == (tmp_path / "before.ckpt").read_bytes()


def test_multi_gpu_engine_reads_its_primary_replica_and_apply_goes_through_set_rows(monkeypatch):
    """(that every replica follows is fmx_set_rows' own contract, which apply goes through, and its tests')"""
    k = 16
    inp = P.inputs(True, k)
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine("mb32", inp["p"], k, monkeypatch, n_gpus=2, gpus_share_device=1)
    assert e.group_info()["replicas"] == 2
    e.set_params(w0, w, v)
    gw, gv, pairs, status = e.fold_in_pairs(_matrix(inp), inp["ids"], 0.1, 0.1, apply=True)
    assert M.rel_err(_theta(gw, gv), P.reference(True, k)[0]) <= BAR
    rw, rv = e.get_rows(inp["ids"])
    assert np.array_equal(rw, gw.astype(np.float32).astype(np.float64)) and np.array_equal(rv, gv.astype(np.float32).astype(np.float64))
    one = _engine("mb32", inp["p"], k, monkeypatch)
    one.set_params(w0, w, v)
    assert _bits((gw, gv, pairs, status), one.fold_in_pairs(_matrix(inp), inp["ids"], 0.1, 0.1))


# ------------------------------------------------------------------------------------------------ exact properties

@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_new_users_w_is_exactly_zero_and_lambda_w_zero_fails_their_pivot(kind, monkeypatch):
    k = 16
    inp = P.inputs(False, k)                                              # one-hot: the user-like groups are all U
    ids, sizes = inp["ids"], inp["sizes"]
    users = np.array([g for g in range(len(ids)) if P.user_like(g)])
    items = np.setdiff1d(np.arange(len(ids)), users)
    w0, w, v = M.model_params(inp["p"], k)
    e = _engine(kind, inp["p"], k, monkeypatch)
    e.set_params(w0, w, v)
    m = _matrix(inp)
    gw, gv, pairs, status = e.fold_in_pairs(m, ids, 0.1, 0.1)
    assert not status.any() and np.all(gw[users] == 0.0) and np.all(gw[items[sizes[items] > 0]] != 0.0)
    empty = list(sizes).index(0)                                          # no pair, positive lambdas: theta = 0, solved
    assert pairs[empty] == 0 and status[empty] == 0 and gw[empty] == 0 and np.all(gv[:, empty] == 0)
    # lambda_w = 0: Z_t[0] = 0 exactly in every pair of a user, so the first pivot is exactly 0 -- status 1, NaN, and apply leaves the row alone
    before = e.get_rows(ids)
    gw, gv, pairs, status = e.fold_in_pairs(m, ids, 0.0, 0.1, apply=True)
    # (an item-like group without pairs has pivot lambda_w = 0 too)
    failed = np.array([g for g in range(len(ids)) if P.user_like(g) or sizes[g] == 0])
    solved = np.setdiff1d(np.arange(len(ids)), failed)
    assert np.all(status[failed] == 1) and not status[solved].any() and np.array_equal(pairs, sizes)
    assert np.all(np.isnan(gw[failed])) and np.all(np.isnan(gv[:, failed])) and np.all(np.isfinite(gw[solved])) and np.all(np.isfinite(gv[:, solved]))
    after = e.get_rows(ids)
    assert np.array_equal(after[0][failed], before[0][failed]) and np.array_equal(after[1][:, failed], before[1][:, failed])
    state = np.float32 if kind == "mb32" else np.float64
    assert np.array_equal(after[0][solved], gw[solved].astype(state).astype(np.float64))
    assert np.array_equal(after[1][:, solved], gv[:, solved].astype(state).astype(np.float64))
    ref = P.reference(False, k, 0.0, 0.1)
    assert np.array_equal(ref[2], status) and M.rel_err(_theta(gw, gv)[solved], ref[0][solved]) <= BAR
    # keep_w1 = 0: w_u is not a variable, and a user-side fold-in needs no lambda_w
    e0 = _engine(kind, inp["p"], k, monkeypatch, k1=0)
    e0.set_params(w0, w, v)
    gw, gv, pairs, status = e0.fold_in_pairs(m, ids, 0.0, 0.1)
    assert not status.any() and np.all(gw == 0.0)


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_touch_nothing(monkeypatch):
    from fmwr_amd import _lib as L, engine
    k = 8
    inp = P.inputs(True, k)
    p, ids = inp["p"], inp["ids"]
    w0, w, v = M.model_params(p, k)
    rank = _engine("mb32", p, k, monkeypatch)
    cls = _engine("mb32", p, k, monkeypatch, task=L.TASK_CLASSIFICATION)
    reg = _engine("mb32", p, k, monkeypatch, task=L.TASK_REGRESSION)
    wide = _engine("mb64", p, 65, monkeypatch)
    for e in (rank, cls, reg):
        e.set_params(w0, w, v)
    m = _matrix(inp)
    other_p = engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], p + 1)
    odd = engine.Matrix.from_csr(inp["rp"][:-1], inp["col"][:inp["rp"][-2]], inp["val"][:inp["rp"][-2]], p)

    def appended(cols_a, cols_b):
        """the matrix with one more pair: rows of the given columns, values 1"""
        rp2 = np.concatenate([inp["rp"], [inp["rp"][-1] + len(cols_a), inp["rp"][-1] + len(cols_a) + len(cols_b)]])
        extra = list(cols_a) + list(cols_b)
        return engine.Matrix.from_csr(rp2, np.concatenate([inp["col"], extra]).astype(np.uint32), np.concatenate([inp["val"], np.ones(len(extra))]).astype(np.float32), p)

    two = appended([5, ids[3], ids[4]], [7])                               # a row with two fold features
    twice = appended([5], [ids[3], 9, ids[3]])                             # a row with the same fold column stored twice
    mixed = appended([5, ids[3]], [ids[4], 7])                             # a pair whose rows hold different fold features

    def refused(e, mat, idl, lw=0.1, lv=0.1, newton=8, apply=1):
        idl = np.ascontiguousarray(idl, np.uint32)
        n = len(idl)
        ow = np.full(max(n, 1), 7.0); ov = np.full(max(n * max(e.k, 1), 1), 7.0)
        opairs = np.full(max(n, 1), 7, np.int64); ost = np.full(max(n, 1), 7, np.int32)
        params = e.get_params()
        st = L.lib().fmx_fold_in_pairs(e.h, mat.h, idl.ctypes.data_as(C.c_void_p), n, lw, lv, newton, apply, ow.ctypes.data_as(C.c_void_p),
                                       ov.ctypes.data_as(C.c_void_p), opairs.ctypes.data_as(C.c_void_p), ost.ctypes.data_as(C.c_void_p))
        msg = L.lib().fmx_last_error().decode()
        after = e.get_params()
        untouched = (np.all(ow == 7) and np.all(ov == 7) and np.all(opairs == 7) and np.all(ost == 7) and after[0] == params[0]
                     and after[1].tobytes() == params[1].tobytes() and after[2].tobytes() == params[2].tobytes())
        return st, untouched, msg

    cases = {
        "p mismatch": (rank, other_p, ids), "odd row count": (rank, odd, ids), "CLASSIFICATION engine": (cls, m, ids), "REGRESSION engine": (reg, m, ids),
        "more than 64 factors": (wide, m, ids), "id >= p": (rank, m, [ids[0], p]), "id twice": (rank, m, [ids[0], ids[1], ids[0]]),
        "negative lambda_w": (rank, m, ids, -0.1, 0.1), "negative lambda_v": (rank, m, ids, 0.1, -1e-300), "NaN lambda_w": (rank, m, ids, np.nan, 0.1),
        "NaN lambda_v": (rank, m, ids, 0.1, np.nan), "n_newton = 0": (rank, m, ids, 0.1, 0.1, 0), "n_newton < 0": (rank, m, ids, 0.1, 0.1, -3),
        "two fold features in a row": (rank, two, ids), "one fold column twice in a row": (rank, twice, ids),
        "different fold features in the rows of a pair": (rank, mixed, ids),
    }
    for name, args in cases.items():
        st, untouched, msg = refused(*args)
        assert st == L.ERR_INVALID and untouched and msg, name
        if "engine" in name:
            assert "fmx_fold_in" in msg.replace("fmx_fold_in_pairs", ""), msg      # it points to the call that solves such an engine
    for e_h, m_h in ((None, m.h), (rank.h, None)):
        assert L.lib().fmx_fold_in_pairs(e_h, m_h, ids.ctypes.data_as(C.c_void_p), len(ids), 0.1, 0.1, 8, 0, None, None, None, None) == L.ERR_INVALID
    # not refusals: no ids (nothing written), the offending rows' columns not folded, a matrix with labels of any kind
    st, untouched, _ = refused(rank, m, [])
    assert st == L.OK and untouched
    assert not rank.fold_in_pairs(two, ids[:3], 0.1, 0.1)[3].any()
    assert not rank.fold_in_pairs(mixed, ids[:4], 0.1, 0.1)[3].any()
    labelled = _matrix(inp, np.full(inp["n"], 0.25, np.float32))
    assert _bits(rank.fold_in_pairs(labelled, ids, 0.1, 0.1), rank.fold_in_pairs(m, ids, 0.1, 0.1))
    # fmx_fold_in keeps refusing RANKING engines
    assert L.lib().fmx_fold_in(rank.h, labelled.h, ids.ctypes.data_as(C.c_void_p), len(ids), 0.1, 0.1, 8, 0, None, None, None, None) == L.ERR_INVALID
    if L.lib().fmx_device_count is not None:
        cnt = C.c_int32()
        L.check(L.lib().fmx_device_count(C.byref(cnt)))
        if cnt.value > 1:                                                  # a matrix on another device
            far = engine.Matrix.from_csr(inp["rp"], inp["col"], inp["val"], p, device=1)
            st, untouched, _ = refused(rank, far, ids)
            assert st == L.ERR_INVALID and untouched


# ------------------------------------------------------------------------------------------------ fm_fold_in_rank

def test_fm_fold_in_rank_end_to_end():
    """The planted cold-start problem of tests/test_foldin_pairs_cpu.py: the FM object is built by hand from the planted item rows, the 40
    new users' rows zero; no training is involved."""
    import copy
    import scipy.sparse as sp
    import fmwr_amd as fm
    cs = P.cold_start(0)
    p, nu, ni = cs["p"], P.CS_USERS, P.CS_ITEMS
    users = ni + np.arange(nu)
    ctx = fm.fm_matrix(sp.csr_matrix((np.ones(nu), (np.arange(nu), users)), shape=(nu, p)))
    items = fm.fm_matrix(sp.csr_matrix((np.ones(ni), (np.arange(ni), np.arange(ni))), shape=(ni, p)))
    model, solver, track = fm.model_control("RANK", **{"factor.number": P.CS_K}), fm.solver_control(solver=fm.SGD_solver()), fm.track_control()
    fit = {"class": "FM", "Model": {"w0": 0.0, "w": cs["w"].copy(), "v": cs["v"].copy(), "model.control": model, "solver.control": solver,
                                    "track.control": track, "convergence": False},
           "Scales": {"mean": None, "std": None, "model.vars": list(ctx.feature_names), "target.range": (-1.0, 1.0)},
           "engine": {"mode": "minibatch", "batch_rows": 256, "device": 0}}
    keep = copy.deepcopy(fit)
    train, held = [r for r in cs["train"]], [r for r in cs["held"]]
    folded = fm.fm_fold_in_rank(fit, ctx, items, train, list(users), n_neg=P.CS_NEG, l2_w=0.1, l2_v=0.1, newton_steps=8, seed=0)
    assert folded is not fit and "fold.in" not in fit                      # the input object is untouched
    assert np.array_equal(fit["Model"]["w"], keep["Model"]["w"]) and np.array_equal(fit["Model"]["v"], keep["Model"]["v"])
    info = folded["fold.in"]
    assert info["features"] == [f"V{j + 1}" for j in users] and np.array_equal(info["pairs"], np.full(nu, P.CS_TRAIN * P.CS_NEG)) and not info["status"].any()
    assert np.array_equal(folded["Model"]["w"][:ni], fit["Model"]["w"][:ni]) and np.array_equal(folded["Model"]["v"][:, :ni], fit["Model"]["v"][:, :ni])
    assert np.all(folded["Model"]["w"][users] == 0.0) and np.all(np.any(folded["Model"]["v"][:, users] != 0, axis=0))
    auc = lambda f: fm.fm_recommend_metrics(f, ctx, items, held, k=10, exclude=train, normalize=False)["auc"]
    before, after = auc(fit), auc(folded)
    _record(f"fm_fold_in_rank: held-out AUC unfolded {before:.4f}, folded {after:.4f}")
    assert after >= before + 0.10
    by_name = fm.fm_fold_in_rank(fit, ctx, items, train, [f"V{j + 1}" for j in users], n_neg=P.CS_NEG)
    assert np.array_equal(by_name["Model"]["w"], folded["Model"]["w"]) and np.array_equal(by_name["Model"]["v"], folded["Model"]["v"])
    # status 1 keeps the old row and warns: a user-side fold-in with l2_w = 0
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        part = fm.fm_fold_in_rank(fit, ctx, items, train, [int(users[0])], n_neg=P.CS_NEG, l2_w=0.0)
    assert part["fold.in"]["status"][0] == 1 and np.all(part["Model"]["v"][:, users[0]] == 0) and any("could not be solved" in str(r.message) for r in rec)
    # a new item: the contexts are the (folded) users, the item's pairs are those where it is the positive or a sampled negative
    new_item = int(cs["train"][0][0])
    cold = copy.deepcopy(folded)
    cold["Model"]["w"][new_item] = 0.0
    cold["Model"]["v"][:, new_item] = 0.0
    warm = fm.fm_fold_in_rank(cold, ctx, items, train, [new_item], n_neg=P.CS_NEG)
    assert warm["fold.in"]["status"][0] == 0 and warm["fold.in"]["pairs"][0] >= P.CS_NEG and np.any(warm["Model"]["v"][:, new_item] != 0)
    # a new user and a new item that meet in one row: the advisory error
    with pytest.raises(ValueError, match="separate calls"):
        fm.fm_fold_in_rank(fit, ctx, items, train, [int(users[0]), new_item], n_neg=P.CS_NEG)
    # refusals: models of other tasks (with a pointer to fm_fold_in), columns in another order
    for task in ("REGRESSION", "CLASSIFICATION"):
        other = copy.deepcopy(fit)
        other["Model"]["model.control"] = fm.model_control(task, **{"factor.number": P.CS_K})
        with pytest.raises(ValueError, match="fm_fold_in"):
            fm.fm_fold_in_rank(other, ctx, items, train, list(users))
    with pytest.raises(ValueError):
        fm.fm_fold_in_rank(fit, fm.fm_matrix(sp.csr_matrix((np.ones(nu), (np.arange(nu), users)), shape=(nu, p)), feature_names=list(ctx.feature_names)[::-1]),
                           items, train, list(users))
