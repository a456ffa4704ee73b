"""FMX_TASK_RANKING (BPR on pair matrices): the device sampler fmx_matrix_pairs, the pair step against the oracle's
update from numpy-formed pair sums, w0 untouched, the forms of phase 1, the refusals, the pair metrics, and fm_train_rank learning a planted
preference structure."""
import ctypes as C
import os
import struct

import numpy as np
import pytest
import scipy.sparse as sp

import oracle

pytestmark = pytest.mark.gpu

KINDS = ["mb64", "mb32", "mb32_wir"]


def _L():
    from fmwr_amd import _lib as L
    return L


def _engine(kind, p, k, monkeypatch, solver="sgd", **kw):
    from fmwr_amd import engine
    L = _L()
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    opts = dict(task=L.TASK_RANKING, solver=L.SOLVER_SGD if solver == "sgd" else L.SOLVER_FTRL, num_factor=k, mode=L.MODE_MINIBATCH,
                state_fp64=int(kind == "mb64"), batch_rows=64)
    opts.update(kw)
    return engine.Engine(p, **opts)


def _csr(rows, p, rng, lo=1):
    """CSR of the given lists of column ids, normal values (a length-0 list is allowed)"""
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    return rp, col, val


def _ctx_items(n_ctx, n_items, rng, extra=6):
    """context c holds feature c (value 1) and up to `extra` shared features; item i holds feature n_ctx + extra + i (value 1) and a shared
    item feature -- so every exported row names its context and item"""
    p = n_ctx + extra + n_items + 3
    crows, irows = [], []
    for c in range(n_ctx):
        crows.append([c] + sorted(rng.choice(extra, rng.integers(0, extra + 1), replace=False) + n_ctx))
    for i in range(n_items):
        irows.append([n_ctx + extra + i] + sorted(rng.choice(3, rng.integers(0, 2), replace=False) + n_ctx + extra + n_items))
    C_ = _csr(crows, p, rng); I_ = _csr(irows, p, rng)
    C_[2][C_[0][:-1]] = 1.0; I_[2][I_[0][:-1]] = 1.0
    return p, C_, I_


def _dev(m, p, y=None):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p, y)


def _pos_matrix(lists, n_items):
    from fmwr_amd import engine
    rp = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(r, np.int64) for r in lists]).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    return engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), n_items)


def _pairs(C_, I_, p, lists, n_items, n_neg, seed, epoch):
    from fmwr_amd import engine
    return engine.Matrix.pairs(_dev(C_, p), _dev(I_, p), _pos_matrix(lists, n_items), n_neg, seed, epoch)


# ------------------------------------------------------------------------------------------------ sampler
def _parse(pm, n_ctx, n_items, extra, C_, I_):
    rp, col, val, y = pm.export()
    out = []
    for r in range(pm.n):
        cc, vv = col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]
        c = int(cc[0])
        lc = int(C_[0][c + 1] - C_[0][c])
        assert np.array_equal(cc[:lc], C_[1][C_[0][c]:C_[0][c + 1]]) and np.array_equal(vv[:lc], C_[2][C_[0][c]:C_[0][c + 1]])
        it = int(cc[lc]) - n_ctx - extra
        assert 0 <= it < n_items
        assert np.array_equal(cc[lc:], I_[1][I_[0][it]:I_[0][it + 1]]) and np.array_equal(vv[lc:], I_[2][I_[0][it]:I_[0][it + 1]])
        out.append((c, it))
    assert np.all(y == 1.0)
    return out


def test_sampler_rows_counts_and_determinism():
    rng = np.random.default_rng(1)
    n_ctx, n_items, extra = 40, 30, 6
    p, C_, I_ = _ctx_items(n_ctx, n_items, rng, extra)
    lists = [list(rng.integers(0, n_items, rng.integers(0, 6))) for _ in range(n_ctx)]
    lists[3] = [5, 5, 7, 5]                    # duplicates count once
    lists[4] = [i for i in range(n_items) if i != 11] * 2   # all items but one: every negative is item 11
    n_neg = 3
    pm = _pairs(C_, I_, p, lists, n_items, n_neg, seed=9, epoch=0)
    distinct = {(c, i) for c, l in enumerate(lists) for i in set(l)}
    assert pm.n == 2 * n_neg * len(distinct)
    rows = _parse(pm, n_ctx, n_items, extra, C_, I_)
    count = {}
    for t in range(pm.n // 2):
        (c, i), (c2, j) = rows[2 * t], rows[2 * t + 1]
        assert c == c2 and i in set(lists[c]) and j not in set(lists[c])
        if c == 4:
            assert j == 11
        count[(c, i)] = count.get((c, i), 0) + 1
    assert set(count) == distinct and all(v == n_neg for v in count.values())
    # same seed and epoch: same bits; another epoch: other negatives and order
    again = _pairs(C_, I_, p, lists, n_items, n_neg, seed=9, epoch=0)
    a, b = pm.export(), again.export()
    assert all(np.array_equal(x, z) for x, z in zip(a, b))
    other = _pairs(C_, I_, p, lists, n_items, n_neg, seed=9, epoch=1)
    o = other.export()
    assert other.n == pm.n and not np.array_equal(o[1], a[1])
    # a context that holds every item is refused
    bad = [list(range(n_items))] + lists[1:]
    from fmwr_amd import _lib as L
    with pytest.raises(L.FmxError) as ei:
        _pairs(C_, I_, p, bad, n_items, 1, 0, 0)
    assert ei.value.status == L.ERR_INVALID


def test_sampler_negatives_are_uniform():
    rng = np.random.default_rng(2)
    n_items, n_neg = 21, 4000
    p, C_, I_ = _ctx_items(2, n_items, rng, 2)
    lists = [[3], [0, 20]]
    pm = _pairs(C_, I_, p, lists, n_items, n_neg, seed=1234, epoch=0)
    rows = _parse(pm, 2, n_items, 2, C_, I_)
    neg = np.array([rows[2 * t + 1] for t in range(pm.n // 2)])
    for c, l in enumerate(lists):
        j = neg[neg[:, 0] == c, 1]
        allowed = [i for i in range(n_items) if i not in l]
        assert set(j) <= set(allowed)
        obs = np.bincount(j, minlength=n_items)[allowed]
        exp = len(j) / len(allowed)
        chi2 = ((obs - exp) ** 2 / exp).sum()
        assert chi2 < 3.0 * len(allowed), (c, chi2)   # loose: the 0.999 quantile of chi2(19) is 43.8, of chi2(18) 42.3


def test_sampler_empty_positives_make_an_empty_matrix():
    rng = np.random.default_rng(3)
    p, C_, I_ = _ctx_items(3, 4, rng)
    pm = _pairs(C_, I_, p, [[], [], []], 4, 2, 0, 0)
    assert pm.n == 0 and pm.nnz == 0


# ------------------------------------------------------------------------------------------------ step vs oracle
def _oracle_pair_step(P, st, X, rows, k, p):
    """one BPR step over the pairs held in `rows` (a list of row ranges) from the oracle's forward, the sums formed as fmo_batch_sums forms them"""
    yh = oracle.predict_batch(P, X, st["w0"].value, st["w"], st["v"])
    v = st["v"].reshape(k, p)
    acc = dict(G0=0.0, Q0=0.0, Gw=np.zeros(p), Qw=np.zeros(p), cw=np.zeros(p), Gv=np.zeros(k * p), Qv=np.zeros(k * p))
    B = 0
    for b0, b1 in rows:
        B += b1 - b0
        d = yh[b0:b1:2] - yh[b0 + 1:b1:2]
        m0 = -1.0 / (1.0 + np.exp(d))
        mult = np.empty(b1 - b0); mult[0::2] = m0; mult[1::2] = -m0
        for r in range(b0, b1):
            a, e = X.row_ptr[r], X.row_ptr[r + 1]
            cols, x = X.col[a:e].astype(np.int64), X.val[a:e].astype(np.float64)
            s = (v[:, cols] * x).sum(1)
            mu = mult[r - b0]
            g = mu * x
            np.add.at(acc["Gw"], cols, g); np.add.at(acc["Qw"], cols, g * g); np.add.at(acc["cw"], cols, 1.0)
            gv = mu * (s[:, None] * x[None, :] - v[:, cols] * (x * x)[None, :])   # [k][entries]
            at = (np.arange(k)[:, None] * p + cols[None, :]).ravel()
            np.add.at(acc["Gv"], at, gv.ravel()); np.add.at(acc["Qv"], at, (gv * gv).ravel())
    return acc, B, yh


def _state(solver, w, v, k, p):
    st = dict(w0=C.c_double(0.0), w=w.copy(), v=v.ravel().copy())
    if solver == "sgd":
        st.update(q_w=np.zeros(p), q_v=np.zeros(k * p), u=np.zeros(2))
    else:
        st.update(zn0=np.zeros(2), z_w=np.zeros(p), n_w=np.zeros(p), z_v=np.zeros(k * p), n_v=np.zeros(k * p))
    return st


def _pair_problem(n_pairs, p, rng):
    """a user-built pair matrix: random rows of 2..9 distinct ascending columns, normal values"""
    rows = [sorted(rng.choice(p, rng.integers(2, 10), replace=False)) for _ in range(2 * n_pairs)]
    return _csr(rows, p, rng)


def _run_vs_oracle(kind, solver, monkeypatch, k=4, batch=64, steps=4, reduce="mean", reg="l2", tile_rows=0, n_pairs=160, seed=0, env=None, big=False,
                   n_gpus=1):
    L = _L()
    rng = np.random.default_rng(seed)
    p = 300
    m = _pair_problem(n_pairs, p, rng)
    w = rng.normal(0, 0.1, p); v = rng.normal(0, 0.3, (k, p))
    if big:  # pair 0 with d ~ +50, pair 1 with d ~ -50 (multipliers -> -0 and -> -1)
        rp, col, val = m
        for r in (0, 3):
            val[rp[r]:rp[r + 1]] = 1.0
            w[col[rp[r]:rp[r + 1]]] += 50.0 / (rp[r + 1] - rp[r])
    hyper = dict(learn_rate=0.05)
    if reg == "l2":
        hyper.update(l2_w1=1e-3, l2_v=2e-3)
    else:
        hyper.update(l1_w1=1e-4, l1_v=2e-4)
    if solver == "ftrl":
        hyper.update(alpha_w=0.2, alpha_v=0.1, beta_w=1.0, beta_v=1.0)
    for key, val in (env or {}).items():
        monkeypatch.setenv(key, val)
    e = _engine(kind, p, k, monkeypatch, solver=solver, batch_rows=batch, tile_rows=tile_rows, batch_reduce=L.REDUCE_MEAN if reduce == "mean" else L.REDUCE_SUM,
                n_gpus=n_gpus, gpus_share_device=int(n_gpus > 1), **hyper)
    w0 = 0.625
    if kind != "mb64":  # the fp32 tables hold fp32 values: start the oracle from the same numbers
        w = w.astype(np.float32).astype(np.float64); v = v.astype(np.float32).astype(np.float64)
    e.set_params(w0, w, v)
    dm = _dev(m, p, np.ones(2 * n_pairs, np.float32))
    P = oracle.params(task=oracle.CLASSIFICATION, k=k, k0=False, learn_rate=0.05, batch_mean=reduce == "mean",
                      **({"l2_regw": 1e-3, "l2_regv": 2e-3} if reg == "l2" else {"l1_regw": 1e-4, "l1_regv": 2e-4}),
                      **({"alpha_w": 0.2, "alpha_v": 0.1} if solver == "ftrl" else {}))
    X = oracle.Matrix(m[0], m[1], m[2], p)
    st = _state(solver, w, v, k, p)
    n = 2 * n_pairs
    done = 0
    for s in range(steps):
        if n_gpus == 1:
            b0 = (s * batch) % n
            ranges = [(b0, min(b0 + batch, n))]
        else:  # shard r holds rows [r n / 2, (r + 1) n / 2); global step s = local batch s of each
            half = n // 2
            ranges = [(r * half + (s * batch) % half, r * half + min((s * batch) % half + batch, half)) for r in range(2)]
        acc, B, yh = _oracle_pair_step(P, st, X, ranges, k, p)
        (oracle.sgd_apply_sums if solver == "sgd" else oracle.ftrl_apply_sums)(P, p, st, float(B), acc)
        done += B
    e.train(dm, done)
    w0e, we, ve = e.get_params()
    return e, dm, (w0, w0e), (st["w"], we), (st["v"].reshape(k, p), ve), yh


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("solver", ["sgd", "ftrl"])
@pytest.mark.parametrize("reduce,reg", [("mean", "l2"), ("sum", "l1"), ("mean", "l1"), ("sum", "l2")])
def test_pair_step_matches_oracle(kind, solver, reduce, reg, monkeypatch):
    _, _, (w0, w0e), (w_o, w_e), (v_o, v_e), _ = _run_vs_oracle(kind, solver, monkeypatch, reduce=reduce, reg=reg, steps=5)
    tol = 1e-10 if kind == "mb64" else 1e-5
    assert w0e == w0  # bit for bit: w0 takes no step
    assert np.max(np.abs(w_e - w_o)) <= tol * max(1.0, np.max(np.abs(w_o)))
    assert np.max(np.abs(v_e - v_o)) <= tol * max(1.0, np.max(np.abs(v_o)))


@pytest.mark.parametrize("kind", KINDS)
def test_pair_step_extreme_differences(kind, monkeypatch):
    e, dm, (w0, w0e), (w_o, w_e), (v_o, v_e), yh = _run_vs_oracle(kind, "sgd", monkeypatch, big=True, steps=1, batch=64)
    d = yh[0::2] - yh[1::2]
    assert np.max(np.abs(d)) > 40  # the planted pairs are far apart
    assert np.all(np.isfinite(w_e)) and np.all(np.isfinite(v_e))
    tol = 1e-10 if kind == "mb64" else 1e-5
    assert np.max(np.abs(v_e - v_o)) <= tol * max(1.0, np.max(np.abs(v_o)))
    assert np.max(np.abs(w_e - w_o)) <= tol * max(1.0, np.max(np.abs(w_o)))


def _scalars(e, tmp_path, name):
    path = str(tmp_path / name)
    e.save(path)
    raw = open(path, "rb").read()
    return struct.unpack("<12d", raw[64:64 + 96])


@pytest.mark.parametrize("solver", ["sgd", "ftrl"])
def test_w0_and_its_state_stay_as_set(solver, monkeypatch, tmp_path):
    e, dm, (w0, w0e), _, _, _ = _run_vs_oracle("mb32", solver, monkeypatch, steps=3)
    before = _scalars(e, tmp_path, "a.fmx")
    assert before[0] == 0.625 and w0e == 0.625
    e.train(dm, dm.n)
    after = _scalars(e, tmp_path, "b.fmx")
    assert after[:3] == before[:3]        # w0, z0, n0 bit for bit
    assert after[5] == 0.0 and after[6] == 0.0   # SC_G0 / SC_Q0


# ------------------------------------------------------------------------------------------------ forms
@pytest.mark.parametrize("kind,k,batch", [("mb32", 4, 64),        # one-wave workgroups, four lane groups per row (SPLIT = 4)
                                          ("mb32", 64, 64),       # 16-lane rows: SPLIT = 4 would put one row in a workgroup -> SPLIT 1
                                          ("mb64", 128, 64),      # 64-lane rows in one-wave workgroups -> 256-thread workgroups
                                          ("mb64", 64, 4096),     # 256-thread workgroups (step rows x lanes >= 131072)
                                          ("mb32", 64, 8192)])    # the same, fp32
def test_forms_match_oracle(kind, k, batch, monkeypatch):
    n_pairs = max(160, batch)
    _, _, (w0, w0e), (w_o, w_e), (v_o, v_e), _ = _run_vs_oracle(kind, "sgd", monkeypatch, k=k, batch=batch, steps=2, n_pairs=n_pairs)
    tol = 1e-10 if kind == "mb64" else 1e-5
    assert w0e == w0
    assert np.max(np.abs(v_e - v_o)) <= tol * max(1.0, np.max(np.abs(v_o)))
    assert np.max(np.abs(w_e - w_o)) <= tol * max(1.0, np.max(np.abs(w_o)))


def _large_run(kind, monkeypatch, env):
    """three large FTRL steps (wide workgroups: the opt-in forms apply to pointwise steps of this size) on rows of differing lengths"""
    L = _L()
    for key in ("FMX_ROWS_PULL", "FMX_ROWS_FLAT"):
        monkeypatch.delenv(key, raising=False)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    rng = np.random.default_rng(8)
    p, k, n = 5000, 16, 1 << 16
    m = _pair_problem(n // 2, p, rng)
    e = _engine(kind, p, k, monkeypatch, solver="ftrl", batch_rows=n // 2, batch_reduce=L.REDUCE_SUM, alpha_v=0.05)
    e.set_params(0.0, rng.normal(0, 0.1, p), rng.normal(0, 0.3, (k, p)))
    dm = _dev(m, p, np.ones(n, np.float32))
    e.train(dm, n + n // 2)
    return e.get_params()


@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_opt_in_forms_and_tiles(kind, monkeypatch):
    ref = _large_run(kind, monkeypatch, {})
    for env in ({"FMX_ROWS_PULL": "1"}, {"FMX_ROWS_FLAT": "1"}):
        got = _large_run(kind, monkeypatch, env)
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), env   # ranking steps run the default form there: its bits
    monkeypatch.delenv("FMX_ROWS_FLAT", raising=False)
    tiled = _run_vs_oracle(kind, "ftrl", monkeypatch, batch=128, steps=3, reduce="sum", tile_rows=18)
    tol = 1e-10 if kind == "mb64" else 1e-5
    _, _, (w0, w0e), (w_o, w_e), (v_o, v_e), _ = tiled
    assert w0e == w0
    assert np.max(np.abs(v_e - v_o)) <= tol * max(1.0, np.max(np.abs(v_o)))
    assert np.max(np.abs(w_e - w_o)) <= tol * max(1.0, np.max(np.abs(w_o)))


@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_two_replicas_match_the_global_batch(kind, monkeypatch):
    _, _, (w0, w0e), (w_o, w_e), (v_o, v_e), _ = _run_vs_oracle(kind, "sgd", monkeypatch, batch=32, steps=5, n_pairs=160, n_gpus=2)
    tol = 1e-10 if kind == "mb64" else 1e-5
    assert w0e == w0
    assert np.max(np.abs(v_e - v_o)) <= tol * max(1.0, np.max(np.abs(v_o)))
    assert np.max(np.abs(w_e - w_o)) <= tol * max(1.0, np.max(np.abs(w_o)))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_parameters_untouched(monkeypatch):
    L = _L()
    lib = L.lib()
    rng = np.random.default_rng(5)
    p, k = 50, 4
    e = _engine("mb32", p, k, monkeypatch, batch_rows=8)
    e.set_params(0.5, rng.normal(size=p), rng.normal(size=(k, p)))
    before = e.get_params()
    odd = _dev(_csr([[1, 2], [3], [4, 5]], p, rng), p, np.ones(3, np.float32))
    even = _dev(_csr([[1, 2], [3], [4, 5], [6]], p, rng), p, np.ones(4, np.float32))
    nb = C.c_int64()
    tc = L.TrackConfig(C.sizeof(L.TrackConfig), L.EVAL_PAIR_ACC, 2, 1e-4, 0, 0)
    out = C.c_double(-7.0)
    calls = [lambda: lib.fmx_train(e.h, odd.h, C.c_int64(2), None),
             lambda: lib.fmx_train(e.h, even.h, C.c_int64(3), None),
             lambda: lib.fmx_num_batches(e.h, odd.h, C.byref(nb)),
             lambda: lib.fmx_step(e.h, odd.h, C.c_int64(0), C.c_int64(0)),
             lambda: lib.fmx_step(e.h, even.h, C.c_int64(0), C.c_int64(3)),
             lambda: lib.fmx_grad(e.h, even.h, C.c_int64(0), C.c_int64(1)),
             lambda: lib.fmx_grad_begin(e.h, even.h, C.c_int64(0), C.c_int64(3)),
             lambda: lib.fmx_grad_compact(e.h, even.h, C.c_int64(0), C.c_int64(1)),
             lambda: lib.fmx_train_tracked(e.h, even.h, C.c_int64(4), C.byref(tc), None, None),
             lambda: lib.fmx_evaluate(e.h, even.h, C.c_int(L.EVAL_LL), C.byref(out)),
             lambda: lib.fmx_evaluate(e.h, odd.h, C.c_int(L.EVAL_PAIR_ACC), C.byref(out))]
    for i, call in enumerate(calls):
        assert call() == L.ERR_INVALID, (i, lib.fmx_last_error().decode())
        assert lib.fmx_last_error().decode()
    assert out.value == -7.0
    after = e.get_params()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and np.array_equal(after[2], before[2])
    # the pair metrics on a pointwise engine
    from fmwr_amd import engine
    ec = engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=k, mode=L.MODE_MINIBATCH, batch_rows=8)
    assert lib.fmx_evaluate(ec.h, even.h, C.c_int(L.EVAL_BPR), C.byref(out)) == L.ERR_INVALID
    # a two-replica ranking engine refuses an odd matrix before it shards it
    e2 = _engine("mb32", p, k, monkeypatch, batch_rows=8, n_gpus=2, gpus_share_device=1)
    assert lib.fmx_train(e2.h, odd.h, C.c_int64(2), None) == L.ERR_INVALID


# ------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("kind", KINDS)
def test_pair_metrics_match_numpy(kind, monkeypatch):
    L = _L()
    rng = np.random.default_rng(6)
    p, k = 200, 8
    e = _engine(kind, p, k, monkeypatch)
    e.set_params(0.2, rng.normal(0, 1, p), rng.normal(0, 0.5, (k, p)))
    m = _pair_problem(500, p, rng)
    rp, col, val = m
    # ties: pairs 0..9 are a row and its copy (d = 0 exactly)
    rows = [(col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]) for r in range(len(rp) - 1)]
    for t in range(10):
        rows[2 * t + 1] = rows[2 * t]
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    col = np.concatenate([c for c, _ in rows]); val = np.concatenate([v for _, v in rows])
    dm = _dev((rp, col, val), p, np.ones(len(rp) - 1, np.float32))
    y = e.predict(dm, L.LINK_NONE)
    d = y[0::2] - y[1::2]
    assert np.all(d[:10] == 0.0)
    acc = np.mean(np.where(d > 0, 1.0, np.where(d == 0, 0.5, 0.0)))
    bpr = np.mean(np.logaddexp(0.0, -d))
    a1, b1 = e.evaluate(dm, L.EVAL_PAIR_ACC), e.evaluate(dm, L.EVAL_BPR)
    assert abs(a1 - acc) <= 1e-12 and abs(b1 - bpr) <= 1e-12 * max(1.0, bpr)
    a2, b2 = e.evaluate(dm, L.EVAL_PAIR_ACC), e.evaluate(dm, L.EVAL_BPR)
    assert a1 == a2 and b1 == b2


# ------------------------------------------------------------------------------------------------ it learns
def _planted(n_users=2000, n_items=500, k=8, top=20, held=2, seed=11):
    """users and items with planted factors and an item bias; positives = each user's `top` best items, `held` of them held out"""
    rng = np.random.default_rng(seed)
    U = rng.normal(0, 1, (n_users, k)); W = rng.normal(0, 1, (n_items, k)); b = rng.normal(0, 1.0, n_items)
    S = U @ W.T + b[None, :]
    best = np.argsort(-S, axis=1)[:, :top]
    train, test = [], []
    for u in range(n_users):
        sel = rng.permutation(top)
        test.append(list(best[u, sel[:held]])); train.append(list(best[u, sel[held:]]))
    import fmwr_amd as fm
    p = n_users + n_items
    ctx = sp.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, p))
    its = sp.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, p))
    return fm.fm_matrix(ctx), fm.fm_matrix(its), train, test


def test_fm_train_rank_learns_a_planted_order():
    import fmwr_amd as fm
    context, items, train, test = _planted()
    n_users, n_items = context.dim[0], items.dim[0]
    ctl = [fm.model_control("RANK", **{"factor.number": 16, "v.init_stdev": 0.1}), fm.solver_control(solver=fm.SGD_solver(learn_rate=0.1))]
    fit0 = fm.fm_train_rank(context, items, train, control=ctl, epochs=0, seed=3, batch_rows=4096)
    before = fm.fm_rank_evaluate(fit0, context, items, test, n_neg=4, seed=1)
    fit = fm.fm_train_rank(context, items, train, control=ctl, n_neg=2, epochs=30, seed=3, batch_rows=4096)
    after = fm.fm_rank_evaluate(fit, context, items, test, n_neg=4, seed=1)
    print("held-out pair_acc", before, "->", after)
    assert abs(before["pair_acc"] - 0.5) < 0.05
    assert after["pair_acc"] >= 0.8
    assert fit["Model"]["w0"] == 0.0 and fit["Model"]["model.control"]["task"] == "RANK"
    # fm_recommend with the training positives excluded beats item popularity on recall@10 of the held-out positives
    rec = fm.fm_recommend(fit, context, items, top_k=10, exclude=train, normalize=False)
    pop = np.bincount(np.concatenate([np.asarray(t) for t in train]), minlength=n_items)
    hit_m = hit_p = 0
    for u in range(n_users):
        seen = set(train[u])
        order = [i for i in np.argsort(-pop, kind="stable") if i not in seen][:10]
        hit_p += len(set(order) & set(test[u])); hit_m += len(set(rec["index"][u]) & set(test[u]))
    print("recall@10 model", hit_m / (2 * n_users), "popularity", hit_p / (2 * n_users))
    assert hit_m > hit_p
    # predict (raw scores), fm_explain's efficiency identity
    pairs = sp.hstack([sp.csr_matrix((np.ones(4), (np.arange(4), np.arange(4))), shape=(4, n_users)),
                       sp.csr_matrix((np.ones(4), (np.arange(4), [0, 1, 2, 3])), shape=(4, n_items))]).tocsr()
    nd = fm.fm_matrix(pairs)
    y = fm.predict(fit, nd, normalize=False)
    mdl = fit["Model"]
    X = oracle.Matrix(np.concatenate([[0], np.cumsum(nd.features["row_size"])]), nd.features["col_idx"], nd.features["value"], n_users + n_items)
    P = oracle.params(task=oracle.CLASSIFICATION, k=16)
    y_o = oracle.predict_batch(P, X, mdl["w0"], mdl["w"], mdl["v"].ravel())
    assert np.max(np.abs(y - y_o[:4])) <= 1e-10 * max(1.0, np.max(np.abs(y_o[:4])))
    ex = fm.fm_explain(fit, nd, normalize=False)
    assert np.max(np.abs(ex["intercept"] + np.asarray(ex["contrib"].sum(1)).ravel() - y)) <= 1e-9 * max(1.0, np.max(np.abs(y)))
