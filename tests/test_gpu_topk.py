"""fmx_topk: the K best item rows per context row under the FM score of the concatenated row c (+) i, checked against the oracle's
forward of c (+) i itself, under the total order (higher score first, ties by the lower item index, NaN last)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import oracle

pytestmark = pytest.mark.gpu


def _csr(n, lo, hi, nnz, rng, empty=()):
    """n rows of up to `nnz` distinct sorted columns in [lo, hi), random values; rows listed in `empty` hold nothing"""
    rows = []
    for r in range(n):
        m = 0 if r in empty else int(rng.integers(1, nnz + 1))
        rows.append(np.sort(rng.choice(np.arange(lo, hi), min(m, hi - lo), replace=False)))
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    return rp, col, val


def _row(m, r):
    rp, col, val = m
    return col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]


def _pairs(C, I):
    """the CSR of every concatenated row c (+) i, context-major"""
    nc, ni = len(C[0]) - 1, len(I[0]) - 1
    cols, vals, rp = [], [], [0]
    for c in range(nc):
        cc, cv = _row(C, c)
        for i in range(ni):
            ic, iv = _row(I, i)
            cols.append(np.concatenate([cc, ic])); vals.append(np.concatenate([cv, iv]))
            rp.append(rp[-1] + len(cc) + len(ic))
    return np.array(rp, np.int64), np.concatenate(cols).astype(np.uint32), np.concatenate(vals).astype(np.float32)


def _engine(kind, p, k, task=None, **kw):
    from fmwr_amd import _lib as L, engine
    task = L.TASK_REGRESSION if task is None else task
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=task, **kw)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=task, batch_rows=256, state_fp64=int(kind == "mb64"), **kw)
    rng = np.random.default_rng(k + 11)
    e.set_params(0.3, rng.normal(0, 0.5, p), rng.normal(0, 0.4, (k, p)))
    return e


def _mat(m, p):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _oracle(e, C, I, p):
    """oracle scores [nc][ni] of c (+) i from the engine's stored parameters, and the scale sum |terms| of each"""
    k = e.k
    w0, w, v = e.get_params()
    P = oracle.params(task=oracle.REGRESSION, k=k)
    rp, col, val = _pairs(C, I)
    X = oracle.Matrix(rp, col, val, p)
    y = oracle.predict_batch(P, X, w0, w, v.ravel())
    A = sp.csr_matrix((np.abs(val).astype(np.float64), col, rp), shape=(len(rp) - 1, p))
    scale = abs(w0) + A @ np.abs(w) + 0.5 * ((A @ np.abs(v).T) ** 2).sum(1) + 1e-300
    nc, ni = len(C[0]) - 1, len(I[0]) - 1
    return y.reshape(nc, ni), np.asarray(scale).reshape(nc, ni)


def _ranked(idx, score):
    """does each row follow the total order (higher score first, equal scores by the lower index, NaN last)?"""
    for r in range(idx.shape[0]):
        s, i = score[r], idx[r]
        order = np.lexsort((i, np.where(np.isnan(s), np.inf, -s)))
        if not np.array_equal(order, np.arange(len(i))):
            return False
    return True


RTOL = {"seq64": 1e-12, "mb64": 1e-12, "mb32": 1e-5}


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
@pytest.mark.parametrize("k", [0, 1, 3, 8, 16, 64, 100])
def test_full_ranking_scores_equal_the_oracle_of_the_concatenated_rows(kind, k):
    rng = np.random.default_rng(k)
    p, nc, ni = 80, 6, 41
    C = _csr(nc, 0, 40, 6, rng)
    I = _csr(ni, 40, 80, 4, rng)
    e = _engine(kind, p, k)
    idx, score = e.topk(_mat(C, p), _mat(I, p), ni)
    ref, scale = _oracle(e, C, I, p)
    assert idx.shape == (nc, ni)
    for c in range(nc):
        assert sorted(idx[c]) == list(range(ni))
        assert np.all(np.abs(score[c] - ref[c, idx[c]]) <= RTOL[kind] * scale[c, idx[c]])
    assert _ranked(idx, score)
    # top-K is the first K of the full ranking, bit for bit
    for K in (1, 5, 17):
        i2, s2 = e.topk(_mat(C, p), _mat(I, p), K)
        assert np.array_equal(i2, idx[:, :K]) and np.array_equal(s2, score[:, :K])
        # and against the oracle: the same set, up to near-ties at the cut
        for c in range(nc):
            o = np.lexsort((np.arange(ni), -ref[c]))
            if K < ni and abs(ref[c, o[K - 1]] - ref[c, o[K]]) <= 2 * RTOL[kind] * scale[c].max():
                continue
            assert set(i2[c]) == set(o[:K])


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_context_and_items_sharing_features(kind):
    rng = np.random.default_rng(5)
    p, nc, ni = 30, 5, 25
    C = _csr(nc, 0, 30, 8, rng)
    I = _csr(ni, 0, 30, 8, rng)   # the same id range: c (+) i may hold a feature twice
    e = _engine(kind, p, 8)
    idx, score = e.topk(_mat(C, p), _mat(I, p), ni)
    ref, scale = _oracle(e, C, I, p)
    for c in range(nc):
        assert np.all(np.abs(score[c] - ref[c, idx[c]]) <= RTOL[kind] * scale[c, idx[c]])
    assert _ranked(idx, score)


def test_ties_padding_and_empty_rows():
    rng = np.random.default_rng(9)
    p, nc = 40, 4
    C = _csr(nc, 0, 20, 5, rng, empty=(2,))
    I = _csr(10, 20, 40, 4, rng, empty=(3, 7))
    # duplicate item rows 1 -> 5, 8 and 0 -> 9
    rows = [_row(I, i) for i in range(10)]
    rows[5] = rows[8] = rows[1]; rows[9] = rows[0]
    rp = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    I = (rp, np.concatenate([r[0] for r in rows]).astype(np.uint32), np.concatenate([r[1] for r in rows]).astype(np.float32))
    for kind in ("seq64", "mb32"):
        e = _engine(kind, p, 8)
        idx, score = e.topk(_mat(C, p), _mat(I, p), 10)
        assert _ranked(idx, score)
        for c in range(nc):
            pos = {int(j): r for r, j in enumerate(idx[c])}
            assert pos[1] < pos[5] < pos[8] and pos[0] < pos[9]
            assert score[c, pos[1]] == score[c, pos[5]] == score[c, pos[8]] and score[c, pos[0]] == score[c, pos[9]]
            assert score[c, pos[3]] == score[c, pos[7]]   # the two empty item rows
        # top_k beyond the item count: -1 / NaN padding
        i2, s2 = e.topk(_mat(C, p), _mat(I, p), 13)
        assert np.array_equal(i2[:, :10], idx) and np.array_equal(s2[:, :10], score)
        assert np.all(i2[:, 10:] == -1) and np.all(np.isnan(s2[:, 10:]))
    # all items identical: index order
    same = (np.arange(7, dtype=np.int64) * 2, np.tile(np.array([21, 30], np.uint32), 6), np.tile(np.array([0.5, -1.0], np.float32), 6))
    e = _engine("mb32", p, 4)
    idx, score = e.topk(_mat(C, p), _mat(same, p), 6)
    assert np.all(idx == np.arange(6)) and np.all(score == score[:, :1])
    # no items at all
    none = (np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32))
    idx, score = e.topk(_mat(C, p), _mat(none, p), 3)
    assert np.all(idx == -1) and np.all(np.isnan(score))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_exclusion(kind):
    from fmwr_amd import engine
    rng = np.random.default_rng(13)
    p, nc, ni = 60, 5, 30
    C = _csr(nc, 0, 30, 5, rng)
    I = _csr(ni, 30, 60, 4, rng)
    e = _engine(kind, p, 8)
    full_i, full_s = e.topk(_mat(C, p), _mat(I, p), ni)
    lists = [np.array([17, 3, 3, 29, 0, 17], np.uint32),   # unsorted, duplicates
             np.array([], np.uint32),
             np.arange(ni, dtype=np.uint32)[::-1].copy(),   # everything
             rng.choice(ni, 12, replace=False).astype(np.uint32),
             np.array([5], np.uint32)]
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    X = engine.Matrix.from_csr(rp, np.concatenate(lists), np.ones(int(rp[-1]), np.float32), ni)
    for K in (4, ni):
        idx, score = e.topk(_mat(C, p), _mat(I, p), K, exclude=X)
        for c in range(nc):
            keep = [r for r in range(ni) if full_i[c, r] not in set(lists[c].tolist())]
            want_i = np.full(K, -1); want_s = np.full(K, np.nan)
            n = min(K, len(keep))
            want_i[:n] = full_i[c, keep[:n]]; want_s[:n] = full_s[c, keep[:n]]
            assert np.array_equal(idx[c], want_i)
            assert np.array_equal(score[c], want_s, equal_nan=True)
            assert not set(idx[c].tolist()) & set(lists[c].tolist())
        assert np.all(idx[2] == -1) and np.all(np.isnan(score[2]))


def _merge(parts, K):
    """numpy merge of per-part results (index already offset) under the total order"""
    idx = np.concatenate([p[0] for p in parts], axis=1)
    sc = np.concatenate([p[1] for p in parts], axis=1)
    out_i = np.empty((idx.shape[0], K), np.int64); out_s = np.empty((idx.shape[0], K))
    for r in range(idx.shape[0]):
        o = np.lexsort((idx[r], np.where(np.isnan(sc[r]), np.inf, -sc[r])))[:K]
        out_i[r], out_s[r] = idx[r, o], sc[r, o]
    return out_i, out_s


def _synthetic(n, lo, hi, nnz, seed):
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(lo, hi, (n, nnz)), axis=1).astype(np.uint32).ravel()
    val = rng.uniform(0.5, 1.5, n * nnz).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * nnz, col, val


def _sub(m, r0, r1):
    rp, col, val = m
    return rp[r0:r1 + 1] - rp[r0], col[rp[r0]:rp[r1]], val[rp[r0]:rp[r1]]


def _hip():
    import os
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library is not loadable")


def test_invariance_over_slices_chunks_and_calls():
    p, nc, ni, k, K = 300_000, 3000, 200_000, 16, 100
    C = _synthetic(nc, 0, 100_000, 12, 1)
    I = _synthetic(ni, 100_000, 300_000, 5, 2)
    e = _engine("mb32", p, k)
    mc, mi = _mat(C, p), _mat(I, p)
    idx, score = e.topk(mc, mi, K)
    assert _ranked(idx, score) and np.all(idx >= 0)
    # one context alone
    for c in (0, 1234, nc - 1):
        i1, s1 = e.topk(_mat(_sub(C, c, c + 1), p), mi, K)
        assert np.array_equal(i1[0], idx[c]) and np.array_equal(s1[0], score[c])
    # a permuted batch
    perm = np.random.default_rng(3).permutation(nc)[:700]
    rows = [_row(C, c) for c in perm]
    Cp = (np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64), np.concatenate([r[0] for r in rows]),
          np.concatenate([r[1] for r in rows]))
    ip, sp_ = e.topk(_mat(Cp, p), mi, K)
    assert np.array_equal(ip, idx[perm]) and np.array_equal(sp_, score[perm])
    # a sub-range through the device entry point (buffers from the HIP runtime itself)
    r0, r1 = 1000, 1700
    hip = _hip()
    nbytes = (r1 - r0) * K * 8
    di, ds = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(di), ctypes.c_size_t(nbytes)) == 0 and hip.hipMalloc(ctypes.byref(ds), ctypes.c_size_t(nbytes)) == 0
    try:
        e.topk_device(mc, r0, r1, mi, K, di.value, ds.value)
        e.sync()
        hi, hs = np.empty((r1 - r0, K), np.int64), np.empty((r1 - r0, K))
        assert hip.hipMemcpy(hi.ctypes.data_as(ctypes.c_void_p), di, ctypes.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
        assert hip.hipMemcpy(hs.ctypes.data_as(ctypes.c_void_p), ds, ctypes.c_size_t(nbytes), 2) == 0
    finally:
        hip.hipFree(di); hip.hipFree(ds)
    assert np.array_equal(hi, idx[r0:r1]) and np.array_equal(hs, score[r0:r1])
    # the two halves of the items, merged under the total order
    h = ni // 2
    a = e.topk(mc, _mat(_sub(I, 0, h), p), K)
    b = e.topk(mc, _mat(_sub(I, h, ni), p), K)
    mi_, ms_ = _merge([a, (b[0] + h, b[1])], K)
    assert np.array_equal(mi_, idx) and np.array_equal(ms_, score)
    # the scores themselves against the parameters, on a few contexts
    w0, w, v = e.get_params()
    # (rows may repeat a column: the squares are taken per entry, never on scipy's merged duplicates)
    Ai = sp.csr_matrix((I[2].astype(np.float64), I[1], I[0]), shape=(ni, p))
    Si = Ai @ v.T
    bi = Ai @ w + 0.5 * ((Si ** 2).sum(1) - (sp.csr_matrix((I[2].astype(np.float64) ** 2, I[1], I[0]), shape=(ni, p)) @ (v.T ** 2)).sum(1))
    Ac = sp.csr_matrix((C[2].astype(np.float64), C[1], C[0]), shape=(nc, p))
    Sc = Ac @ v.T
    bc = w0 + Ac @ w + 0.5 * ((Sc ** 2).sum(1) - (sp.csr_matrix((C[2].astype(np.float64) ** 2, C[1], C[0]), shape=(nc, p)) @ (v.T ** 2)).sum(1))
    for c in (0, 777, 2999):
        ref = bc[c] + bi[idx[c]] + Si[idx[c]] @ Sc[c]
        assert np.allclose(score[c], ref, rtol=1e-4, atol=1e-4)


def test_links_rank_on_the_raw_score():
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(21)
    p, nc, ni = 60, 5, 30
    C = _csr(nc, 0, 30, 5, rng)
    I = _csr(ni, 30, 60, 4, rng)
    pairs = _pairs(C, I)
    cases = [(L.TASK_CLASSIFICATION, L.SOLVER_SGD, L.LINK_LOGISTIC, {}),
             (L.TASK_CLASSIFICATION, L.SOLVER_ALS, L.LINK_PROBIT, {}),
             (L.TASK_REGRESSION, L.SOLVER_SGD, L.LINK_CLAMP, {"min_target": -0.5, "max_target": 0.5})]
    for task, solver, link, kw in cases:
        e = _engine("seq64", p, 8, task=task, solver=solver, **kw)
        raw_i, raw_s = e.topk(_mat(C, p), _mat(I, p), ni)
        li, ls = e.topk(_mat(C, p), _mat(I, p), ni, link=link)
        assert np.array_equal(li, raw_i)   # the order of the raw score, clamp ties included
        direct = e.predict(_mat(pairs, p), link).reshape(nc, ni)
        for c in range(nc):
            assert np.allclose(ls[c], direct[c, li[c]], rtol=1e-12, atol=1e-12)
        if link == L.LINK_CLAMP:
            assert np.sum(ls == 0.5) > 1   # ties at max_target exist and keep the raw order (checked above)


@pytest.mark.parametrize("layout", ["w_in_row", "mb64", "n_gpus2"])
def test_table_layouts(layout, monkeypatch):
    rng = np.random.default_rng(31)
    p, nc, ni, k = 80, 6, 40, 16
    C = _csr(nc, 0, 40, 6, rng)
    I = _csr(ni, 40, 80, 4, rng)
    if layout == "w_in_row":
        out = []
        for flag in ("0", "1"):
            monkeypatch.setenv("FMX_W_IN_ROW", flag)
            e = _engine("mb32", p, k)
            out.append(e.topk(_mat(C, p), _mat(I, p), ni))
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
        kind = "mb32"
    elif layout == "mb64":
        e = _engine("mb64", p, k)
        kind = "mb64"
    else:
        e = _engine("mb32", p, k, n_gpus=2, gpus_share_device=1)
        kind = "mb32"
    idx, score = e.topk(_mat(C, p), _mat(I, p), ni)
    ref, scale = _oracle(e, C, I, p)
    for c in range(nc):
        assert np.all(np.abs(score[c] - ref[c, idx[c]]) <= RTOL[kind] * scale[c, idx[c]])
    assert _ranked(idx, score)


def test_fm_recommend_movielens_shaped():
    import fmwr_amd as fm
    from tests.test_gpu_api import _movielens_shaped
    X, rating = _movielens_shaped()
    users, items = 943, 1682
    y = (rating >= 4).astype(np.float64)
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 8, "L2.w1": 1e-3, "L2.v": 1e-3, "v.init_stdev": 0.05}),
           fm.solver_control(max_iter=100_000, solver=fm.SGD_solver(learn_rate=0.02))]
    fit = fm.fm_train(fm.fm_matrix(X, y), normalize=False, control=ctl, seed=42)
    p = users + items
    who = np.random.default_rng(0).choice(users, 20, replace=False)
    ctx = sp.csr_matrix((np.ones(20), who, np.arange(21)), shape=(20, p))
    itm = sp.csr_matrix((np.ones(items), np.arange(items) + users, np.arange(items + 1)), shape=(items, p))
    Xc = X.tocsr()
    u_of = Xc.indices[Xc.indptr[:-1]]
    i_of = Xc.indices[Xc.indptr[:-1] + 1] - users
    rated = [np.unique(i_of[u_of == u]) for u in who]
    K = 10
    out = fm.fm_recommend(fit, fm.fm_matrix(ctx), fm.fm_matrix(itm), top_k=K, exclude=rated, normalize=False)
    assert out["index"].shape == (20, K) and out["score"].shape == (20, K)
    for r, u in enumerate(who):
        cross = sp.csr_matrix((np.ones(2 * items), np.stack([np.full(items, u), np.arange(items) + users], 1).ravel(), np.arange(0, 2 * items + 1, 2)),
                              shape=(items, p))
        pred = fm.predict(fit, fm.fm_matrix(cross), normalize=False)
        pred[rated[r]] = -np.inf
        order = np.lexsort((np.arange(items), -pred))
        got = out["index"][r]
        assert not set(got.tolist()) & set(rated[r].tolist())
        assert np.allclose(out["score"][r], pred[got], rtol=1e-12, atol=1e-15)
        if np.array_equal(got, order[:K]):
            continue
        # only near-ties may reorder
        assert np.all(np.abs(np.sort(pred[got]) - np.sort(pred[order[:K]])) <= 1e-12)


def test_full_size_spot_checked():
    import time
    p, nc, ni, k, K = 1_000_000, 10_000, 1_000_000, 16, 100
    t0 = time.time()
    C = _synthetic(nc, 0, p, 25, 7)
    I = _synthetic(ni, 0, p, 5, 8)
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(5, 0.0, 0.1)
    rng = np.random.default_rng(1)
    w = rng.normal(0, 0.1, p)
    _, _, v = e.get_params()
    e.set_params(0.2, w, v)
    w0, w, v = e.get_params()
    idx, score = e.topk(_mat(C, p), _mat(I, p), K)
    assert np.all(idx >= 0) and _ranked(idx, score)
    # (rows may repeat a column: the squares are taken per entry, never on scipy's merged duplicates)
    Ai = sp.csr_matrix((I[2].astype(np.float64), I[1], I[0]), shape=(ni, p))
    Si = Ai @ v.T
    bi = Ai @ w + 0.5 * ((Si ** 2).sum(1) - (sp.csr_matrix((I[2].astype(np.float64) ** 2, I[1], I[0]), shape=(ni, p)) @ (v.T ** 2)).sum(1))
    mi = np.abs(Ai) @ np.abs(v.T)
    for c in np.random.default_rng(2).choice(nc, 20, replace=False):
        cc, cv = _row(C, c)
        ac = sp.csr_matrix((cv.astype(np.float64), cc, [0, len(cc)]), shape=(1, p))
        sc = np.asarray(ac @ v.T).ravel()
        bc = w0 + float(ac @ w) + 0.5 * (np.sum(sc ** 2) - float((sp.csr_matrix((cv.astype(np.float64) ** 2, cc, [0, len(cc)]), shape=(1, p)) @ (v.T ** 2)).sum()))
        ref = bc + bi + Si @ sc
        tol = 1e-5 * (1 + abs(bc) + np.abs(bi) + mi @ np.abs(sc))
        assert np.all(np.abs(score[c] - ref[idx[c]]) <= tol[idx[c]])
        o = np.lexsort((np.arange(ni), -ref))
        if not np.array_equal(idx[c], o[:K]):
            # a difference only among near-ties: the returned K-th is within tolerance of the true K-th, nothing better was skipped
            assert abs(ref[idx[c][-1]] - ref[o[K - 1]]) <= 2 * tol.max()
            assert set(o[:K]) - set(idx[c]) <= {j for j in o[:2 * K] if ref[j] <= ref[o[K - 1]] + 2 * tol.max()}
    assert time.time() - t0 < 60
