"""fmx_heldout_rank / fmx_heldout_rank_device / fmx_heldout_metrics / fm_recommend_metrics: the rank of every held-out item in its context's
full ranking under fmx_topk's order, checked against fmx_topk itself and against numpy, and the metrics built on those ranks."""
import ctypes
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


def _csr(n, lo, hi, nnz, rng):
    rows = [np.sort(rng.choice(np.arange(lo, hi), int(rng.integers(1, nnz + 1)), replace=False)) for _ in range(n)]
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows])]).astype(np.int64)
    return rp, np.concatenate(rows).astype(np.uint32), rng.normal(0, 1, int(rp[-1])).astype(np.float32)


def _lists_csr(lists):
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(x, np.int64) for x in lists]).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    return rp, col


def _mat(m, p):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _ids(lists, n_items):
    from fmwr_amd import engine
    rp, col = _lists_csr(lists)
    return engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), n_items)


def _engine(kind, p, k, k0=1, k1=1, seed=11):
    from fmwr_amd import _lib as L, engine
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION, keep_w0=k0, keep_w1=k1)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=256, state_fp64=int(kind == "mb64"),
                          keep_w0=k0, keep_w1=k1)
    rng = np.random.default_rng(seed)
    e.set_params(0.3, rng.normal(0, 0.5, p), rng.normal(0, 0.4, (k, p)))
    return e


def _problem(n_ctx, n_items, p_ctx, p_items, rng, nnz=4):
    """context rows over features [0, p_ctx), item rows over [p_ctx, p_ctx + p_items)"""
    return _csr(n_ctx, 0, p_ctx, nnz, rng), _csr(n_items, p_ctx, p_ctx + p_items, nnz, rng)


def _random_lists(n_ctx, n_items, rng, most, empty_every=5, avoid=None):
    out = []
    for c in range(n_ctx):
        if empty_every and c % empty_every == 3:
            out.append([])
            continue
        pool = np.setdiff1d(np.arange(n_items), avoid[c]) if avoid is not None else np.arange(n_items)
        out.append(list(rng.choice(pool, int(rng.integers(1, most + 1)), replace=False)))
    return out


def _flat(lists):
    return [(c, int(h)) for c, hs in enumerate(lists) for h in hs]


def _count_ranks(S, held, excl):
    """rank by the definition, from a full score matrix S [n_ctx][n_items] (the total order: higher first, ties by index, NaN last)"""
    out = []
    n_items = S.shape[1]
    for c, h in _flat(held):
        x = set(int(j) for j in (excl[c] if excl is not None else []))
        s_h = S[c, h]
        r = 0
        for j in range(n_items):
            if j == h or j in x:
                continue
            s = S[c, j]
            if np.isnan(s_h):
                before = (not np.isnan(s)) or j < h
            else:
                before = (not np.isnan(s)) and (s > s_h or (s == s_h and j < h))
            r += bool(before)
        out.append(r)
    return np.array(out, np.int64)


def _numpy_scores(e, C_, I_, p):
    """fp64 scores of every (context, item) pair from the engine's parameters: base_c (w0 included) + base_i + <s_c, s_i>"""
    w0, w, v = e.get_params()
    k0, k1 = e.cfg.keep_w0, e.cfg.keep_w1

    def parts(m):
        rp, col, val = m
        n = len(rp) - 1
        X = sp.csr_matrix((val.astype(np.float64), col.astype(np.int64), rp), shape=(n, p))
        s = X @ v.T
        base = k1 * (X @ w) + 0.5 * (np.sum(s * s, 1) - (X.multiply(X)) @ np.sum(v * v, 0))
        return base, s
    bc, sc = parts(C_)
    bi, si = parts(I_)
    return (k0 * w0 + bc)[:, None] + bi[None, :] + sc @ si.T


def _metrics_numpy(ranks_by_ctx, n_items, nx, ks):
    """per-context metric rows from the sorted distinct ranks of each context (None: no held-out item)"""
    rows = []
    for c, r in enumerate(ranks_by_ctx):
        if not r:
            rows.append([math.nan] * (4 * len(ks) + 2))
            continue
        r = sorted(r)
        m = len(r)
        row = []
        for K in ks:
            hits = sum(1 for x in r if x < K)
            dcg = sum(1 / math.log2(x + 2) for x in r if x < K)
            idcg = sum(1 / math.log2(t + 2) for t in range(min(K, m)))
            row += [hits / K, hits / m, dcg / idcg, float(hits > 0)]
        row.append(1 / (1 + r[0]))
        N = n_items - nx[c] - m
        row.append(math.nan if N <= 0 else sum((N - (x - t)) / N for t, x in enumerate(r)) / m)
        rows.append(row)
    return np.array(rows)


# ------------------------------------------------------------------------------------------------ 1. agreement with fmx_topk
@pytest.mark.parametrize("kind", ["mb32", "mb64", "seq64"])
@pytest.mark.parametrize("with_exclude", [False, True])
@pytest.mark.parametrize("keep", [(1, 1), (0, 0)])
def test_ranks_agree_with_topk_exactly(kind, with_exclude, keep):
    rng = np.random.default_rng(3)
    n_ctx, n_items, pc, pi, k = 37, 700, 50, 400, 12
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng)
    p = pc + pi
    e = _engine(kind, p, k, *keep)
    excl = [list(rng.choice(n_items, int(rng.integers(0, 60)), replace=True)) for _ in range(n_ctx)] if with_exclude else None
    held = _random_lists(n_ctx, n_items, rng, 9, avoid=excl)
    cm, im, hm = _mat(C_, p), _mat(I_, p), _ids(held, n_items)
    xm = _ids(excl, n_items) if with_exclude else None
    rank, score = e.heldout_rank(cm, im, hm, exclude=xm)
    idx, sc = e.topk(cm, im, n_items, exclude=xm)
    for q, (c, h) in enumerate(_flat(held)):
        pos = np.nonzero(idx[c] == h)[0]
        assert len(pos) == 1
        assert rank[q] == pos[0], (c, h)
        assert score[q].tobytes() == sc[c, pos[0]].tobytes()


# ------------------------------------------------------------------------------------------------ 2. brute force
@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_brute_force_against_numpy(kind):
    rng = np.random.default_rng(5)
    n_ctx, n_items, pc, pi, k = 29, 260, 40, 200, 8
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng)
    p = pc + pi
    e = _engine(kind, p, k)
    excl = [list(rng.choice(n_items, int(rng.integers(0, 30)), replace=True)) for _ in range(n_ctx)]
    held = _random_lists(n_ctx, n_items, rng, 12, avoid=excl)
    cm, im, hm, xm = _mat(C_, p), _mat(I_, p), _ids(held, n_items), _ids(excl, n_items)
    rank, score = e.heldout_rank(cm, im, hm, exclude=xm)
    S = _numpy_scores(e, C_, I_, p)
    tol = 1e-12 if kind == "seq64" else 1e-4
    assert np.max(np.abs(score - np.array([S[c, h] for c, h in _flat(held)]))) <= tol * max(1.0, np.max(np.abs(S)))
    assert np.array_equal(rank, _count_ranks(S, held, excl))
    ks = [1, 5, 20, 1000]
    res = e.heldout_metrics(cm, im, hm, ks, exclude=xm, per_context=True)
    by_ctx = [[] for _ in range(n_ctx)]
    for q, (c, h) in enumerate(_flat(held)):
        by_ctx[c].append(int(rank[q]))
    nx = [len(set(x)) for x in excl]
    want = _metrics_numpy(by_ctx, n_items, nx, ks)
    got = res["per_context"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.nanmax(np.abs(got - want)) <= 1e-12
    counted = [c for c in range(n_ctx) if by_ctx[c]]
    assert res["counted"] == (len(counted), len(counted))
    assert np.max(np.abs(res["mean"] - np.nanmean(want, 0))) <= 1e-12


# ------------------------------------------------------------------------------------------------ 3. ties and NaN
def test_identical_items_rank_by_index_and_nan_ranks_last():
    rng = np.random.default_rng(8)
    n_ctx, pc, pi, k = 6, 20, 30, 8
    p = pc + pi
    C_ = _csr(n_ctx, 0, pc, 3, rng)
    base = _csr(10, pc, pc + pi - 1, 3, rng)
    rows = [base[1][base[0][r]:base[0][r + 1]] for r in range(10)]
    vals = [base[2][base[0][r]:base[0][r + 1]] for r in range(10)]
    # items 10..14 are copies of item 3; item 15 holds the NaN feature p - 1 alone, item 16 the NaN feature with item 3's entries
    rows += [rows[3]] * 5 + [np.array([p - 1], np.uint32), np.concatenate([rows[3], [p - 1]]).astype(np.uint32)]
    vals += [vals[3]] * 5 + [np.ones(1, np.float32), np.concatenate([vals[3], [1.0]]).astype(np.float32)]
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    I_ = (rp, np.concatenate(rows).astype(np.uint32), np.concatenate(vals).astype(np.float32))
    n_items = len(rows)
    e = _engine("seq64", p, k)
    w0, w, v = e.get_params()
    w[p - 1] = np.nan
    e.set_params(w0, w, v)
    held = [[3, 10, 12, 14, 15, 16] for _ in range(n_ctx)]
    cm, im, hm = _mat(C_, p), _mat(I_, p), _ids(held, n_items)
    rank, score = e.heldout_rank(cm, im, hm)
    rank = rank.reshape(n_ctx, 6)
    score = score.reshape(n_ctx, 6)
    assert np.all(np.isnan(score[:, 4:]))
    for c in range(n_ctx):
        # the copies rank in index order: 3, 10, (11), 12, (13), 14
        assert list(rank[c, :4] - rank[c, 0]) == [0, 1, 3, 5]
        assert rank[c, 4] == n_items - 2 and rank[c, 5] == n_items - 1  # after every numeric item, NaNs by index
    idx, _ = e.topk(cm, im, n_items)
    for c in range(n_ctx):
        assert list(idx[c, -2:]) == [15, 16]


# ------------------------------------------------------------------------------------------------ 4. duplicates and edge cases
def test_duplicates_empty_contexts_and_no_eligible_negative():
    rng = np.random.default_rng(9)
    n_ctx, n_items, pc, pi, k = 5, 40, 20, 60, 4
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng)
    p = pc + pi
    e = _engine("mb64", p, k)
    held = [[3, 7, 3, 3], [], [5], list(range(20, 40)), [1, 2]]
    excl = [[], [], [0], list(range(0, 20)) + [4, 4], []]   # context 3: every item held out or excluded -> N = 0
    cm, im, hm, xm = _mat(C_, p), _mat(I_, p), _ids(held, n_items), _ids(excl, n_items)
    rank, score = e.heldout_rank(cm, im, hm, exclude=xm)
    assert rank[0] == rank[2] == rank[3] and score[0].tobytes() == score[2].tobytes() == score[3].tobytes()
    res = e.heldout_metrics(cm, im, hm, [1, 3], exclude=xm, per_context=True)
    pcm = res["per_context"]
    assert np.all(np.isnan(pcm[1]))
    assert np.isnan(pcm[3, -1]) and not np.any(np.isnan(pcm[3, :-1]))
    assert res["counted"] == (4, 3)
    # context 0 counts {3, 7} once each: recall@3 has denominator 2
    r0 = sorted({int(rank[0]), int(rank[1])})
    assert pcm[0, 4 + 1] == sum(1 for x in r0 if x < 3) / 2
    # context 3: its 20 held-out items are the only eligible ones, ranked 0..19
    assert sorted(rank[5:25]) == list(range(20)) and pcm[3, 4 * 1 + 1] == 3 / 20
    assert res["mean"][-1] == pytest.approx(np.nanmean(pcm[:, -1]), rel=1e-14)


def test_overlap_with_exclude_is_refused_and_writes_nothing():
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(10)
    n_ctx, n_items, pc, pi, k = 4, 30, 10, 40, 4
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng)
    p = pc + pi
    e = _engine("mb32", p, k)
    held = [[1], [2, 3], [4], [5]]
    excl = [[0], [9], [8], [5, 6]]  # context 3 holds item 5 in both
    cm, im, hm, xm = _mat(C_, p), _mat(I_, p), _ids(held, n_items), _ids(excl, n_items)
    rank = np.full(5, 77, np.int64)
    score = np.full(5, 7.5)
    st = L.lib().fmx_heldout_rank(e.h, cm.h, im.h, hm.h, xm.h, rank.ctypes.data_as(ctypes.c_void_p), score.ctypes.data_as(ctypes.c_void_p))
    assert st == L.ERR_INVALID and b"heldout" in L.lib().fmx_last_error()
    assert np.all(rank == 77) and np.all(score == 7.5)
    out = np.full(6, 7.5)
    counted = np.full(2, 77, np.int64)
    ks = np.array([2], np.int32)
    st = L.lib().fmx_heldout_metrics(e.h, cm.h, im.h, hm.h, xm.h, ks.ctypes.data_as(ctypes.c_void_p), ctypes.c_int32(1),
                                     out.ctypes.data_as(ctypes.c_void_p), None, counted.ctypes.data_as(ctypes.c_void_p))
    assert st == L.ERR_INVALID
    assert np.all(out == 7.5) and np.all(counted == 77)
    # the engine still works
    e.heldout_rank(cm, im, hm)


def test_empty_items():
    rng = np.random.default_rng(12)
    pc, pi, k = 10, 20, 4
    p = pc + pi
    C_ = _csr(3, 0, pc, 3, rng)
    e = _engine("mb32", p, k)
    from fmwr_amd import engine
    im = engine.Matrix.from_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), p)
    hm = _ids([[], [], []], 0)
    rank, score = e.heldout_rank(_mat(C_, p), im, hm)
    assert rank.size == 0 and score.size == 0
    res = e.heldout_metrics(_mat(C_, p), im, hm, [5])
    assert np.all(np.isnan(res["mean"])) and res["counted"] == (0, 0)


# ------------------------------------------------------------------------------------------------ 5. invariance
def _hip():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library is not loadable")


def _device_ranks(e, cm, r0, r1, im, hm, xm, cnt):
    hip = _hip()
    dr, ds = ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(dr), ctypes.c_size_t(max(cnt, 1) * 8)) == 0
    assert hip.hipMalloc(ctypes.byref(ds), ctypes.c_size_t(max(cnt, 1) * 8)) == 0
    try:
        e.heldout_rank_device(cm, r0, r1, im, hm, dr.value, ds.value, exclude=xm)
        e.sync()
        r, s = np.empty(cnt, np.int64), np.empty(cnt)
        if cnt:
            assert hip.hipMemcpy(r.ctypes.data_as(ctypes.c_void_p), dr, ctypes.c_size_t(cnt * 8), 2) == 0
            assert hip.hipMemcpy(s.ctypes.data_as(ctypes.c_void_p), ds, ctypes.c_size_t(cnt * 8), 2) == 0
    finally:
        hip.hipFree(dr)
        hip.hipFree(ds)
    return r, s


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
def test_bitwise_invariance(kind):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(13)
    n_ctx, n_items, pc, pi, k = 45, 1500, 60, 500, 16
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng)
    p = pc + pi
    e = _engine(kind, p, k)
    excl = [list(rng.choice(n_items, int(rng.integers(0, 80)))) for _ in range(n_ctx)]
    held = _random_lists(n_ctx, n_items, rng, 15, avoid=excl)
    held[7] = list(np.setdiff1d(np.arange(n_items), excl[7])[rng.permutation(n_items - len(set(excl[7])))[:400]])  # many windows
    cm, im, hm, xm = _mat(C_, p), _mat(I_, p), _ids(held, n_items), _ids(excl, n_items)
    ks = [1, 10, 100, 2000]
    rank, score = e.heldout_rank(cm, im, hm, exclude=xm)
    met = e.heldout_metrics(cm, im, hm, ks, exclude=xm, per_context=True)
    # repeated calls
    r2, s2 = e.heldout_rank(cm, im, hm, exclude=xm)
    assert np.array_equal(rank, r2) and score.tobytes() == s2.tobytes()
    m2 = e.heldout_metrics(cm, im, hm, ks, exclude=xm, per_context=True)
    assert met["mean"].tobytes() == m2["mean"].tobytes() and met["per_context"].tobytes() == m2["per_context"].tobytes()
    # small windows and chunks (test hook, one call each)
    L.check(L.lib().fmx_debug_heldout_limits(ctypes.c_int32(4), ctypes.c_int64(3)))
    r3, s3 = e.heldout_rank(cm, im, hm, exclude=xm)
    assert np.array_equal(rank, r3) and score.tobytes() == s3.tobytes()
    L.check(L.lib().fmx_debug_heldout_limits(ctypes.c_int32(1), ctypes.c_int64(1)))
    m3 = e.heldout_metrics(cm, im, hm, ks, exclude=xm, per_context=True)
    assert met["mean"].tobytes() == m3["mean"].tobytes() and met["per_context"].tobytes() == m3["per_context"].tobytes()
    # device sub-ranges
    hrp = _lists_csr(held)[0]
    for r0, r1 in ((0, n_ctx), (5, 6), (7, 8), (3, 30), (44, 45), (10, 10)):
        a, b = int(hrp[r0]), int(hrp[r1])
        rd, sd = _device_ranks(e, cm, r0, r1, im, hm, xm, b - a)
        assert np.array_equal(rd, rank[a:b]) and sd.tobytes() == score[a:b].tobytes()
    # permuted contexts
    perm = rng.permutation(n_ctx)
    Cp = _lists_csr([C_[1][C_[0][c]:C_[0][c + 1]] for c in perm])
    Cv = np.concatenate([C_[2][C_[0][c]:C_[0][c + 1]] for c in perm])
    rp_, sp_ = e.heldout_rank(_mat((Cp[0], Cp[1], Cv), p), im, _ids([held[c] for c in perm], n_items), exclude=_ids([excl[c] for c in perm], n_items))
    off = 0
    for c in perm:
        m = len(held[c])
        assert np.array_equal(rp_[off:off + m], rank[hrp[c]:hrp[c] + m]) and sp_[off:off + m].tobytes() == score[hrp[c]:hrp[c] + m].tobytes()
        off += m
    mp = e.heldout_metrics(_mat((Cp[0], Cp[1], Cv), p), im, _ids([held[c] for c in perm], n_items), ks, exclude=_ids([excl[c] for c in perm], n_items),
                           per_context=True)
    assert mp["per_context"].tobytes() == met["per_context"][perm].tobytes()


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_chunk_without_entries_between_chunks_with_entries(kind):
    """rows of 2, 0, 0 and 3 held-out items (one twice): with chunks of one context the two middle chunks hold nothing, with chunks of
    three the last one is a chunk of its own; ranks, scores and metrics are the unhooked call's bits and numpy's count"""
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(21)
    n_ctx, n_items, pc, pi, k = 4, 8, 10, 12, 3
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng, nnz=3)
    p = pc + pi
    e = _engine(kind, p, k)
    held = [[1, 5], [], [], [2, 6, 2]]
    cm, im, hm = _mat(C_, p), _mat(I_, p), _ids(held, n_items)
    rank, score = e.heldout_rank(cm, im, hm)
    met = e.heldout_metrics(cm, im, hm, [1, 3], per_context=True)
    idx, sc = e.topk(cm, im, n_items)   # the engine's own score of every pair
    S = np.empty((n_ctx, n_items))
    for c in range(n_ctx):
        assert sorted(idx[c]) == list(range(n_items))
        S[c, idx[c]] = sc[c]
    assert np.array_equal(rank, _count_ranks(S, held, None))
    assert score.tobytes() == np.array([S[c, h] for c, h in _flat(held)]).tobytes()
    assert np.all(np.isnan(met["per_context"][1:3])) and not np.any(np.isnan(met["per_context"][[0, 3]]))
    for window, chunk in ((1, 1), (4, 3)):
        L.check(L.lib().fmx_debug_heldout_limits(ctypes.c_int32(window), ctypes.c_int64(chunk)))
        r2, s2 = e.heldout_rank(cm, im, hm)
        assert np.array_equal(rank, r2) and score.tobytes() == s2.tobytes(), (window, chunk)
        L.check(L.lib().fmx_debug_heldout_limits(ctypes.c_int32(window), ctypes.c_int64(chunk)))
        m2 = e.heldout_metrics(cm, im, hm, [1, 3], per_context=True)
        assert met["mean"].tobytes() == m2["mean"].tobytes() and met["per_context"].tobytes() == m2["per_context"].tobytes(), (window, chunk)
        assert met["counted"] == m2["counted"]


# ------------------------------------------------------------------------------------------------ 6. K beyond 1024
def test_k_beyond_the_topk_limit():
    rng = np.random.default_rng(17)
    n_ctx, n_items, pc, pi, k = 12, 20000, 30, 3000, 8
    C_, I_ = _problem(n_ctx, n_items, pc, pi, rng, nnz=3)
    p = pc + pi
    e = _engine("seq64", p, k)
    excl = [list(rng.choice(n_items, 500, replace=False)) for _ in range(n_ctx)]
    held = _random_lists(n_ctx, n_items, rng, 40, empty_every=0, avoid=excl)
    cm, im, hm, xm = _mat(C_, p), _mat(I_, p), _ids(held, n_items), _ids(excl, n_items)
    rank, _ = e.heldout_rank(cm, im, hm, exclude=xm)
    S = _numpy_scores(e, C_, I_, p)
    want = []
    for c, h in _flat(held):
        ok = np.ones(n_items, bool)
        ok[excl[c]] = False
        ok[h] = False
        s = S[c]
        want.append(int(np.sum(ok & ((s > s[h]) | ((s == s[h]) & (np.arange(n_items) < h))))))
    assert np.array_equal(rank, np.array(want))
    res = e.heldout_metrics(cm, im, hm, [5000, 20000], exclude=xm)
    hits = sum(1 for r in rank if r < 5000)
    assert res["counted"] == (n_ctx, n_ctx)
    by_ctx = [[] for _ in range(n_ctx)]
    for q, (c, h) in enumerate(_flat(held)):
        by_ctx[c].append(int(rank[q]))
    want_m = np.nanmean(_metrics_numpy(by_ctx, n_items, [500] * n_ctx, [5000, 20000]), 0)
    assert np.max(np.abs(res["mean"] - want_m)) <= 1e-12
    assert hits > 0 and res["mean"][4 + 1] == 1.0  # recall@20000: every held-out item is ranked


# ------------------------------------------------------------------------------------------------ 7. end to end
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


def test_end_to_end_on_a_planted_problem():
    import fmwr_amd as fm
    context, items, train, test = _planted()
    n_users = context.dim[0]
    ctl = [fm.model_control("RANK", **{"factor.number": 16, "v.init_stdev": 0.1}), fm.solver_control(solver=fm.SGD_solver(learn_rate=0.1))]
    fit0 = fm.fm_train_rank(context, items, train, control=ctl, epochs=0, seed=3, batch_rows=4096)
    fit = fm.fm_train_rank(context, items, train, control=ctl, n_neg=2, epochs=30, seed=3, batch_rows=4096)
    before = fm.fm_recommend_metrics(fit0, context, items, test, k=[10, 50], exclude=train, normalize=False)
    after = fm.fm_recommend_metrics(fit, context, items, test, k=[10, 50], exclude=train, normalize=False, per_context=True, ranks=True)
    print("before", before, "\nafter", {k: v for k, v in after.items() if k not in ("per_context", "rank")})
    assert after["n_contexts"] == n_users and after["n_auc_contexts"] == n_users
    # recall@10 is exactly the hit count of fm_recommend's top 10
    rec = fm.fm_recommend(fit, context, items, top_k=10, exclude=train, normalize=False)
    hits = sum(len(set(rec["index"][u]) & set(test[u])) for u in range(n_users))
    assert after["recall@10"] * 2 * n_users == pytest.approx(hits, abs=1e-9)
    per = after["per_context"]["recall@10"] * 2
    for u in range(0, n_users, 97):
        assert per[u] == len(set(rec["index"][u]) & set(test[u]))
    R = after["rank"].tocsr()
    for u in range(0, n_users, 131):
        for h in test[u]:
            r = int(R[u, h])
            assert (r < 10) == (h in set(rec["index"][u])) and (r >= 10 or rec["index"][u][r] == h)
    # auc without exclusion estimates what fm_rank_evaluate samples: a held-out positive against a uniform non-held-out item
    auc = fm.fm_recommend_metrics(fit, context, items, test, k=10, normalize=False)["auc"]
    pair = fm.fm_rank_evaluate(fit, context, items, test, n_neg=50, seed=5)["pair_acc"]
    # 2 000 users x 2 held-out x 50 draws = 200 000 pairs: the sampling standard error is below 0.001; 0.01 is ten of them
    assert abs(auc - pair) < 0.01, (auc, pair)
    for key in ("precision@10", "recall@10", "ndcg@10", "hit@10", "precision@50", "recall@50", "ndcg@50", "hit@50", "mrr", "auc"):
        assert after[key] > before[key], key
