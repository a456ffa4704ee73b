"""fmx_rank_lists / fmx_topk_lists / fmx_project: candidate lists scored and ordered with work proportional to the lists.  The yardsticks are
calls that existed before them -- fmx_topk (with the complement of a list as its exclusion), fmx_heldout_rank, fmx_predict -- and the oracle;
scores, positions and top-K lists are compared as bit patterns."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from tests import lists_model
from tests.test_gpu_topk import RTOL, _csr, _engine, _mat, _oracle, _row, _sub
from tests.util import DevBuf

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _lists_matrix(lists, ni):
    from fmwr_amd import engine
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if rp[-1] else np.zeros(0, np.uint32)
    return engine.Matrix.from_csr(rp, col, np.ones(int(rp[-1]), np.float32), ni), rp


def _random_lists(nc, ni, rng):
    """unsorted lists with duplicates, an empty one, one holding every item, a single candidate"""
    lists = [rng.integers(0, ni, int(rng.integers(2, 2 * ni))).astype(np.uint32) for _ in range(nc)]
    lists[1] = np.zeros(0, np.uint32)
    lists[2] = rng.permutation(ni).astype(np.uint32)
    lists[3] = np.array([ni - 1], np.uint32)
    lists[4] = np.array([5, 5, 5, 0, 5, 0], np.uint32)
    return lists


def _dense_scores(e, mc, mi, ni):
    """every pair's raw score as fmx_topk(K = n_items) lists it: S[c, j]"""
    idx, score = e.topk(mc, mi, ni)
    S = np.empty(score.shape)
    for c in range(idx.shape[0]):
        assert sorted(idx[c]) == list(range(ni))
        S[c, idx[c]] = score[c]
    return S


def _complement(lists, ni):
    return [np.setdiff1d(np.arange(ni, dtype=np.uint32), np.asarray(x, np.uint32)) for x in lists]


def _problem(seed, ni=41, nc=6):
    rng = np.random.default_rng(seed)
    C = _csr(nc, 0, 40, 6, rng)
    I = _csr(ni, 40, 80, 4, rng)
    return rng, C, I


def _check_against_topk(e, C, I, lists, p=80, Ks=(1, 5, 17), links=None):
    """scores, positions and top-K of the lists against fmx_topk on the same engine (exclude = the complement of every list)"""
    from fmwr_amd import _lib as L
    ni, nc = len(I[0]) - 1, len(C[0]) - 1
    mc, mi = _mat(C, p), _mat(I, p)
    ml, rp = _lists_matrix(lists, ni)
    S = _dense_scores(e, mc, mi, ni)
    score, pos = e.rank_lists(mc, mi, ml)
    mx, _ = _lists_matrix(_complement(lists, ni), ni)
    full_i, full_s = e.topk(mc, mi, ni, exclude=mx)
    for c in range(nc):
        lst = lists[c].astype(np.int64)
        sl = slice(rp[c], rp[c + 1])
        assert _same(score[sl], S[c, lst]), (c, score[sl], S[c, lst])
        slot = {int(j): t for t, j in enumerate(full_i[c]) if j >= 0}
        assert len(slot) == len(set(lst.tolist()))
        assert np.array_equal(pos[sl], np.array([slot[int(j)] for j in lst], np.int64)), c
        assert np.array_equal(pos[sl], lists_model.positions(S[c], lst))
    s_only, none = e.rank_lists(mc, mi, ml, positions=False)
    assert none is None and _same(s_only, score)
    for link in (links or [L.LINK_NONE]):
        ls, lp = e.rank_lists(mc, mi, ml, link=link)
        assert np.array_equal(lp, pos)   # positions always follow the raw score
        for K in Ks:
            want_i, want_s = e.topk(mc, mi, K, exclude=mx, link=link)
            got_i, got_s = e.topk_lists(mc, mi, ml, K, link=link)
            assert np.array_equal(got_i, want_i), (link, K)
            assert _same(got_s, want_s), (link, K)
            for c in range(nc):   # and the linked per-entry scores are the linked top-K scores of the same candidates
                for t in range(K):
                    if got_i[c, t] >= 0:
                        hit = np.nonzero(lists[c] == got_i[c, t])[0]
                        assert _same(ls[rp[c] + hit], np.full(len(hit), got_s[c, t]))
    return score, pos


KINDS = [("seq64", k) for k in (0, 1, 3, 16, 64, 100)] + [("mb64", k) for k in (0, 1, 3, 16, 64, 100)] + \
        [("mb32", k) for k in (0, 1, 3, 16, 64, 100)] + [("mb32w", k) for k in (1, 3, 16)]


@pytest.mark.parametrize("kind,k", KINDS)
def test_scores_positions_and_topk_equal_fmx_topk_bit_for_bit(kind, k, monkeypatch):
    if kind == "mb32w":
        monkeypatch.setenv("FMX_W_IN_ROW", "1")
    rng, C, I = _problem(100 + k)
    e = _engine("mb32" if kind == "mb32w" else kind, 80, k)
    if kind == "mb32w":
        assert e.w_in_row()
    _check_against_topk(e, C, I, _random_lists(6, 41, rng))


@pytest.mark.parametrize("kind", ["seq64", "mb64", "mb32"])
@pytest.mark.parametrize("k", [0, 1, 3, 16, 64, 100])
def test_scores_against_the_oracle_of_the_concatenated_rows(kind, k):
    rng, C, I = _problem(200 + k)
    e = _engine(kind, 80, k)
    lists = _random_lists(6, 41, rng)
    ml, rp = _lists_matrix(lists, 41)
    score, _ = e.rank_lists(_mat(C, 80), _mat(I, 80), ml)
    ref, scale = _oracle(e, C, I, 80)
    for c in range(6):
        lst = lists[c].astype(np.int64)
        assert np.all(np.abs(score[rp[c]:rp[c + 1]] - ref[c, lst]) <= RTOL[kind] * scale[c, lst])


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_many_items_against_heldout_rank(kind):
    """n_items > 1024: the scores are fmx_heldout_rank(heldout = lists)'s; with L_c = every item outside X_c the positions are its ranks"""
    rng = np.random.default_rng(7)
    p, nc, ni = 80, 5, 1500
    C = _csr(nc, 0, 40, 6, rng)
    I = _csr(ni, 40, 80, 4, rng)
    e = _engine(kind, p, 16)
    mc, mi = _mat(C, p), _mat(I, p)
    lists = [rng.integers(0, ni, 30).astype(np.uint32) for _ in range(nc)]
    lists[2] = np.zeros(0, np.uint32)
    lists[3] = rng.integers(0, ni, 1300).astype(np.uint32)   # beyond the fused path's budget: the general path
    ml, rp = _lists_matrix(lists, ni)
    score, pos = e.rank_lists(mc, mi, ml)
    _, h_score = e.heldout_rank(mc, mi, ml)
    assert _same(score, h_score)
    X = [rng.choice(ni, int(rng.integers(0, 1400)), replace=False).astype(np.uint32) for _ in range(nc)]
    X[1] = np.zeros(0, np.uint32)
    rest = _complement(X, ni)
    rest = [rng.permutation(x) for x in rest]
    mx, _ = _lists_matrix(X, ni)
    mr, _ = _lists_matrix(rest, ni)
    s2, p2 = e.rank_lists(mc, mi, mr)
    h_rank, h_s = e.heldout_rank(mc, mi, mr, exclude=mx)
    assert np.array_equal(p2, h_rank) and _same(s2, h_s)
    # the top of such a list is fmx_topk's
    for K in (1, 17, 1024):
        gi, gs = e.topk_lists(mc, mi, mr, K)
        wi, ws = e.topk(mc, mi, K, exclude=mx)
        assert np.array_equal(gi, wi) and _same(gs, ws)


def _duplicate_rows(I, pairs):
    rows = [_row(I, i) for i in range(len(I[0]) - 1)]
    for dst, src in pairs:
        rows[dst] = rows[src]
    rp = np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])]).astype(np.int64)
    return rp, np.concatenate([r[0] for r in rows]).astype(np.uint32), np.concatenate([r[1] for r in rows]).astype(np.float32)


@pytest.mark.parametrize("kind", ["seq64", "mb64", "mb32"])
def test_exact_ties_zero_scores_and_nan(kind):
    rng, C, I = _problem(33)
    lists = _random_lists(6, 41, rng)
    # exact ties: duplicated item rows (and two empty ones)
    I2 = _duplicate_rows(I, [(5, 1), (8, 1), (9, 0), (30, 12)])
    e = _engine(kind, 80, 8)
    score, pos = _check_against_topk(e, C, I2, lists)
    ml, rp = _lists_matrix(lists, 41)
    c = 2   # the list holding every item
    by_item = {int(j): (score[rp[c] + t], pos[rp[c] + t]) for t, j in enumerate(lists[c])}
    assert by_item[1][0] == by_item[5][0] == by_item[8][0] and by_item[1][1] < by_item[5][1] < by_item[8][1]
    assert by_item[0][0] == by_item[9][0] and by_item[0][1] < by_item[9][1]
    # a zero model: every score is 0, the order is the index order
    e.set_params(0.0, np.zeros(80), np.zeros((8, 80)))
    score, pos = _check_against_topk(e, C, I, lists)
    assert np.all(score == 0.0)
    assert np.array_equal(pos[rp[2]:rp[3]], lists[2].astype(np.int64))
    # -0: a model whose only parameter is a bias of -0
    e.set_params(-0.0, np.zeros(80), np.zeros((8, 80)))
    _check_against_topk(e, C, I, lists)
    # NaN: planted in the V rows of two item-side features
    e = _engine(kind, 80, 8)
    used = np.unique(I[1])
    bad = used[[1, len(used) // 2]].astype(np.uint32)
    w, v = e.get_rows(bad)
    v[3, :] = np.nan
    e.set_rows(bad, w, v)
    score, pos = _check_against_topk(e, C, I, lists)
    assert np.isnan(score).any() and not np.isnan(score).all()
    sl = slice(rp[2], rp[3])
    nan_items = lists[2][np.isnan(score[sl])].astype(np.int64)
    n_ok = 41 - len(nan_items)
    assert np.array_equal(np.sort(pos[sl][np.isnan(score[sl])]), np.arange(n_ok, 41))   # NaN below every number, by the index
    assert np.array_equal(pos[sl][np.isnan(score[sl])] - n_ok, np.argsort(np.argsort(nan_items)))


def test_every_link():
    from fmwr_amd import _lib as L
    rng, C, I = _problem(21)
    lists = _random_lists(6, 41, rng)
    cases = [("seq64", L.TASK_CLASSIFICATION, L.SOLVER_SGD, [L.LINK_LOGISTIC], {}),
             ("seq64", L.TASK_CLASSIFICATION, L.SOLVER_ALS, [L.LINK_PROBIT], {}),
             ("seq64", L.TASK_REGRESSION, L.SOLVER_SGD, [L.LINK_CLAMP], {"min_target": -0.5, "max_target": 0.5}),
             ("mb32", L.TASK_CLASSIFICATION, L.SOLVER_SGD, [L.LINK_LOGISTIC, L.LINK_PROBIT], {}),
             ("mb32", L.TASK_REGRESSION, L.SOLVER_SGD, [L.LINK_CLAMP], {"min_target": -0.5, "max_target": 0.5})]
    for kind, task, solver, links, kw in cases:
        e = _engine(kind, 80, 8, task=task, solver=solver, **kw)
        _check_against_topk(e, C, I, lists, links=[L.LINK_NONE] + links)


def _device_rank(e, mc, r0, r1, mi, ml, cnt, link=0):
    ds, dp = DevBuf(cnt), DevBuf(cnt, np.int64)
    try:
        e.rank_lists_device(mc, r0, r1, mi, ml, ds.ptr.value, dp.ptr.value, link=link)
        e.sync()
        return ds.numpy()[:cnt], dp.numpy()[:cnt]
    finally:
        ds.free(); dp.free()


def _device_topk(e, mc, r0, r1, mi, ml, K):
    di, ds = DevBuf((r1 - r0) * K, np.int64), DevBuf((r1 - r0) * K)
    try:
        e.topk_lists_device(mc, r0, r1, mi, ml, K, di.ptr.value, ds.ptr.value)
        e.sync()
        return di.numpy().reshape(r1 - r0, K), ds.numpy().reshape(r1 - r0, K)
    finally:
        di.free(); ds.free()


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_invariance_over_paths_chunks_ranges_order_and_calls(kind):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(55)
    p, nc, ni, K = 80, 11, 60, 7
    C = _csr(nc, 0, 40, 6, rng)
    I = _duplicate_rows(_csr(ni, 40, 80, 4, rng), [(7, 3), (50, 3)])
    e = _engine(kind, p, 16)
    mc, mi = _mat(C, p), _mat(I, p)
    lists = [rng.integers(0, ni, int(rng.integers(0, 12))).astype(np.uint32) for _ in range(nc)]
    lists[0] = np.array([9], np.uint32)
    lists[5] = np.zeros(0, np.uint32)
    lists[8] = rng.permutation(ni).astype(np.uint32)
    ml, rp = _lists_matrix(lists, ni)
    score, pos = e.rank_lists(mc, mi, ml)
    ti, ts = e.topk_lists(mc, mi, ml, K)
    # the same call twice
    s2, p2 = e.rank_lists(mc, mi, ml)
    assert _same(score, s2) and np.array_equal(pos, p2)
    # device calls over a partition of the rows (an empty range included)
    for cuts in ([0, nc], [0, 1, 1, 6, 9, nc]):
        ds, dp, di, dt = [], [], [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            cnt = int(rp[b] - rp[a])
            s, q = _device_rank(e, mc, a, b, mi, ml, cnt)
            ds.append(s); dp.append(q)
            i, t = _device_topk(e, mc, a, b, mi, ml, K)
            di.append(i); dt.append(t)
        assert _same(np.concatenate(ds), score) and np.array_equal(np.concatenate(dp), pos)
        assert np.array_equal(np.concatenate(di), ti) and _same(np.concatenate(dt), ts)
    # tiny LDS budgets and chunks: lists longer than the budget take the general path, the others the fused one
    try:
        for lds, chunk in ((1, 1), (4, 3), (1, 3), (4, 1), (1024, 1), (1, 0)):
            L.check(L.lib().fmx_debug_lists_limits(ctypes.c_int32(lds), ctypes.c_int64(chunk)))
            s3, p3 = e.rank_lists(mc, mi, ml)
            assert _same(score, s3) and np.array_equal(pos, p3), (lds, chunk)
            i3, t3 = e.topk_lists(mc, mi, ml, K)
            assert np.array_equal(i3, ti) and _same(t3, ts), (lds, chunk)
            s4, p4 = _device_rank(e, mc, 2, 10, mi, ml, int(rp[10] - rp[2]))
            assert _same(s4, score[rp[2]:rp[10]]) and np.array_equal(p4, pos[rp[2]:rp[10]])
    finally:
        L.check(L.lib().fmx_debug_lists_limits(ctypes.c_int32(0), ctypes.c_int64(0)))
    # another entry order: per distinct candidate the same score and position, and the same top-K
    perm = [rng.permutation(len(x)) for x in lists]
    shuffled = [x[q] for x, q in zip(lists, perm)]
    ml2, _ = _lists_matrix(shuffled, ni)
    s5, p5 = e.rank_lists(mc, mi, ml2)
    for c in range(nc):
        sl = slice(rp[c], rp[c + 1])
        assert _same(s5[sl], score[sl][perm[c]]) and np.array_equal(p5[sl], pos[sl][perm[c]])
    i5, t5 = e.topk_lists(mc, mi, ml2, K)
    assert np.array_equal(i5, ti) and _same(t5, ts)
    # a context alone, and no lists at all
    for c in (0, 8):
        m1, _ = _lists_matrix([lists[c]], ni)
        s6, p6 = e.rank_lists(_mat(_sub(C, c, c + 1), p), mi, m1)
        assert _same(s6, score[rp[c]:rp[c + 1]]) and np.array_equal(p6, pos[rp[c]:rp[c + 1]])
    m0, _ = _lists_matrix([np.zeros(0, np.uint32)] * nc, ni)
    s7, p7 = e.rank_lists(mc, mi, m0)
    assert len(s7) == 0 and len(p7) == 0
    i7, t7 = e.topk_lists(mc, mi, m0, 3)
    assert np.all(i7 == -1) and np.all(np.isnan(t7))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_chunk_without_entries_between_chunks_with_entries(kind):
    """lists of 2, 0, 0 and 3 candidates (one twice) on the general path (budget 1): with chunks of one context the two middle chunks hold
    nothing, with chunks of three the last one is a chunk of its own; scores, positions and top-K are the unhooked call's bits and numpy's order"""
    from fmwr_amd import _lib as L
    p, nc, ni, K = 80, 4, 8, 2
    rng, C, I = _problem(77, ni=ni, nc=nc)
    e = _engine(kind, p, 3)
    mc, mi = _mat(C, p), _mat(I, p)
    lists = [np.array(x, np.uint32) for x in ([1, 5], [], [], [2, 6, 2])]
    ml, rp = _lists_matrix(lists, ni)
    score, pos = e.rank_lists(mc, mi, ml)
    ti, ts = e.topk_lists(mc, mi, ml, K)
    S = _dense_scores(e, mc, mi, ni)
    for c in range(nc):
        lst = lists[c].astype(np.int64)
        sl = slice(rp[c], rp[c + 1])
        assert _same(score[sl], S[c, lst]) and np.array_equal(pos[sl], lists_model.positions(S[c], lst))
    assert np.all(ti[1:3] == -1) and np.all(np.isnan(ts[1:3])) and np.all(ti[[0, 3]] >= 0)
    try:
        for lds, chunk in ((1, 1), (1, 3)):
            L.check(L.lib().fmx_debug_lists_limits(ctypes.c_int32(lds), ctypes.c_int64(chunk)))
            s2, p2 = e.rank_lists(mc, mi, ml)
            assert _same(score, s2) and np.array_equal(pos, p2), (lds, chunk)
            i2, t2 = e.topk_lists(mc, mi, ml, K)
            assert np.array_equal(i2, ti) and _same(t2, ts), (lds, chunk)
    finally:
        L.check(L.lib().fmx_debug_lists_limits(ctypes.c_int32(0), ctypes.c_int64(0)))


def _round_to(x, dt):
    """the Fraction x rounded to the nearest value of the float type dt, ties to even"""
    if dt == np.float64:
        return np.float64(float(x))   # int / int true division: correctly rounded
    f = np.float32(float(x))
    cands = {np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))}
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))


def _chain(sc, si, dt):
    """fma(sc[k-1], si[k-1], ... fma(sc[0], si[0], 0)) with one rounding to dt per step"""
    acc = Fraction(0)
    for a, b in zip(sc, si):
        acc = Fraction(float(_round_to(Fraction(float(a)) * Fraction(float(b)) + acc, dt)))
    return np.float64(float(acc))


@pytest.mark.parametrize("kind", ["seq64", "mb64", "mb32"])
@pytest.mark.parametrize("k", [0, 1, 3, 16])
def test_project_reproduces_the_topk_score(kind, k):
    rng, C, I = _problem(300 + k)
    p, nc, ni = 80, 6, 41
    e = _engine(kind, p, k)
    mc, mi = _mat(C, p), _mat(I, p)
    S = _dense_scores(e, mc, mi, ni)
    bc, s_c = e.project(mc, with_w0=True)
    bi, s_i = e.project(mi, with_w0=False)
    assert s_c.shape == (nc, k) and s_i.shape == (ni, k) and bc.shape == (nc,) and bi.shape == (ni,)
    dt = np.float32 if kind == "mb32" else np.float64
    if kind == "mb32":   # the factor sums are the state type's values, widened exactly
        assert np.array_equal(s_c.astype(np.float32).astype(np.float64), s_c) and np.array_equal(s_i.astype(np.float32).astype(np.float64), s_i)
    assert np.all(np.isfinite(S)) and np.all(bc[:, None] + bi[None, :] != 0)   # (the identity's one exception, a zero dot on a zero base, cannot occur)
    if k == 0:
        got = bc[:, None] + bi[None, :] + 0.0
    elif k == 1:   # one correctly rounded product is the fma onto 0
        dot = (s_c.astype(dt) * s_i.astype(dt).T).astype(np.float64)
        got = (bc[:, None] + bi[None, :]) + dot
    else:
        got = np.array([[(bc[c] + bi[i]) + _chain(s_c[c], s_i[i], dt) for i in range(ni)] for c in range(nc)])
    assert _same(got, S)
    # base: the forward of the row, w0 as the forward adds it
    w0, w, v = e.get_params()
    b0, _ = e.project(mc, with_w0=False)
    A = sp.csr_matrix((np.abs(C[2]).astype(np.float64), C[1], C[0]), shape=(nc, p))
    scale = abs(w0) + A @ np.abs(w) + 0.5 * ((A @ np.abs(v).T) ** 2).sum(1) + 1e-300
    assert np.all(np.abs((bc - b0) - w0) <= 64 * 2.0 ** -52 * scale)   # each side: fewer than 32 fp64 roundings of partial sums no larger than scale
    assert np.all(np.abs(bc - e.predict(mc)) <= RTOL[kind] * scale)
    # row ranges through the device entry point
    for a, b in ((0, ni), (0, 0), (3, 17), (17, ni)):
        db, dsb = DevBuf(b - a), DevBuf((b - a) * k)
        try:
            e.project_device(mi, a, b, db.ptr.value, dsb.ptr.value if k else None)
            e.sync()
            assert _same(db.numpy()[:b - a], bi[a:b]) and _same(dsb.numpy()[:(b - a) * k].reshape(b - a, k), s_i[a:b])
        finally:
            db.free(); dsb.free()


def test_project_without_the_global_bias():
    rng, C, I = _problem(5)
    for kind in ("seq64", "mb32"):
        e = _engine(kind, 80, 3, keep_w0=0)
        b1, s1 = e.project(_mat(C, 80), with_w0=True)
        b0, s0 = e.project(_mat(C, 80), with_w0=False)
        assert _same(b1, b0) and _same(s1, s0)


@pytest.fixture(scope="module")
def movielens_fit():
    import fmwr_amd as fm
    from tests.test_gpu_api import _movielens_shaped
    X, rating = _movielens_shaped()
    y = (rating >= 4).astype(np.float64)
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 8, "L2.w1": 1e-3, "L2.v": 1e-3, "v.init_stdev": 0.05}),
           fm.solver_control(max_iter=100_000, solver=fm.SGD_solver(learn_rate=0.02))]
    return fm.fm_train(fm.fm_matrix(X, y), normalize=False, control=ctl, seed=42), X


def test_fm_rerank_movielens_shaped(movielens_fit):
    import fmwr_amd as fm
    fit, X = movielens_fit
    users, items = 943, 1682
    p = users + items
    rng = np.random.default_rng(0)
    who = rng.choice(users, 20, replace=False)
    ctx = fm.fm_matrix(sp.csr_matrix((np.ones(20), who, np.arange(21)), shape=(20, p)))
    itm = fm.fm_matrix(sp.csr_matrix((np.ones(items), np.arange(items) + users, np.arange(items + 1)), shape=(items, p)))
    K = 10
    # candidates = every item: fm_recommend itself
    every = [rng.permutation(items) for _ in range(20)]
    want = fm.fm_recommend(fit, ctx, itm, top_k=K, normalize=False)
    got = fm.fm_rerank(fit, ctx, itm, every, top_k=K, normalize=False)
    assert np.array_equal(got["index"], want["index"]) and _same(got["score"], want["score"])
    # candidates = every item a user has not rated: the position of a held-out item is fm_recommend_metrics' rank, and the head is fm_recommend's
    Xc = X.tocsr()
    u_of = Xc.indices[Xc.indptr[:-1]]
    i_of = Xc.indices[Xc.indptr[:-1] + 1] - users
    rated = [np.unique(i_of[u_of == u]) for u in who]
    rest = [rng.permutation(np.setdiff1d(np.arange(items), r)) for r in rated]
    held = [np.sort(r[:3]) for r in rest]
    met = fm.fm_recommend_metrics(fit, ctx, itm, held, k=K, exclude=rated, normalize=False, ranks=True)
    cand = sp.csr_matrix((np.ones(sum(len(r) for r in rest)), np.concatenate(rest), np.concatenate([[0], np.cumsum([len(r) for r in rest])])),
                         shape=(20, items))
    out = fm.fm_rerank(fit, ctx, itm, cand, normalize=False)
    assert out["score"].shape == out["position"].shape == (20, items)
    assert np.array_equal(out["position"].indices, cand.indices) and np.array_equal(out["position"].indptr, cand.indptr)
    assert np.array_equal(met["rank"].indices, np.concatenate(held))
    for r in range(20):
        where = {int(j): int(q) for j, q in zip(rest[r], out["position"].data[cand.indptr[r]:cand.indptr[r + 1]])}
        assert [where[int(h)] for h in held[r]] == met["rank"].data[3 * r:3 * r + 3].tolist()
    want = fm.fm_recommend(fit, ctx, itm, top_k=K, exclude=rated, normalize=False)
    got = fm.fm_rerank(fit, ctx, itm, cand, top_k=K, normalize=False)
    assert np.array_equal(got["index"], want["index"]) and _same(got["score"], want["score"])
    # the per-entry scores are the same linked scores, duplicates and all
    dup = [np.concatenate([w[:4], w[:2]]) for w in want["index"]]
    out = fm.fm_rerank(fit, ctx, itm, dup, normalize=False)
    assert out["score"].nnz == 20 * 6
    for r in range(20):
        sl = slice(out["score"].indptr[r], out["score"].indptr[r + 1])
        assert _same(out["score"].data[sl], want["score"][r][[0, 1, 2, 3, 0, 1]])
        assert np.array_equal(out["position"].data[sl], [0, 1, 2, 3, 0, 1])


def test_fm_embed_round_trips_at_one_factor():
    import fmwr_amd as fm
    rng = np.random.default_rng(3)
    p, nc, ni = 30, 7, 19
    ctl = {"model": fm.model_control("REGRESSION", **{"factor.number": 1}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    fit = {"Model": {"w0": 0.25, "w": rng.normal(size=p), "v": rng.normal(size=(1, p)), "model.control": ctl["model"],
                     "solver.control": ctl["solver"], "track.control": ctl["track"]},
           "Scales": {"mean": None, "std": None, "target.range": (-1e300, 1e300)}}   # a clamp that never acts: the scores are raw
    ctx = fm.fm_matrix(sp.random(nc, p, 0.3, random_state=1, format="csr") + sp.eye(nc, p, format="csr"))
    itm = fm.fm_matrix(sp.random(ni, p, 0.3, random_state=2, format="csr") + sp.eye(ni, p, k=5, format="csr"))
    rec = fm.fm_recommend(fit, ctx, itm, top_k=ni, normalize=False)
    ec = fm.fm_embed(fit, ctx, normalize=False, with_w0=True)
    ei = fm.fm_embed(fit, itm, normalize=False)
    assert ec["s"].shape == (nc, 1) and ei["s"].shape == (ni, 1)
    raw = (ec["base"][:, None] + ei["base"][None, :]) + ec["s"] * ei["s"].T   # the model's state is fp64: one rounded product is the fma onto 0
    for c in range(nc):
        assert _same(rec["score"][c], raw[c, rec["index"][c]])


def test_refusals_leave_the_outputs_untouched():
    from fmwr_amd import _lib as L, engine
    rng, C, I = _problem(9)
    p, nc, ni = 80, 6, 41
    e = _engine("mb32", p, 8)
    mc, mi = _mat(C, p), _mat(I, p)
    lists = _random_lists(nc, ni, rng)
    ml, rp = _lists_matrix(lists, ni)
    nnz = int(rp[-1])
    wrong_items, _ = _lists_matrix(lists, ni + 1)           # the column count is not the item count
    wrong_rows, _ = _lists_matrix(lists[:-1], ni)           # one row short
    ds, dp = DevBuf.from_numpy(np.full(nnz, 7.0)), DevBuf.from_numpy(np.full(nnz, 7, np.int64))
    K = 4
    di, dt = DevBuf.from_numpy(np.full(nc * K, 7, np.int64)), DevBuf.from_numpy(np.full(nc * K, 7.0))
    lib = L.lib()

    def rank(lm=ml, link=L.LINK_NONE, r0=0, r1=nc, items=mi):
        return lib.fmx_rank_lists_device(e.h, mc.h, ctypes.c_int64(r0), ctypes.c_int64(r1), items.h, lm.h, ctypes.c_int(link), ds.ptr, dp.ptr)

    def top(lm=ml, top_k=K, link=L.LINK_NONE, r0=0, r1=nc):
        return lib.fmx_topk_lists_device(e.h, mc.h, ctypes.c_int64(r0), ctypes.c_int64(r1), mi.h, lm.h, ctypes.c_int32(top_k), ctypes.c_int(link),
                                         di.ptr, dt.ptr)
    try:
        refused = [rank(lm=wrong_items), rank(lm=wrong_rows), rank(link=4), rank(link=-1), rank(r0=2, r1=nc + 1), rank(r0=-1), rank(r0=3, r1=2),
                   top(lm=wrong_items), top(lm=wrong_rows), top(top_k=0), top(top_k=1025), top(top_k=-1), top(link=7), top(r1=nc + 1)]
        assert all(st == L.ERR_INVALID for st in refused), refused
        assert lib.fmx_last_error().decode()
        other = engine.Engine(p + 1, mode=L.MODE_MINIBATCH, num_factor=8)   # an engine with another feature count
        assert lib.fmx_rank_lists_device(other.h, mc.h, ctypes.c_int64(0), ctypes.c_int64(nc), mi.h, ml.h, ctypes.c_int(0), ds.ptr, dp.ptr) == L.ERR_INVALID
        n_dev = ctypes.c_int32()
        L.check(lib.fmx_device_count(ctypes.byref(n_dev)))
        if n_dev.value > 1:   # lists on another device than the engine's
            rp_ = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
            far = engine.Matrix.from_csr(rp_, np.concatenate(lists), np.ones(nnz, np.float32), ni, device=1)
            assert rank(lm=far) == L.ERR_INVALID and top(lm=far) == L.ERR_INVALID
        # (a factor count above fmx_topk's limit cannot be built: engines hold at most 128 factors, the limit is 256 floats / 128 doubles)
        with pytest.raises(L.FmxError):
            engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=129)
        e.sync()
        assert np.all(ds.numpy() == 7.0) and np.all(dp.numpy() == 7) and np.all(di.numpy() == 7) and np.all(dt.numpy() == 7.0)
        # the host forms refuse the same way, and write nothing
        hs, hp = np.full(nnz, 7.0), np.full(nnz, 7, np.int64)
        st = lib.fmx_rank_lists(e.h, mc.h, mi.h, wrong_items.h, ctypes.c_int(0), hs.ctypes.data_as(ctypes.c_void_p), hp.ctypes.data_as(ctypes.c_void_p))
        assert st == L.ERR_INVALID and np.all(hs == 7.0) and np.all(hp == 7)
        hi, ht = np.full(nc * K, 7, np.int64), np.full(nc * K, 7.0)
        st = lib.fmx_topk_lists(e.h, mc.h, mi.h, ml.h, ctypes.c_int32(2000), ctypes.c_int(0), hi.ctypes.data_as(ctypes.c_void_p), ht.ctypes.data_as(ctypes.c_void_p))
        assert st == L.ERR_INVALID and np.all(hi == 7) and np.all(ht == 7.0)
        # an empty range is fine and writes nothing
        assert rank(r0=3, r1=3) == L.OK and top(r0=nc, r1=nc) == L.OK
        e.sync()
        assert np.all(ds.numpy() == 7.0) and np.all(di.numpy() == 7)
        # and the same buffers take a real call afterwards
        assert rank() == L.OK and top() == L.OK
        e.sync()
        score, pos = e.rank_lists(mc, mi, ml)
        assert _same(ds.numpy(), score) and np.array_equal(dp.numpy(), pos)
    finally:
        for b in (ds, dp, di, dt):
            b.free()


def test_parameters_are_not_modified():
    rng, C, I = _problem(4)
    e = _engine("mb32", 80, 8)
    before = e.get_params()
    ml, _ = _lists_matrix(_random_lists(6, 41, rng), 41)
    e.rank_lists(_mat(C, 80), _mat(I, 80), ml)
    e.topk_lists(_mat(C, 80), _mat(I, 80), ml, 5)
    e.project(_mat(I, 80))
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
