"""fmx_diversify / fmx_diversify_device / fm_diversify: greedy MMR selection over ranked pools, held to tests/diversify_model.py in every bit
(the sign of a zero margin canonicalised: the zero-padded chain can turn -0 into +0), to fmx_topk / fmx_topk_lists at lambda = 1, and to
itself across forms, chunks, calls and slot orders."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from tests import diversify_model as dm
from tests.test_gpu_topk import _csr, _engine, _mat
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

NI = 300
LAMBDAS = (0.0, 0.3, 0.7, 1.0)
MODES = (dm.REL_SCORE, dm.REL_MINMAX)


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(a == 0, 0.0, a).view(np.uint64)   # the sign of a zero is canonicalised


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same3(got, want):
    return np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and _same(got[2], want[2])


def _cached(chain):
    """`chain` with every (row, vector) pair computed once: the Fraction emulation is the slow part of these tests"""
    cache = {}

    def f(rows, v):
        vb = np.ascontiguousarray(v).tobytes()
        out = np.empty(len(rows))
        for q, r in enumerate(rows):
            key = (np.ascontiguousarray(r).tobytes(), vb)
            if key not in cache:
                cache[key] = chain(r[None, :], v)[0]
            out[q] = cache[key]
        return out
    return f


def _one_hot_engine(kind, k, v, monkeypatch=None):
    """an engine over NI features whose item i is the one-hot row of feature i: s_i is column i of v, in the state type"""
    from fmwr_amd import engine
    if kind == "mb32w":
        monkeypatch.setenv("FMX_W_IN_ROW", "1")
    e = _engine("mb32" if kind == "mb32w" else kind, NI, k)
    if kind == "mb32w":
        assert e.w_in_row()
    rng = np.random.default_rng(k)
    e.set_params(0.1, rng.normal(0, 0.5, NI), v)
    mi = engine.Matrix.from_csr(np.arange(NI + 1, dtype=np.int64), np.arange(NI, dtype=np.uint32), np.ones(NI, np.float32), NI)
    _, s = e.project(mi)
    return e, mi, s


def _pools(rng, P, n, zero_item=None):
    """n pools of P slots with the edge cases of the CPU tests: row 0 distinct items and plain scores; row 1 ties by item, duplicate items and
    sprinkled -1 slots; row 2 only empty slots; row 3 a NaN score, +-inf scores and the item whose projection is zero; the others random"""
    index = np.array([rng.permutation(NI)[:P] if P <= NI else rng.integers(0, NI, P) for _ in range(n)], np.int64)
    score = rng.normal(0, 1, (n, P))
    if n > 1:
        score[1] = np.round(score[1])
        if P > 2:
            index[1, 2] = index[1, 0]
            index[1, rng.integers(0, P, max(1, P // 8))] = -1
            score[1, 2] = score[1, 0]
    if n > 2:
        index[2] = -1
    if n > 3:
        score[3, 0] = np.nan
        if P > 3:
            score[3, 1], score[3, 3] = np.inf, -np.inf
        if zero_item is not None and P > 1:
            index[3, P // 2] = zero_item
    return index, score


KINDS = [("seq64", k) for k in (0, 1, 3, 16, 64, 100)] + [("mb64", k) for k in (0, 1, 3, 16, 64, 100)] + \
        [("mb32", k) for k in (0, 1, 3, 16, 64, 100)] + [("mb32w", k) for k in (1, 3, 16)]


@pytest.mark.parametrize("kind,k", KINDS)
def test_random_factors_equal_the_model_bit_for_bit(kind, k, monkeypatch):
    """random V: the Fraction emulation of the chain is the model (K = P only where it is cheap: k <= 3)"""
    rng = np.random.default_rng(1000 + k)
    v = rng.normal(0, 0.4, (k, NI))
    if k:
        v[:, 7] = 0.0
    e, mi, s = _one_hot_engine(kind, k, v, monkeypatch)
    dt = np.float32 if kind in ("mb32", "mb32w") else np.float64
    if dt == np.float32:
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    chain = _cached(dm.chain_exact(dt))
    inv = dm.norms_inv(s, chain)
    assert inv[7] == 0.0 or k == 0
    for P in (1, 2, 63, 65):
        index, score = _pools(rng, P, 4, zero_item=7)
        Ks = sorted({1, min(2, P), P if k <= 3 else min(P, 4)})
        for lam in LAMBDAS:
            for mode in MODES:
                want = dm.diversify_rows(s, index, score, Ks[-1], lam, mode, chain, inv)
                for K in Ks:
                    got = e.diversify(mi, index, score, K, lam, mode)
                    assert _same3(got, [w[:, :K] for w in want]), (P, K, lam, mode, got, want)
                assert np.all(want[0][2] == -1) and np.all(np.isnan(want[2][2]))


@pytest.mark.parametrize("kind,k", KINDS)
def test_large_pools_equal_the_model_bit_for_bit(kind, k, monkeypatch):
    """V in eighths: every chain is exact in fp32 and a float64 dot product is the model; the pools sit on the wave, workgroup and
    slots-per-thread edges and reach both the LDS and the global form"""
    rng = np.random.default_rng(2000 + k)
    v = rng.integers(-8, 9, (k, NI)) / 8.0
    if k:
        v[:, 11] = 0.0
    e, mi, s = _one_hot_engine(kind, k, v, monkeypatch)
    assert np.array_equal(s, v.T)
    inv = dm.norms_inv(s, dm.chain_dot)
    for P in (64, 255, 256, 257, 1024):
        n = 4 if P < 1024 else 3
        index, score = _pools(rng, P, n, zero_item=11)
        configs = [(lam, mode) for lam in LAMBDAS for mode in MODES] if P == 64 else [(0.3, dm.REL_MINMAX), (0.7, dm.REL_SCORE), (0.0, dm.REL_SCORE),
                                                                                      (1.0, dm.REL_MINMAX)]
        for lam, mode in configs:
            want = dm.diversify_rows(s, index, score, P, lam, mode, dm.chain_dot, inv)
            for K in (1, 2, P):
                got = e.diversify(mi, index, score, K, lam, mode)
                assert _same3(got, [w[:, :K] for w in want]), (P, K, lam, mode)
        # K beyond the non-empty slots: the tail is -1 / NaN / NaN
        assert np.all(want[0][1, -1:] == -1) and np.all(want[0][2] == -1)


def _problem(seed, ni=41, nc=6, p=80):
    rng = np.random.default_rng(seed)
    return rng, _csr(nc, 0, 40, 6, rng), _csr(ni, 40, 80, 4, rng)


def _lists_matrix(lists, ni):
    from fmwr_amd import engine
    rp = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    col = np.concatenate([np.asarray(x, np.uint32) for x in lists]) if rp[-1] else np.zeros(0, np.uint32)
    return engine.Matrix.from_csr(rp, col, np.ones(int(rp[-1]), np.float32), ni)


@pytest.mark.parametrize("kind", ["seq64", "mb64", "mb32"])
@pytest.mark.parametrize("k", [0, 3, 16])
def test_lambda_one_is_fmx_topk_and_fmx_topk_lists(kind, k):
    """consequence a on pools the two calls produce (item rows of up to four real-valued entries), and the model on the same pools"""
    rng, C, I = _problem(40 + k)
    ni, nc, p = 41, 6, 80
    e = _engine(kind, p, k)
    mc, mi = _mat(C, p), _mat(I, p)
    pool_i, pool_s = e.topk(mc, mi, ni)
    for K in (1, 5, ni):
        wi, ws = e.topk(mc, mi, K)
        gi, gs, gm = e.diversify(mi, pool_i, pool_s, K, 1.0, dm.REL_SCORE)
        assert np.array_equal(gi, wi) and _same(gs, ws) and _same(gm, ws - 0.0)
        assert np.array_equal(np.ascontiguousarray(gs).view(np.uint64), np.ascontiguousarray(ws).view(np.uint64))   # the given score's bits, signs included
    lists = [rng.integers(0, ni, int(rng.integers(2, 60))).astype(np.uint32) for _ in range(nc)]
    lists[1] = np.zeros(0, np.uint32)
    lists[3] = np.array([ni - 1], np.uint32)
    ml = _lists_matrix(lists, ni)
    P = 32
    pool_i, pool_s = e.topk_lists(mc, mi, ml, P)
    assert np.all(pool_i[1] == -1) and (pool_i == -1).any(axis=1).sum() >= 2
    for K in (1, 7, P):
        wi, ws = e.topk_lists(mc, mi, ml, K)
        gi, gs, gm = e.diversify(mi, pool_i, pool_s, K, 1.0, dm.REL_SCORE)
        assert np.array_equal(gi, wi) and _same(gs, ws)
    # the model on these pools, with the norms implied by fmx_project's output
    dt = np.float32 if kind == "mb32" else np.float64
    _, s = e.project(mi)
    chain = _cached(dm.chain_exact(dt))
    for lam, mode in ((0.5, dm.REL_MINMAX), (0.2, dm.REL_SCORE)):
        want = dm.diversify_rows(s, pool_i, pool_s, 6, lam, mode, chain)
        assert _same3(e.diversify(mi, pool_i, pool_s, 6, lam, mode), want)


def _device(e, mi, index, score, K, lam, mode, margin=True):
    n, P = index.shape
    di, ds = DevBuf.from_numpy(index), DevBuf.from_numpy(score)
    oi, os_, om = DevBuf(n * K, np.int64), DevBuf(n * K), DevBuf(n * K)
    try:
        e.diversify_device(mi, n, P, di.ptr.value, ds.ptr.value, K, lam, mode, oi.ptr.value, os_.ptr.value, om.ptr.value if margin else None)
        e.sync()
        return oi.numpy().reshape(n, K), os_.numpy().reshape(n, K), om.numpy().reshape(n, K)
    finally:
        for b in (di, ds, oi, os_, om):
            b.free()


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_invariance_over_forms_chunks_rows_order_and_calls(kind):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(77)
    k = 16
    e, mi, s = _one_hot_engine(kind, k, rng.normal(0, 0.4, (k, NI)))
    before = e.get_params()
    lib = L.lib()
    for P, K in ((65, 9), (257, 12)):
        n = 5
        index = np.array([rng.permutation(NI)[:P] for _ in range(n)], np.int64)   # distinct items in every row
        score = rng.normal(0, 1, (n, P))
        index[3, ::5] = -1
        for lam, mode in ((0.3, dm.REL_MINMAX), (0.7, dm.REL_SCORE)):
            ref = e.diversify(mi, index, score, K, lam, mode)
            assert (ref[0][0] >= 0).all()
            assert _same3(e.diversify(mi, index, score, K, lam, mode), ref)              # d: the same bits on every call
            assert _same3(_device(e, mi, index, score, K, lam, mode), ref)               # the device form
            dev = _device(e, mi, index, score, K, lam, mode, margin=False)               # ... without a margin buffer
            assert np.array_equal(dev[0], ref[0]) and _same(dev[1], ref[1])
            for c in (0, 3):                                                             # b: a row alone, a row range
                assert _same3(e.diversify(mi, index[c:c + 1], score[c:c + 1], K, lam, mode), [r[c:c + 1] for r in ref])
            assert _same3(_device(e, mi, index[1:4], score[1:4], K, lam, mode), [r[1:4] for r in ref])
            q = rng.permutation(P)                                                       # b: the order of the slots
            assert _same3(e.diversify(mi, index[:, q], score[:, q], K, lam, mode), ref)
            for K1 in (1, 2, K - 1):                                                     # c: prefix
                assert _same3(e.diversify(mi, index, score, K1, lam, mode), [r[:, :K1] for r in ref])
            try:                                                                         # b: the internal form and the chunking
                for rows, chunk in ((-1, 0), (-1, 1), (0, 1), (0, 2), (64, 2), (1024, 0)):
                    L.check(lib.fmx_debug_diversify_limits(ctypes.c_int32(rows), ctypes.c_int64(chunk)))
                    assert _same3(e.diversify(mi, index, score, K, lam, mode), ref), (rows, chunk)
                    assert _same3(_device(e, mi, index, score, K, lam, mode), ref), (rows, chunk)
            finally:
                L.check(lib.fmx_debug_diversify_limits(ctypes.c_int32(0), ctypes.c_int64(0)))
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_refusals_leave_the_outputs_untouched():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(5)
    e, mi, s = _one_hot_engine("mb32", 8, rng.normal(0, 0.4, (8, NI)))
    n, P, K = 3, 10, 4
    index = np.array([rng.permutation(NI)[:P] for _ in range(n)], np.int64)
    score = rng.normal(0, 1, (n, P))
    di, ds = DevBuf.from_numpy(index), DevBuf.from_numpy(score)
    oi, os_, om = DevBuf.from_numpy(np.full(n * K, 7, np.int64)), DevBuf.from_numpy(np.full(n * K, 7.0)), DevBuf.from_numpy(np.full(n * K, 7.0))
    lib = L.lib()
    other = engine.Engine(NI + 1, mode=L.MODE_MINIBATCH, num_factor=8)   # an engine with another feature count

    def dev(eng=e, n=n, pool=P, top_k=K, lam=0.5, rel=0):
        return lib.fmx_diversify_device(eng.h, mi.h, n, pool, di.ptr, ds.ptr, top_k, lam, rel, oi.ptr, os_.ptr, om.ptr)

    hi, hs, hm = np.full((n, K), 7, np.int64), np.full((n, K), 7.0), np.full((n, K), 7.0)

    def host(idx=index, n=n, pool=P, top_k=K, lam=0.5, rel=0):
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        return lib.fmx_diversify(e.h, mi.h, n, pool, p(idx), p(score), top_k, lam, rel, p(hi), p(hs), p(hm))
    try:
        refused = [dev(pool=0), dev(pool=1025, top_k=4), dev(top_k=0), dev(top_k=P + 1), dev(top_k=-1), dev(lam=-0.1), dev(lam=1.5), dev(lam=float("nan")),
                   dev(rel=2), dev(rel=-1), dev(eng=other), dev(n=-1)]
        assert all(st == L.ERR_INVALID for st in refused), refused
        assert lib.fmx_last_error().decode()
        n_dev = ctypes.c_int32()
        L.check(lib.fmx_device_count(ctypes.byref(n_dev)))
        if n_dev.value > 1:   # items on another device than the engine's
            far = engine.Matrix.from_csr(np.arange(NI + 1, dtype=np.int64), np.arange(NI, dtype=np.uint32), np.ones(NI, np.float32), NI, device=1)
            assert lib.fmx_diversify_device(e.h, far.h, n, P, di.ptr, ds.ptr, K, 0.5, 0, oi.ptr, os_.ptr, om.ptr) == L.ERR_INVALID
        assert lib.fmx_diversify_device(e.h, mi.h, n, P, None, ds.ptr, K, 0.5, 0, oi.ptr, os_.ptr, om.ptr) == L.ERR_INVALID
        e.sync()
        assert np.all(oi.numpy() == 7) and np.all(os_.numpy() == 7.0) and np.all(om.numpy() == 7.0)
        # the host form refuses the same way, and an index that is neither -1 nor an item row (the device form cannot check that)
        bad_hi, bad_lo = index.copy(), index.copy()
        bad_hi[1, 3], bad_lo[2, 0] = NI, -2
        refused = [host(pool=0), host(top_k=P + 1), host(lam=float("nan")), host(lam=2.0), host(rel=5), host(idx=bad_hi), host(idx=bad_lo)]
        assert all(st == L.ERR_INVALID for st in refused), refused
        assert b"index[2][0]" in lib.fmx_last_error()
        assert np.all(hi == 7) and np.all(hs == 7.0) and np.all(hm == 7.0)
        # n == 0 is fine and writes nothing
        assert dev(n=0) == L.OK and host(n=0) == L.OK
        e.sync()
        assert np.all(oi.numpy() == 7) and np.all(hi == 7)
        # the device form takes such indices as empty slots, and the same buffers take a real call afterwards
        want = e.diversify(mi, np.where(bad_hi == NI, -1, index), score, K, 0.5, 0)
        di.upload(bad_hi)
        assert dev() == L.OK
        e.sync()
        assert _same3((oi.numpy().reshape(n, K), os_.numpy().reshape(n, K), om.numpy().reshape(n, K)), want)
        assert host() == L.OK and _same3((hi, hs, hm), e.diversify(mi, index, score, K, 0.5, 0))
    finally:
        for b in (di, ds, oi, os_, om):
            b.free()


def _fit(rng, p, k):
    import fmwr_amd as fm
    ctl = {"model": fm.model_control("REGRESSION", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    return {"Model": {"w0": 0.25, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"],
                      "solver.control": ctl["solver"], "track.control": ctl["track"]},
            "Scales": {"mean": None, "std": None, "target.range": (-1e300, 1e300)}}   # a clamp that never acts


def test_fm_diversify():
    import fmwr_amd as fm
    rng = np.random.default_rng(12)
    p, nc, ni, k = 60, 7, 150, 4
    fit = _fit(rng, p, k)
    ctx = fm.fm_matrix(sp.random(nc, p, 0.2, random_state=1, format="csr") + sp.eye(nc, p, format="csr"))
    itm = fm.fm_matrix(sp.random(ni, p, 0.1, random_state=2, format="csr") + sp.eye(ni, p, k=3, format="csr"))
    # trade_off = 1 on the score itself: fm_recommend and fm_rerank(top_k)
    rec = fm.fm_recommend(fit, ctx, itm, top_k=10, normalize=False)
    got = fm.fm_diversify(fit, ctx, itm, top_k=10, trade_off=1.0, relevance="score", normalize=False)
    assert set(got) == {"index", "score", "margin"} and got["index"].shape == got["score"].shape == got["margin"].shape == (nc, 10)
    assert np.array_equal(got["index"], rec["index"]) and _same(got["score"], rec["score"])
    excl = [rng.choice(ni, 20, replace=False) for _ in range(nc)]
    rec = fm.fm_recommend(fit, ctx, itm, top_k=10, exclude=excl, normalize=False)
    got = fm.fm_diversify(fit, ctx, itm, top_k=10, trade_off=1.0, exclude=excl, relevance="score", normalize=False)
    assert np.array_equal(got["index"], rec["index"]) and _same(got["score"], rec["score"])
    cand = [rng.choice(ni, int(rng.integers(3, 40)), replace=False) for _ in range(nc)]
    rer = fm.fm_rerank(fit, ctx, itm, cand, top_k=5, normalize=False)
    got = fm.fm_diversify(fit, ctx, itm, top_k=5, trade_off=1.0, candidates=cand, pool=40, relevance="score", normalize=False)
    assert np.array_equal(got["index"], rer["index"]) and _same(got["score"], rer["score"])
    # the default pool is min(1024, n_items, max(100, 10 top_k)) = 100 here: the call is the engine's on fm_recommend(top_k = 100)'s pool
    div = fm.fm_diversify(fit, ctx, itm, top_k=10, normalize=False)
    pool = fm.fm_recommend(fit, ctx, itm, top_k=100, normalize=False)
    emb = fm.fm_embed(fit, itm, normalize=False)["s"]
    want = dm.diversify_rows(emb, pool["index"], pool["score"], 10, 0.7, dm.REL_MINMAX, _cached(dm.chain_exact(np.float64)))
    assert _same3((div["index"], div["score"], div["margin"]), want)
    assert not np.array_equal(div["index"], pool["index"][:, :10])     # (it does diversify)
    assert np.array_equal(div["index"][:, 0], pool["index"][:, 0])     # the first pick is the best-scored item
    small = fm.fm_diversify(fit, ctx, itm, top_k=3, pool=3, exclude=excl, normalize=False)
    assert sorted(small["index"][0]) == sorted(fm.fm_recommend(fit, ctx, itm, top_k=3, exclude=excl, normalize=False)["index"][0])
    for kw, err in (({"candidates": cand, "exclude": excl}, ValueError), ({"top_k": 0}, ValueError), ({"top_k": 5, "pool": 4}, ValueError),
                    ({"pool": 2000}, ValueError), ({"trade_off": 1.5}, ValueError), ({"trade_off": float("nan")}, ValueError),
                    ({"relevance": "rank"}, ValueError), ({"top_k": 2.5}, ValueError)):
        with pytest.raises(err):
            fm.fm_diversify(fit, ctx, itm, normalize=False, **kw)
