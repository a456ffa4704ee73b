"""fmx_neighbors / fmx_neighbors_device / fm_similar: the K most similar rows by the cosine (or the dot product) of the projections, held to
tests/neighbors_model.py in every bit (the sign of a zero canonicalised: the zero-padded chain can turn -0 into +0; a NaN equals any NaN), to
fmx_diversify's similarity on the device, and to itself across slices, chunks, row ranges, batches and calls.

Items are one-hot rows (item i = feature i), so s_i is column i of V, read back through fmx_project.  Where the Fraction emulation of the chain
is too slow the factors are eighths (times a power of two): every partial sum of a chain is then exact in fp32 and a float64 dot product,
narrowed to the state type, is the chain.  Two refusals cannot be reached from a test: items->n >= 2^31 - 1 needs a matrix of 2^31 rows, and an
engine holds at most 128 factors, which is the selection's limit for doubles and half of it for floats."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from tests import diversify_model as dm
from tests import neighbors_model as nm
from tests.test_gpu_topk import _engine
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

NI = 600
METRICS = (nm.SIM_COSINE, nm.SIM_DOT)
QROWS = [0, 5, 8, 9, 10, 11, 12, 13, 20]   # nine queries (a tile of eight and one more), the edge rows among them
BIG = 2.0 ** 70                            # times eighths: the fp32 chain of such a row with itself overflows


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    a = np.where(np.isnan(a), dm.QNAN, np.where(a == 0, 0.0, a))   # one NaN, one zero
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eq(got, want):
    return np.array_equal(got[0], want[0]) and _same(got[1], want[1])


def _dt(kind):
    return np.float32 if kind in ("mb32", "mb32w") else np.float64


def _chain_exact_sums(dt):
    """the chain of rows whose partial sums are exact in dt, or grow monotonically past its range: the float64 dot product narrowed to dt"""
    if dt == np.float64:
        return dm.chain_dot

    def chain(rows, v):
        with np.errstate(all="ignore"):
            return np.asarray(dm.chain_dot(rows, v), np.float64).astype(np.float32).astype(np.float64)
    return chain


def _one_hot(ids, p=NI):
    from fmwr_amd import engine
    ids = np.asarray(ids, np.uint32)
    return engine.Matrix.from_csr(np.arange(len(ids) + 1, dtype=np.int64), ids, np.ones(len(ids), np.float32), p)


def _setup(kind, k, v, monkeypatch=None):
    """an engine over NI features holding v, the matrix of all NI one-hot items and their projections"""
    if kind == "mb32w":
        monkeypatch.setenv("FMX_W_IN_ROW", "1")
    e = _engine("mb32" if kind == "mb32w" else kind, NI, k)
    if kind == "mb32w":
        assert e.w_in_row()
    rng = np.random.default_rng(k)
    e.set_params(0.1, rng.normal(0, 0.5, NI), v)
    mi = _one_hot(np.arange(NI))
    _, s = e.project(mi)
    return e, mi, s


def _eighths(rng, k, edges=True):
    """V in eighths with the edge columns: 5 zero, 9 = 8, 11 = -10, 13 = 12 scaled by 2^70 (its fp32 norm is inf), 20 with a NaN factor"""
    v = rng.integers(-8, 9, (k, NI)) / 8.0
    if k and edges:
        v[0, [8, 10, 12]] = [0.5, -0.75, 1.0]      # no zero row among the partners
        v[:, 5] = 0.0
        v[:, 9] = v[:, 8]
        v[:, 11] = -v[:, 10]
        v[:, 13] = v[:, 12] * BIG
        v[0, 20] = np.nan
    return v


class _Limits:
    """fmx_debug_neighbors_limits for a with-block (sticky: restored on exit)"""
    def __init__(self, slice_items, chunk_rows):
        self.args = (slice_items, chunk_rows)

    def __enter__(self):
        from fmwr_amd import _lib as L
        L.check(L.lib().fmx_debug_neighbors_limits(*self.args))

    def __exit__(self, *exc):
        from fmwr_amd import _lib as L
        L.check(L.lib().fmx_debug_neighbors_limits(0, 0))


def _device(e, mq, r0, r1, mi, K, metric=nm.SIM_COSINE, skip=False):
    n = r1 - r0
    oi, os_ = DevBuf(n * K, np.int64), DevBuf(n * K)
    try:
        e.neighbors_device(mq, r0, r1, mi, K, oi.ptr.value, os_.ptr.value, metric=metric, skip_self=skip)
        e.sync()
        return oi.numpy().reshape(n, K), os_.numpy().reshape(n, K)
    finally:
        oi.free(); os_.free()


KINDS = [(kind, k) for kind in ("seq64", "mb64", "mb32") for k in (0, 1, 3, 16, 17, 64, 100)] + [("mb32w", k) for k in (1, 3, 16)]


@pytest.mark.parametrize("kind,k", KINDS)
def test_engine_kinds_and_factors_equal_the_model_bit_for_bit(kind, k, monkeypatch):
    """eighths with the edge rows against all NI items (three slices under the hook, the default slicing without), both metrics -- FMX_SIM_DOT
    where the norm of a row is inf or NaN included -- then random factors against the Fraction chain on a few rows"""
    rng = np.random.default_rng(3000 + k)
    dt = _dt(kind)
    v = _eighths(rng, k)
    e, mi, s = _setup(kind, k, v, monkeypatch)
    assert np.array_equal(s, v.T, equal_nan=True)
    chain = _chain_exact_sums(dt)
    mq, sq = _one_hot(QROWS), s[QROWS]
    K = 10
    for metric in METRICS:
        sc = nm.scores(sq, s, metric, chain)
        want = nm.select(sc, K)
        if k and metric == nm.SIM_COSINE:
            assert np.all(sc[1] == 0) and np.all(sc[7] == 0) == (dt == np.float32) and np.all(sc[8] == 0)   # zero row, inf norm, NaN norm
        if k:
            assert np.array_equal(sc[:, 8], sc[:, 9], equal_nan=True)                                    # the twins tie: the lower index first
        if k and metric == nm.SIM_DOT:
            assert np.all(np.isnan(sc[8])) and np.all(want[0][:, :K] != 20)                              # a NaN score is last
            assert np.isinf(sc[7, 13]) == (dt == np.float32)
        if k == 0:
            assert np.all(want[0] == np.arange(K)) and np.all(want[1].view(np.uint64) == 0)              # every score +0.0: the lowest indices
        got = e.neighbors(mq, mi, K, metric=metric)
        assert _eq(got, want), (metric, got, want)
        with _Limits(256, 0):
            assert _eq(e.neighbors(mq, mi, K, metric=metric), want), metric
        # every item against every item, a row never its own neighbour
        want = nm.select(nm.scores(s, s, metric, chain), K, skip_self=True)
        assert _eq(e.neighbors(mi, mi, K, metric=metric, skip_self=True), want), metric
    if k == 0:
        return
    # random factors: the Fraction emulation of the chain is the model
    nb, nq = 24, 2
    v = rng.normal(0, 0.4, (k, NI))
    v[:, 3] = 0.0
    e.set_params(0.1, rng.normal(0, 0.5, NI), v)
    ms = _one_hot(np.arange(nb))
    _, s = e.project(ms)
    if dt == np.float32:
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
    for metric in METRICS:
        want = nm.neighbors(s[:nq], s, nb, metric, dm.chain_exact(dt))
        got = e.neighbors(_one_hot(np.arange(nq)), ms, nb, metric=metric)
        assert _eq(got, want), (metric, got, want)


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_item_counts_on_the_slice_and_workgroup_edges(kind):
    """1, 255, 256, 257 and 600 items: one, two and three slices of 256 under the hook (a partial last one, a round with idle threads), and the
    same bits from the default slicing"""
    rng = np.random.default_rng(31)
    k = 3
    e, mi, s = _setup(kind, k, _eighths(rng, k))
    chain = _chain_exact_sums(_dt(kind))
    for ni in (1, 255, 256, 257, 600):
        mn = _one_hot(np.arange(ni))
        for metric in METRICS:
            want = nm.neighbors(s[:ni], s[:ni], 10, metric, chain, skip_self=True)
            assert _eq(e.neighbors(mn, mn, 10, metric=metric, skip_self=True), want), (ni, metric)
            with _Limits(256, 0):
                assert _eq(e.neighbors(mn, mn, 10, metric=metric, skip_self=True), want), (ni, metric)
            with _Limits(200, 0):   # rounded up to 256
                assert _eq(e.neighbors(mn, mn, 10, metric=metric, skip_self=True), want), (ni, metric)
        if ni == 1:
            assert want[0][0, 0] == -1   # its only item is itself


@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_query_counts_and_top_k_on_the_tile_edges(kind):
    """tiles of 8 (top_k <= 256), 4 (<= 768) and 2 queries; top_k on the buffer-size boundaries; top_k beyond the items: padding; prefixes"""
    rng = np.random.default_rng(32)
    k = 3
    e, mi, s = _setup(kind, k, _eighths(rng, k))
    chain = _chain_exact_sums(_dt(kind))
    for metric in METRICS:
        full = nm.select(nm.scores(s[QROWS], s, metric, chain), 1024)
        assert np.all(full[0][:, NI:] == -1) and np.all(np.isnan(full[1][:, NI:])) and np.all(full[0][:, :NI] >= 0)
        cases = [(1, 10), (8, 10), (9, 10), (9, 256), (5, 300), (3, 800)] + [(2, K) for K in (1, 256, 257, 768, 769, 1024)]
        for nq, K in cases:
            mq = _one_hot(QROWS[:nq])
            want = (full[0][:nq, :K], full[1][:nq, :K])
            assert _eq(e.neighbors(mq, mi, K, metric=metric), want), (metric, nq, K)
            with _Limits(256, 0):
                assert _eq(e.neighbors(mq, mi, K, metric=metric), want), (metric, nq, K)


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_adverse_order_flushes_every_round(kind):
    """the similarity to query 0 rises with the item index: every item beats the running threshold and the buffer is sorted after every round"""
    k = 2
    v = np.zeros((k, NI))
    v[0], v[1] = np.arange(NI), NI
    v[:, 0] = [1.0, 0.0]
    e, mi, s = _setup(kind, k, v)
    assert np.array_equal(s, v.T)
    chain = _chain_exact_sums(_dt(kind))     # integers below 2^24: every partial sum is exact
    mq = _one_hot([0, 1, NI - 1])
    for metric in METRICS:
        sc = nm.scores(s[[0, 1, NI - 1]], s, metric, chain)
        assert np.all(np.diff(sc[0, 1:]) > 0)
        for K in (5, 300, 800):
            want = nm.select(sc, K)
            if K == 5:
                assert list(want[0][0][1:] if metric == nm.SIM_COSINE else want[0][0][:4]) == [NI - 1, NI - 2, NI - 3, NI - 4]
            assert _eq(e.neighbors(mq, mi, K, metric=metric), want), (metric, K)
            with _Limits(256, 0):
                assert _eq(e.neighbors(mq, mi, K, metric=metric), want), (metric, K)


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_invariance_over_batches_ranges_chunks_halves_and_calls(kind):
    rng = np.random.default_rng(33)
    k, K = 16, 12
    e, mi, s = _setup(kind, k, rng.normal(0, 0.4, (k, NI)))
    before = e.get_params()
    ids = rng.permutation(NI)[:20]
    mq = _one_hot(ids)
    for metric in METRICS:
        ref = e.neighbors(mq, mi, K, metric=metric)
        own = e.neighbors(mi, mi, K, metric=metric, skip_self=True)
        assert np.all(ref[0] >= 0) and not (own[0] == np.arange(NI)[:, None]).any()
        assert _eq(e.neighbors(mq, mi, K, metric=metric), ref)                                   # two calls in a row
        for c in (0, 7, 19):                                                                     # one query alone
            assert _eq(e.neighbors(_one_hot(ids[c:c + 1]), mi, K, metric=metric), [r[c:c + 1] for r in ref])
        perm = rng.permutation(20)                                                               # a permuted batch
        assert _eq(e.neighbors(_one_hot(ids[perm]), mi, K, metric=metric), [r[perm] for r in ref])
        assert _eq(_device(e, mq, 0, 20, mi, K, metric), ref)                                    # the device form, and a sub-range of it:
        assert _eq(_device(e, mq, 3, 14, mi, K, metric), [r[3:14] for r in ref])
        assert _eq(_device(e, mi, 100, 131, mi, K, metric, skip=True), [r[100:131] for r in own])  # skip_self goes by the absolute row
        for chunk in (1, 3, 8):                                                                  # chunks of queries, slices of items
            with _Limits(256, chunk):
                assert _eq(e.neighbors(mq, mi, K, metric=metric), ref), chunk
                assert _eq(_device(e, mi, 250, 270, mi, K, metric, skip=True), [r[250:270] for r in own]), chunk
            with _Limits(0, chunk):
                assert _eq(e.neighbors(mq, mi, K, metric=metric), ref), chunk
        lo = e.neighbors(mq, _one_hot(np.arange(300)), K, metric=metric)                         # the two halves of the items, merged in numpy
        hi = e.neighbors(mq, _one_hot(np.arange(300, NI)), K, metric=metric)
        idx = np.concatenate([lo[0], hi[0] + 300], axis=1)
        sc = np.concatenate([lo[1], hi[1]], axis=1)
        for q in range(20):
            dense = np.full(NI, np.nan)
            dense[idx[q]] = sc[q]
            o = nm.order(dense, np.sort(idx[q]))[:K]
            assert np.array_equal(o, ref[0][q]) and _same(dense[o], ref[1][q])
        for K1 in (1, 5):                                                                        # prefix
            assert _eq(e.neighbors(mq, mi, K1, metric=metric), [r[:, :K1] for r in ref])
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
def test_the_cosine_is_fmx_diversify_s_similarity(kind):
    """for items a < b, fmx_diversify on the pool [a, b] with equal scores and lambda = 0 picks a, then b with the margin -sim(b, a): the cosine
    fmx_neighbors gives (query = row b, item = row a), in every bit"""
    rng = np.random.default_rng(34)
    k = 16
    e, mi, s = _setup(kind, k, rng.normal(0, 0.4, (k, NI)))
    idx, sc = e.neighbors(mi, mi, NI)
    cos = np.full((NI, NI), np.nan)
    cos[np.arange(NI)[:, None], idx] = sc
    assert not np.isnan(cos).any()
    pairs = np.sort(np.array([rng.choice(NI, 2, replace=False) for _ in range(48)]), axis=1).astype(np.int64)
    gi, gs, gm = e.diversify(mi, pairs, np.ones(pairs.shape), 2, 0.0, dm.REL_SCORE)
    assert np.array_equal(gi, pairs)
    want = -cos[pairs[:, 1], pairs[:, 0]]
    assert _same(gm[:, 1], want), (gm[:, 1], want)
    assert not _same(cos, cos.T)   # the rounded cosine is not symmetric: the order of the arguments is part of the contract


@pytest.mark.parametrize("kind", ["mb32", "seq64"])
def test_skip_self(kind):
    rng = np.random.default_rng(35)
    k, K = 3, 10
    e, mi, s = _setup(kind, k, _eighths(rng, k))
    chain = _chain_exact_sums(_dt(kind))
    for metric in METRICS:
        full = e.neighbors(mi, mi, K + 1, metric=metric)
        skip = e.neighbors(mi, mi, K, metric=metric, skip_self=True)
        n_absent = 0
        for q in range(NI):
            keep = np.nonzero(full[0][q] != q)[0][:K]
            assert np.array_equal(skip[0][q], full[0][q][keep]) and _same(skip[1][q], full[1][q][keep]), (metric, q)
            n_absent += q not in full[0][q]
        assert 0 < n_absent < NI    # queries whose own row is not among the top_k + 1 best, and queries whose own row is
        # queries that are not the items: index r is removed from query row r and nothing else
        mq = _one_hot(QROWS)
        got = e.neighbors(mq, mi, K, metric=metric, skip_self=True)
        want = nm.neighbors(s[QROWS], s, K, metric, chain, skip_self=True)
        assert _eq(got, want)
        plain = e.neighbors(mq, mi, K + 1, metric=metric)
        for q in range(len(QROWS)):
            keep = np.nonzero(plain[0][q] != q)[0][:K]
            assert np.array_equal(got[0][q], plain[0][q][keep])


def test_refusals_leave_the_outputs_untouched():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(36)
    e, mi, s = _setup("mb32", 8, rng.normal(0, 0.4, (8, NI)))
    n, K = 5, 4
    mq = _one_hot(np.arange(n))
    oi, os_ = DevBuf.from_numpy(np.full(n * K, 7, np.int64)), DevBuf.from_numpy(np.full(n * K, 7.0))
    hi, hs = np.full((n, K), 7, np.int64), np.full((n, K), 7.0)
    lib = L.lib()
    other = engine.Engine(NI + 1, mode=L.MODE_MINIBATCH, num_factor=8)     # another feature count
    with pytest.raises(L.FmxError):   # (a factor count above fmx_topk's limit cannot be built: engines hold at most 128 factors, the limit is 256 floats / 128 doubles)
        engine.Engine(NI, mode=L.MODE_MINIBATCH, num_factor=129)
    empty = engine.Matrix.from_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), NI)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def dev(eng=e, q=mq, r0=0, r1=n, items=mi, top_k=K, metric=0, skip=0, out_i=oi.ptr, out_s=os_.ptr):
        return lib.fmx_neighbors_device(eng.h if eng is not None else None, q.h if q is not None else None, r0, r1, items.h if items is not None else None,
                                        top_k, metric, skip, out_i, out_s)

    def host(eng=e, q=mq, items=mi, top_k=K, metric=0, skip=0, out_i=p(hi), out_s=p(hs)):
        return lib.fmx_neighbors(eng.h if eng is not None else None, q.h if q is not None else None, items.h if items is not None else None, top_k, metric,
                                 skip, out_i, out_s)
    try:
        refused = [dev(eng=None), dev(q=None), dev(items=None), dev(out_i=None), dev(out_s=None), dev(eng=other), dev(top_k=0), dev(top_k=-1),
                   dev(top_k=1025), dev(metric=2), dev(metric=-1), dev(r0=-1), dev(r1=n + 1), dev(r0=3, r1=2)]
        assert all(st == L.ERR_INVALID for st in refused), refused
        assert lib.fmx_last_error().decode()
        refused = [host(eng=None), host(q=None), host(items=None), host(out_i=None), host(out_s=None), host(eng=other), host(top_k=0), host(top_k=1025),
                   host(metric=2), host(metric=-1)]
        assert all(st == L.ERR_INVALID for st in refused), refused
        n_dev = ctypes.c_int32()
        L.check(lib.fmx_device_count(ctypes.byref(n_dev)))
        if n_dev.value > 1:   # a matrix on another device than the engine's
            far = engine.Matrix.from_csr(np.arange(NI + 1, dtype=np.int64), np.arange(NI, dtype=np.uint32), np.ones(NI, np.float32), NI, device=1)
            assert dev(items=far) == L.ERR_INVALID and dev(q=far, r1=1) == L.ERR_INVALID
        # no query rows, an empty range: fine, and nothing is written (not even with NULL outputs)
        assert dev(r0=2, r1=2) == L.OK and dev(r0=2, r1=2, out_i=None, out_s=None) == L.OK and dev(q=empty, r1=0) == L.OK
        assert host(q=empty) == L.OK and host(q=empty, out_i=None, out_s=None) == L.OK
        e.sync()
        assert np.all(oi.numpy() == 7) and np.all(os_.numpy() == 7.0) and np.all(hi == 7) and np.all(hs == 7.0)
        # no items: every slot is padding
        assert dev(items=empty) == L.OK and host(items=empty, skip=1) == L.OK
        e.sync()
        assert np.all(oi.numpy() == -1) and np.all(np.isnan(os_.numpy())) and np.all(hi == -1) and np.all(np.isnan(hs))
        # and the same buffers take a real call afterwards
        want = e.neighbors(mq, mi, K)
        assert dev() == L.OK and host() == L.OK
        e.sync()
        assert _eq((oi.numpy().reshape(n, K), os_.numpy().reshape(n, K)), want) and _eq((hi, hs), want)
    finally:
        oi.free(); os_.free()


def _fit(rng, p, k):
    import fmwr_amd as fm
    ctl = {"model": fm.model_control("REGRESSION", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    return {"Model": {"w0": 0.25, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"],
                      "solver.control": ctl["solver"], "track.control": ctl["track"]},
            "Scales": {"mean": None, "std": None, "target.range": (-1e300, 1e300)}}


def test_fm_similar():
    import fmwr_amd as fm
    rng = np.random.default_rng(37)
    p, nq, ni, k = 60, 7, 150, 4
    fit = _fit(rng, p, k)
    itm = fm.fm_matrix(sp.random(ni, p, 0.1, random_state=2, format="csr") + sp.eye(ni, p, k=3, format="csr"))
    qry = fm.fm_matrix(sp.random(nq, p, 0.2, random_state=1, format="csr") + sp.eye(nq, p, format="csr"))
    emb_i, emb_q = fm.fm_embed(fit, itm, normalize=False)["s"], fm.fm_embed(fit, qry, normalize=False)["s"]
    chain = dm.chain_exact(np.float64)
    got = fm.fm_similar(fit, itm, normalize=False)                          # the items against themselves
    assert set(got) == {"index", "score"} and got["index"].shape == got["score"].shape == (ni, 10)
    assert not (got["index"] == np.arange(ni)[:, None]).any() and np.all(got["index"] >= 0)
    assert _eq((got["index"][:12], got["score"][:12]), nm.neighbors(emb_i[:12], emb_i, 10, nm.SIM_COSINE, chain, skip_self=True))
    for metric, code in (("cosine", nm.SIM_COSINE), ("dot", nm.SIM_DOT)):
        got = fm.fm_similar(fit, itm, queries=qry, top_k=5, metric=metric, normalize=False)
        assert got["index"].shape == got["score"].shape == (nq, 5)
        assert _eq((got["index"], got["score"]), nm.neighbors(emb_q, emb_i, 5, code, chain))
    for kw in ({"metric": "euclid"}, {"metric": 0}, {"top_k": 0}, {"top_k": 2000}, {"top_k": 2.5}):
        with pytest.raises(ValueError):
            fm.fm_similar(fit, itm, normalize=False, **kw)
