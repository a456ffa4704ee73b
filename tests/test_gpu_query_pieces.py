"""The host forms of the query entry points stage their results on the device in pieces (2^22 result slots, 2^16 rows for fmx_project, 2^22
entries for fmx_rank_lists) and copy each piece down.  Every case here sends a host form through two pieces with a partial last one and
compares every output array, bit for bit (the doubles as int64, NaN slots included), with the same entry point's _device form called once
over the whole range: that path does not go through the staging.  The one-piece host forms are held to their _device forms the same way.

The device buffers are tests/util.py's DevBuf (the HIP runtime libfmx.so is linked against), as in the other GPU tests: importing torch after
libfmx.so would bring a second HIP runtime into the process."""
import ctypes as C

import numpy as np
import pytest

from tests.util import DevBuf

pytestmark = pytest.mark.gpu

P, K_FACT, NI = 64, 3, 1100
TOP_K = 1024                      # a piece of the top-K forms: 2^22 / 1024 = 4 096 rows
N_CTX = 4097
TOP_M = 64                        # a piece of fmx_interactions: 2^22 / 64 = 65 536 rows, as many as fmx_project's
N_ROWS = 65537


def _engine(k):
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(P, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=256)
    rng = np.random.default_rng(5 + k)
    e.set_params(0.3, rng.normal(0, 0.5, P), rng.normal(0, 0.4, (k, P)))
    return e


def _rows(n, bands, rng):
    """n rows of one entry per band of columns [lo, hi), random values"""
    col = np.stack([rng.integers(lo, hi, n) for lo, hi in bands], axis=1).astype(np.uint32)
    rp = np.arange(n + 1, dtype=np.int64) * len(bands)
    return rp, col.ravel(), rng.normal(0, 1, col.size).astype(np.float32)


def _mat(m, p=P):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _head(m, n):
    return m[0][:n + 1], m[1][:m[0][n]], m[2][:m[0][n]]


def _lists(n, per, rng):
    """n lists of `per` distinct items each, unsorted"""
    col = np.argsort(rng.random((n, NI)), axis=1)[:, :per].astype(np.uint32)
    rp = np.arange(n + 1, dtype=np.int64) * per
    return _mat((rp, col.ravel(), np.ones(col.size, np.float32)), NI)


class _World:
    def __init__(self):
        rng = np.random.default_rng(2024)
        self.e = _engine(K_FACT)
        self.items = _mat(_rows(NI, [(32, 48), (48, 64)], rng))
        self.ctx_csr = _rows(N_CTX, [(0, 16), (16, 32)], rng)
        self.ctx = _mat(self.ctx_csr)
        self.rows3 = _mat(_rows(N_ROWS, [(0, 20), (20, 40), (40, 64)], rng))
        self.rng = rng


@pytest.fixture(scope="module")
def w():
    return _World()


def _dev(e, call, shapes):
    """call(ptr, ...) on fresh device buffers of the given (count, dtype) -- None for a NULL output -- and their contents"""
    bufs = [None if s is None else DevBuf(s[0], s[1]) for s in shapes]
    try:
        call(*[None if b is None else b.ptr.value for b in bufs])
        e.sync()
        return [None if b is None else b.numpy() for b in bufs]
    finally:
        for b in bufs:
            if b is not None:
                b.free()


def _bits(a):
    a = np.ascontiguousarray(a).ravel()
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, ref, what):
    assert len(got) == len(ref)
    for t, (g, r) in enumerate(zip(got, ref)):
        assert g.size == r.size and g.dtype == r.dtype, (what, t)
        assert np.array_equal(_bits(g), _bits(r)), (what, t)


@pytest.mark.parametrize("n", [N_CTX, N_CTX - 1])
def test_topk_second_piece_of_one_row_and_exactly_one_piece(w, n):
    e, mc = w.e, (w.ctx if n == N_CTX else _mat(_head(w.ctx_csr, n)))
    ref = _dev(e, lambda di, ds: e.topk_device(mc, 0, n, w.items, TOP_K, di, ds), [(n * TOP_K, np.int64), (n * TOP_K, np.float64)])
    assert ref[0].min() >= 0 and not np.isnan(ref[1]).any()     # 1 100 items: every slot is filled
    _same(e.topk(mc, w.items, TOP_K), ref, n)


def test_neighbors_second_piece_of_one_row(w):
    from fmwr_amd import _lib as L
    e, n = w.e, N_CTX
    ref = _dev(e, lambda di, ds: e.neighbors_device(w.ctx, 0, n, w.items, TOP_K, di, ds, metric=L.SIM_COSINE, skip_self=False),
               [(n * TOP_K, np.int64), (n * TOP_K, np.float64)])
    _same(e.neighbors(w.ctx, w.items, TOP_K, metric=L.SIM_COSINE, skip_self=False), ref, "neighbors")


def test_topk_lists_second_piece_and_the_empty_tails(w):
    e, n = w.e, N_CTX
    ml = _lists(n, 8, w.rng)
    ref = _dev(e, lambda di, ds: e.topk_lists_device(w.ctx, 0, n, w.items, ml, TOP_K, di, ds), [(n * TOP_K, np.int64), (n * TOP_K, np.float64)])
    ri, rs = ref[0].reshape(n, TOP_K), ref[1].reshape(n, TOP_K)
    assert (ri[:, :8] >= 0).all() and (ri[:, 8:] == -1).all() and np.isnan(rs[:, 8:]).all() and not np.isnan(rs[:, :8]).any()
    _same(e.topk_lists(w.ctx, w.items, ml, TOP_K), ref, "topk_lists")


def test_interactions_second_piece_and_the_fill(w):
    e, n = w.e, N_ROWS
    ref = _dev(e, lambda da, db, dv: e.interactions_device(w.rows3, 0, n, TOP_M, da, db, dv),
               [(n * TOP_M, np.int64), (n * TOP_M, np.int64), (n * TOP_M, np.float64)])
    a, b, v = (r.reshape(n, TOP_M) for r in ref)
    assert (a[:, :3] >= 0).all() and (a[:, 3:] == -1).all() and (b[:, 3:] == -1).all() and np.isnan(v[:, 3:]).all()   # 3 pairs, 61 slots of fill
    _same(e.interactions(w.rows3, TOP_M), ref, "interactions")


@pytest.mark.parametrize("with_w0", [False, True])
@pytest.mark.parametrize("k", [K_FACT, 0])
def test_project_second_piece_both_widths(w, k, with_w0):
    e, n = (w.e if k else _engine(0)), N_ROWS
    ref = _dev(e, lambda db, ds: e.project_device(w.rows3, 0, n, db, ds, with_w0=with_w0), [(n, np.float64), (n * k, np.float64) if k else None])
    base, s = e.project(w.rows3, with_w0=with_w0)      # k = 0: out_s is NULL
    assert s.shape == (n, k)
    _same([base] + ([s] if k else []), ref[:1 + (k > 0)], ("project", k, with_w0))


def test_rank_lists_two_pieces_cut_by_entries(w):
    """4 100 lists of 1 024 candidates are 4 198 400 entries: the first 4 096 lists fill the budget of 2^22 entries exactly, the last 4 are the
    second piece.  A single list longer than 2^22 entries (a piece of its own) is not reached: it would need a list of over 4 M candidates."""
    e, n, per = w.e, 4100, 1024
    rng = np.random.default_rng(9)
    mc = _mat(_rows(n, [(0, 16), (16, 32)], rng))
    ml = _lists(n, per, rng)
    assert ml.nnz == n * per > 1 << 22
    ref = _dev(e, lambda ds, dp: e.rank_lists_device(mc, 0, n, w.items, ml, ds, dp), [(n * per, np.float64), (n * per, np.int64)])
    assert np.array_equal(np.sort(ref[1].reshape(n, per), axis=1), np.tile(np.arange(per), (n, 1)))   # distinct candidates: every position once
    _same(e.rank_lists(mc, w.items, ml), ref, "rank_lists")
    score, none = e.rank_lists(mc, w.items, ml, positions=False)     # out_pos = NULL
    assert none is None
    _same([score], ref[:1], "rank_lists without positions")


def test_one_piece_forms_equal_their_device_forms(w):
    from fmwr_amd import _lib as L
    e, n = w.e, 1000
    m = _mat(_head(w.ctx_csr, n))
    ref = _dev(e, lambda d: L.check(L.lib().fmx_predict_device(e.h, m.h, C.c_int64(0), C.c_int64(n), C.c_void_p(d), C.c_int(L.LINK_NONE))), [(n, np.float64)])
    _same([e.predict(m)], ref, "predict")
    ref = _dev(e, lambda d: e.contrib_device(m, 0, n, d), [(m.nnz, np.float64)])
    _same([e.contrib(m)], ref, "contrib")
    mh = _lists(n, 2, w.rng)                                         # two held-out items per context
    ref = _dev(e, lambda dr, ds: e.heldout_rank_device(m, 0, n, w.items, mh, dr, ds), [(mh.nnz, np.int64), (mh.nnz, np.float64)])
    _same(e.heldout_rank(m, w.items, mh), ref, "heldout_rank")
    ref = _dev(e, lambda dr: e.heldout_rank_device(m, 0, n, w.items, mh, dr, None), [(mh.nnz, np.int64)])
    rank = np.zeros(mh.nnz, np.int64)                                # out_score = NULL
    L.check(L.lib().fmx_heldout_rank(e.h, m.h, w.items.h, mh.h, None, rank.ctypes.data_as(C.c_void_p), None))
    _same([rank], ref, "heldout_rank without scores")
