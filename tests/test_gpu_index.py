"""fmx_index_build / fmx_index_from_assign / fmx_topk_index held to tests/index_model.py.  Every comparison is exact
equality (the sign of a zero canonicalised: the zero-padded chain can turn -0 into +0; a NaN equals any NaN) except the one-step check of the
centroid update, whose bar is cnt * 2^-53 * sum |term| around the math.fsum mean; the largest share of that bar seen is printed.

Items are one-hot rows (item i = feature i) and so are the contexts (context c = feature NI + c): s is a column of V and the base the linear
weight, read back through fmx_project.  Where the Fraction emulation of the score chain is too slow the factors are eighths: every partial sum
of a chain is then exact in fp32.  The two fp64 chains of the index itself run through the model's exact fma whatever the values.  Both forms
of the fine stage are forced through fmx_debug_index_limits beside the rule's choice."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

from tests import index_model as im
from tests.test_gpu_topk import _engine
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

NI, NC = 1800, 40
P = NI + NC
SIZES = [0, 1, 255, 256, 257, 1025, 6]         # the list sizes of the hand-made index: every workgroup edge, and an empty list
CTX = [0, 1, 2, 3, 5, 8, 13, 21, 34]           # nine contexts


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    a = np.where(np.isnan(a), im.QNAN, np.where(a == 0, 0.0, a))
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eq(got, want):
    """(index, score[, scanned]) against the model's"""
    return np.array_equal(got[0], want[0]) and _same(got[1], want[1]) and (len(got) < 3 or len(want) < 3 or np.array_equal(got[2], want[2]))


def _dt(kind):
    return np.float32 if kind in ("mb32", "mb32w") else np.float64


def _chain(dt):
    """the chain of rows whose partial sums are exact in dt: the float64 dot product narrowed to dt"""
    if dt == np.float64:
        return im.chain_dot

    def chain(rows, v):
        with np.errstate(all="ignore"):
            return np.asarray(im.chain_dot(rows, v), np.float64).astype(np.float32).astype(np.float64)
    return chain


def _one_hot(ids, p=P):
    from fmwr_amd import engine
    ids = np.asarray(ids, np.uint32)
    return engine.Matrix.from_csr(np.arange(len(ids) + 1, dtype=np.int64), ids, np.ones(len(ids), np.float32), p)


def _excl(rows, ni):
    from fmwr_amd import engine
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate(rows).astype(np.uint32) if len(rows) else np.zeros(0, np.uint32)
    return engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), ni)


class Case:
    """an engine over P features holding (w0, w, v), the items 0 .. ni-1 and the contexts, with their projections"""
    def __init__(self, kind, k, v, w=None, ni=NI, ctx=CTX, monkeypatch=None, seed=0):
        if kind == "mb32w":
            monkeypatch.setenv("FMX_W_IN_ROW", "1")
        self.e = _engine("mb32" if kind == "mb32w" else kind, P, k)
        if kind == "mb32w":
            assert self.e.w_in_row()
        rng = np.random.default_rng(seed)
        self.w = rng.integers(-8, 9, P) / 8.0 if w is None else w
        self.e.set_params(0.25, self.w, v)
        self.dt, self.k, self.ni = _dt(kind), k, ni
        self.mi = _one_hot(np.arange(ni))
        self.bi, self.si = self.e.project(self.mi)
        self.set_ctx(ctx)

    def set_ctx(self, ctx):
        self.ctx = list(ctx)
        self.mc = _one_hot(NI + np.asarray(ctx))
        self.bc, self.sc = self.e.project(self.mc, with_w0=True)

    def index(self, assign, cen):
        ix = self.e.index_from_assign(assign, cen)
        ptr, item = im.lists(assign, len(cen))
        assert np.array_equal(ix.list_ptr, ptr) and np.array_equal(ix.list_item, item) and ix.non_empty == int(np.sum(np.diff(ptr) > 0))
        assert np.array_equal(ix.assign, assign) and np.array_equal(ix.centroids.view(np.uint64), np.asarray(cen, np.float64).view(np.uint64))
        assert (ix.n_items, ix.n_lists, ix.k) == (len(assign), len(cen), self.k)
        return ix, ptr, item

    def scores(self, chain):
        return im.pair_scores(self.sc, self.bc, self.si, self.bi, chain)


def _eighths(rng, k, p=P):
    return rng.integers(-8, 9, (k, p)) / 8.0


def _sized_assign(rng, sizes, n):
    asg = np.repeat(np.arange(len(sizes)), sizes).astype(np.uint32)
    assert len(asg) == n
    return asg[rng.permutation(n)]


class _Limits:
    """fmx_debug_index_limits for a with-block (sticky: restored on exit)"""
    def __init__(self, fine_form=0, chunk_rows=0, slice_lists=0):
        self.args = (fine_form, chunk_rows, slice_lists)

    def __enter__(self):
        from fmwr_amd import _lib as L
        L.check(L.lib().fmx_debug_index_limits(*self.args))

    def __exit__(self, *exc):
        from fmwr_amd import _lib as L
        L.check(L.lib().fmx_debug_index_limits(0, 0, 0))


def _all_forms(c, ix, K, n_probe, want, exclude=None):
    """the host call under the rule and with each fine form forced: all equal to `want`"""
    for form in (0, 1, 2):
        with _Limits(form, 0, 0):
            got = c.e.topk_index(ix, c.mc, c.mi, K, n_probe, exclude=exclude)
        if not _eq(got, want):
            return False
    return True


def _device(c, ix, r0, r1, K, n_probe, exclude=None, scanned=True):
    n = r1 - r0
    oi, os_, on = DevBuf(n * K, np.int64), DevBuf(n * K), DevBuf(n, np.int64)
    try:
        c.e.topk_index_device(ix, c.mc, r0, r1, c.mi, K, n_probe, oi.ptr.value, os_.ptr.value, on.ptr.value if scanned else None, exclude=exclude)
        c.e.sync()
        return oi.numpy().reshape(n, K), os_.numpy().reshape(n, K), on.numpy().reshape(n)
    finally:
        oi.free(); os_.free(); on.free()


KINDS = [(kind, k) for kind in ("seq64", "mb64", "mb32") for k in (0, 1, 3, 16, 17, 64, 100)] + [("mb32w", k) for k in (1, 3, 16)]


@pytest.mark.parametrize("kind,k", KINDS)
def test_engine_kinds_and_factors_equal_the_model_bit_for_bit(kind, k, monkeypatch):
    """lists of 0, 1, 255, 256, 257, 1 025 and 6 items in one index; n_probe 1, 2, n_lists - 1, n_lists; with and without exclusions; every list
    probed equals fmx_topk in every bit; then random factors against the Fraction chain"""
    rng = np.random.default_rng(4000 + k)
    c = Case(kind, k, _eighths(rng, k), monkeypatch=monkeypatch)
    assert np.array_equal(c.si, c.e.get_params()[2].T[:NI])
    asg = _sized_assign(rng, SIZES, NI)
    cen = rng.integers(-8, 9, (len(SIZES), k + 1)) / 8.0
    ix, ptr, item = c.index(asg, cen)
    score, g = c.scores(_chain(c.dt)), im.coarse(c.sc, cen)
    K = 10
    excl = [rng.choice(NI, 30, replace=False) for _ in CTX]
    excl[0] = item[ptr[5]:ptr[6]]                                   # empties the list of 1 025
    excl[1] = np.setdiff1d(np.arange(NI), item[ptr[2]:ptr[2] + 4])  # more excluded items than remain: four are left
    mx = _excl(excl, NI)
    top = c.e.topk(c.mc, c.mi, K)
    top_x = c.e.topk(c.mc, c.mi, K, exclude=mx)
    for n_probe in (1, 2, len(SIZES) - 1, len(SIZES)):
        want = im.search_scores(score, g, ptr, item, K, n_probe)
        got = c.e.topk_index(ix, c.mc, c.mi, K, n_probe)
        assert _eq(got, want), (n_probe, got, want)
        want_x = im.search_scores(score, g, ptr, item, K, n_probe, excl)
        got_x = c.e.topk_index(ix, c.mc, c.mi, K, n_probe, exclude=mx)
        assert _eq(got_x, want_x), (n_probe, got_x, want_x)
        assert _all_forms(c, ix, K, n_probe, want) and _all_forms(c, ix, K, n_probe, want_x, exclude=mx), n_probe
        if n_probe >= len(SIZES) - 1:                                # one list is empty: n_lists - 1 probes are every non-empty list
            assert _eq(got[:2], top) and _eq(got_x[:2], top_x) and np.all(got[2] == NI)
            assert np.sum(got_x[0][1] >= 0) == 4
    if k == 0:
        return
    nb, nq = 24, 2
    v = rng.normal(0, 0.4, (k, P))
    c = Case(kind, k, v, w=rng.normal(0, 0.5, P), ni=nb, ctx=CTX[:nq], monkeypatch=monkeypatch)
    asg = rng.integers(0, 3, nb).astype(np.uint32)
    cen = rng.normal(0, 0.5, (3, k + 1))
    ix, ptr, item = c.index(asg, cen)
    for n_probe in (1, 2, 3):
        want = im.search(c.sc, c.bc, c.si, c.bi, cen, ptr, item, nb, n_probe, im.chain_exact(c.dt))
        assert _all_forms(c, ix, nb, n_probe, want), n_probe


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_list_counts_context_counts_and_top_k_on_the_edges(kind):
    """n_lists 1, 2, 7, 64, 257 x contexts 1, 7, 8, 9, 33 (tiles of 8 in the coarse kernel); top_k on the three buffer sizes"""
    rng = np.random.default_rng(51)
    k = 3
    c = Case(kind, k, _eighths(rng, k), ni=600, ctx=np.arange(33))
    score_all = c.scores(_chain(c.dt))
    for n_lists in (1, 2, 7, 64, 257):
        asg = rng.integers(0, n_lists, 600).astype(np.uint32)
        cen = rng.integers(-8, 9, (n_lists, k + 1)) / 8.0
        ix, ptr, item = c.index(asg, cen)
        g_all = im.coarse(c.sc, cen)
        for nc in (1, 7, 8, 9, 33):
            c.set_ctx(np.arange(nc))
            for n_probe in sorted({1, min(2, n_lists), max(n_lists - 1, 1), n_lists}):
                want = im.search_scores(score_all[:nc], g_all[:nc], ptr, item, 10, n_probe)
                assert _all_forms(c, ix, 10, n_probe, want), (n_lists, nc, n_probe)
    c.set_ctx(np.arange(3))
    asg = _sized_assign(rng, [300, 290, 10], 600)
    cen = rng.integers(-8, 9, (3, k + 1)) / 8.0
    ix, ptr, item = c.index(asg, cen)
    g = im.coarse(c.sc, cen)
    for K in (1, 10, 256, 257, 768, 1024):
        for n_probe in (1, 2, 3):
            want = im.search_scores(score_all[:3], g, ptr, item, K, n_probe)
            assert _all_forms(c, ix, K, n_probe, want), (K, n_probe)
        assert _eq(c.e.topk_index(ix, c.mc, c.mi, K, 3)[:2], c.e.topk(c.mc, c.mi, K)), K


def test_more_probes_than_the_selection_holds():
    """1 300 lists, n_probe = 1 100 < non_empty: the coarse stage beyond the LDS selection's 1 024 slots (the segmented sort), in chunks of 2 too"""
    rng = np.random.default_rng(52)
    k = 3
    c = Case("mb32", k, _eighths(rng, k), ni=1500, ctx=np.arange(5))
    asg = np.concatenate([np.arange(1250), rng.integers(0, 1250, 250)]).astype(np.uint32)   # lists 1250 .. 1299 stay empty
    cen = rng.integers(-8, 9, (1300, k + 1)) / 8.0
    cen[7] = cen[3]
    ix, ptr, item = c.index(asg, cen)
    assert ix.non_empty == 1250
    score, g = c.scores(_chain(c.dt)), im.coarse(c.sc, cen)
    for n_probe in (1024, 1025, 1100, 1249):
        want = im.search_scores(score, g, ptr, item, 10, n_probe)
        assert _all_forms(c, ix, 10, n_probe, want), n_probe
        for form in (1, 2):
            with _Limits(form, 2, 0):
                assert _eq(c.e.topk_index(ix, c.mc, c.mi, 10, n_probe), want), (form, n_probe)
    assert _eq(c.e.topk_index(ix, c.mc, c.mi, 10, 1300)[:2], c.e.topk(c.mc, c.mi, 10))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_nan_inf_and_ties(kind):
    """NaN and infinite centroids and projections, tied g and tied scores"""
    rng = np.random.default_rng(53)
    k = 3
    v = _eighths(rng, k)
    v[:, 9] = v[:, 8]                      # twins: tied scores, the lower index first
    v[0, 20] = np.nan                      # a NaN score: below every number, still listed
    v[1, 21] = np.inf
    w = rng.integers(-8, 9, P) / 8.0
    w[9] = w[8]
    w[22] = -np.inf
    v[:, NI + 3] = 0.0                     # a context with no factors: every g is the centroid's last component
    c = Case(kind, k, v, w=w, ni=400, ctx=np.arange(9))
    asg = rng.integers(0, 9, 400).astype(np.uint32)
    asg[[8, 9]] = [2, 5]
    cen = rng.integers(-8, 9, (9, k + 1)) / 8.0
    cen[4] = cen[1]                        # tied g for every context: list 1 first
    cen[6, 0] = np.nan                     # NaN g: probed last
    cen[7, k] = np.inf                     # always first
    cen[8, k] = -np.inf
    cen[[0, 2], k] = 0.5                   # tied g for context 3
    ix, ptr, item = c.index(asg, cen)
    with np.errstate(all="ignore"):
        score, g = c.scores(_chain(c.dt)), im.coarse(c.sc, cen)
    assert np.all(np.isnan(score[:, 20])) and np.all(np.isnan(g[:, 6])) and np.all(g[:, 7] == np.inf) and g[3, 0] == g[3, 2]
    for n_probe in range(1, 10):
        for K in (5, 400):
            want = im.search_scores(score, g, ptr, item, K, n_probe)
            assert _all_forms(c, ix, K, n_probe, want), (n_probe, K)
    assert _eq(c.e.topk_index(ix, c.mc, c.mi, 400, 9)[:2], c.e.topk(c.mc, c.mi, 400))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_adverse_order_flushes_every_round(kind):
    """inside a list the score rises with the item index: every item beats the running threshold and the buffer is sorted after every round"""
    k = 2
    v = np.zeros((k, P))
    v[0, :NI], v[1, :NI] = np.arange(NI), 1.0
    v[:, NI] = [1.0, 0.0]
    c = Case(kind, k, v, w=np.zeros(P), ctx=[0])
    asg = (np.arange(NI) % 2).astype(np.uint32)
    cen = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]])
    ix, ptr, item = c.index(asg, cen)
    score, g = c.scores(_chain(c.dt)), im.coarse(c.sc, cen)          # integers below 2^24: every partial sum is exact
    assert np.all(np.diff(score[0]) > 0)
    for K in (5, 300, 800):
        for n_probe in (1, 2):
            want = im.search_scores(score, g, ptr, item, K, n_probe)
            assert want[0][0, 0] == NI - 1 and _all_forms(c, ix, K, n_probe, want), (K, n_probe)


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_invariance_over_forms_chunks_entry_points_ranges_batches_and_calls(kind):
    rng = np.random.default_rng(54)
    k, K, n_lists = 16, 12, 7
    c = Case(kind, k, rng.normal(0, 0.4, (k, P)), w=rng.normal(0, 0.5, P), ni=600, ctx=np.arange(33))
    before = c.e.get_params()
    asg = rng.integers(0, n_lists, 600).astype(np.uint32)
    ix, ptr, item = c.index(asg, rng.normal(0, 0.5, (n_lists, k + 1)))
    excl = [rng.choice(600, 40, replace=False) for _ in range(33)]
    mx = _excl(excl, 600)
    refs = {}
    for n_probe in (1, 3, 7):
        for x in (None, mx):
            ref = c.e.topk_index(ix, c.mc, c.mi, K, n_probe, exclude=x)
            refs[n_probe, x is None] = ref
            assert _eq(c.e.topk_index(ix, c.mc, c.mi, K, n_probe, exclude=x), ref)                       # a second call
            for form, chunk in ((1, 0), (2, 0), (0, 16), (1, 16), (2, 16), (2, 1), (1, 1)):                # each form, chunks of contexts
                with _Limits(form, chunk, 0):
                    assert _eq(c.e.topk_index(ix, c.mc, c.mi, K, n_probe, exclude=x), ref), (form, chunk)
                    assert _eq(_device(c, ix, 0, 33, K, n_probe, exclude=x), ref), (form, chunk)       # the device form
                    assert _eq(_device(c, ix, 5, 30, K, n_probe, exclude=x), [r[5:30] for r in ref])   # a row range
            assert _eq(_device(c, ix, 5, 30, K, n_probe, exclude=x, scanned=False)[:2], [r[5:30] for r in ref[:2]])
    ref = refs[3, True]
    perm = rng.permutation(33)                                                                             # a permuted batch, one row alone
    c.set_ctx(perm)
    assert _eq(c.e.topk_index(ix, c.mc, c.mi, K, 3), [r[perm] for r in ref])
    c.set_ctx([17])
    assert _eq(c.e.topk_index(ix, c.mc, c.mi, K, 3), [r[17:18] for r in ref])
    c.set_ctx(np.arange(33))
    for K1 in (1, 5):                                                                                      # prefix
        assert _eq(c.e.topk_index(ix, c.mc, c.mi, K1, 3)[:2], [r[:, :K1] for r in ref[:2]])
    runs = [c.e.topk_index(ix, c.mc, c.mi, K, q) for q in range(1, n_lists + 1)]                           # slot-wise nesting
    for lo, hi in zip(runs, runs[1:]):
        assert np.all(hi[2] >= lo[2])
        both = lo[0] >= 0
        assert np.all(hi[0][both] >= 0)
        worse = (hi[1] < lo[1]) | ((hi[1] == lo[1]) & (hi[0] > lo[0]))
        assert not np.any(worse & both)
    assert _eq(runs[-1][:2], c.e.topk(c.mc, c.mi, K))
    after = c.e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_a_two_replica_engine_reads_its_primary():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(55)
    k = 8
    v, w = rng.normal(0, 0.4, (k, P)), rng.normal(0, 0.5, P)
    g = engine.Engine(P, num_factor=k, mode=L.MODE_MINIBATCH, batch_rows=256, n_gpus=2, gpus_share_device=1)
    g.set_params(0.25, w, v)
    c = Case("mb32", k, v, w=w, ni=300, ctx=np.arange(9))
    ix1 = c.e.index_build(c.mi, 7, n_iter=2, seed=3)
    ix2 = g.index_build(c.mi, 7, n_iter=2, seed=3)
    for a, b in zip(ix1.export(), ix2.export()):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    assert _eq(g.topk_index(ix2, c.mc, c.mi, 10, 2), c.e.topk_index(ix1, c.mc, c.mi, 10, 2))
    w0, gw, gv = g.get_params()
    assert w0 == 0.25 and np.array_equal(gw, c.e.get_params()[1]) and np.array_equal(gv, c.e.get_params()[2])


# ---------------------------------------------------------------------------------------------------------------- the build

BUILD_SHAPES = [(1, 1), (255, 2), (256, 7), (257, 64), (1025, 257), (5000, 64), (5000, 7), (5000, 1)]
_share = {"max": 0.0}


class BuildCase(Case):
    """items 0 .. ni-1 over ni + NC features (the build cases go beyond NI items)"""
    def __init__(self, kind, k, ni, v, w):
        self.e = _engine(kind, ni + NC, k)
        self.e.set_params(0.25, w, v)
        self.dt, self.k, self.ni = _dt(kind), k, ni
        self.mi = _one_hot(np.arange(ni), ni + NC)
        self.bi, self.si = self.e.project(self.mi)
        self.a = im.augment(self.si, self.bi)


@pytest.mark.parametrize("ni,n_lists", BUILD_SHAPES)
@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_the_build_step_by_step(kind, ni, n_lists):
    """n_iter = 0: the seeds; for t in 0, 1, 3: the assign of build(t) is the model's arg-min against build(t)'s centroids, and the centroids of
    build(t + 1) are one update step from build(t)'s lists -- within the bar of the fsum mean, and the model's ordered sum in every bit"""
    rng = np.random.default_rng(600 + ni + n_lists)
    k = 3
    v, w = rng.normal(0, 0.5, (k, ni + NC)), rng.normal(0, 0.5, ni + NC)
    dup = ni >= 255
    if dup:
        v[:, 5], w[5] = v[:, 4], w[4]          # duplicate items
        v[0, 11] = np.nan                      # non-finite items
        w[12] = np.inf
    c = BuildCase(kind, k, ni, v, w)
    a = c.a
    seed = 9
    builds = {}
    for slice_lists in (4, 0):
        with _Limits(0, 0, slice_lists):
            for t in (0, 1, 2, 3, 4):
                cen, asg, ptr, item = c.e.index_build(c.mi, n_lists, n_iter=t, seed=seed).export()
                if slice_lists == 4:
                    builds[t] = (cen, asg, ptr, item)
                else:                                                                       # the slicing changes no bit
                    assert all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
                               for x, y in zip(builds[t], (cen, asg, ptr, item))), t
    order = im.seed_order(a, seed)
    assert np.array_equal(builds[0][0].view(np.uint64), a[order[:n_lists]].view(np.uint64))
    for t in (0, 1, 3):
        cen, asg, ptr, item = builds[t]
        assert np.array_equal(asg, im.assign(a, cen)), t
        lp, li = im.lists(asg, n_lists)
        assert np.array_equal(ptr, lp) and np.array_equal(item, li)
        if dup:
            assert asg[11] == 0 and asg[12] == 0
        nxt = builds[t + 1][0]
        mean, bar, live = im.update_bars(a, cen, ptr, item)
        assert np.array_equal(nxt[~live].view(np.uint64), cen[~live].view(np.uint64))      # no finite member: the previous bits
        err = np.abs(nxt[live] - mean[live])
        assert np.all(err <= bar[live]), (t, float(np.max(err / np.maximum(bar[live], 1e-300))))
        if live.any():
            _share["max"] = max(_share["max"], float(np.max(err / np.maximum(bar[live], 1e-300))))
        assert np.array_equal(nxt.view(np.uint64), im.update(a, cen, ptr, item).view(np.uint64)), t
    print(f"largest share of the update bar so far: {_share['max']:.4f}")


def test_duplicates_non_finite_items_repeatability_and_reload():
    rng = np.random.default_rng(61)
    k, ni = 3, 300
    v, w = _eighths(rng, k, ni + NC), rng.integers(-8, 9, ni + NC) / 8.0
    v[:, :ni] = v[:, [0]]                      # every item the same vector: every seed is the same centroid, the higher lists stay empty
    w[:ni] = w[0]
    v[1, 7] = np.nan
    c = BuildCase("mb32", k, ni, v, w)
    ix = c.e.index_build(c.mi, 5, n_iter=2, seed=1)
    cen, asg, ptr, item = ix.export()
    assert np.all(asg == 0) and ix.non_empty == 1 and list(ptr) == [0, ni, ni, ni, ni, ni]
    assert np.array_equal(cen.view(np.uint64), np.tile(c.a[0], (5, 1)).view(np.uint64))     # the mean of equal eighths is exact; empty lists keep the seed
    # non-finite items: in list 0, out of the sums, and not counted as seeds
    v, w = rng.normal(0, 0.5, (k, ni + NC)), rng.normal(0, 0.5, ni + NC)
    bad = np.arange(0, ni, 3)
    v[0, bad] = np.nan
    c = BuildCase("seq64", k, ni, v, w)
    n_fin = ni - len(bad)
    from fmwr_amd import _lib as L
    with pytest.raises(L.FmxError):
        c.e.index_build(c.mi, n_fin + 1, n_iter=0)                                          # fewer finite items than lists
    ix = c.e.index_build(c.mi, n_fin, n_iter=0, seed=4)                                     # exactly as many: every finite item a seed
    assert sorted(map(tuple, ix.centroids)) == sorted(map(tuple, c.a[im.finite_items(c.a)]))
    ix = c.e.index_build(c.mi, 6, n_iter=3, seed=4)
    want = im.build(c.a, 6, 3, 4)
    for got, w_ in zip(ix.export(), want):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(w_).view(np.uint8))
    assert np.all(ix.assign[bad] == 0) and np.all(np.isfinite(ix.centroids))
    again = c.e.index_build(c.mi, 6, n_iter=3, seed=4)                                      # a second call: the same bits
    for x, y in zip(ix.export(), again.export()):
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
    other = c.e.index_build(c.mi, 6, n_iter=3, seed=5)
    assert not np.array_equal(other.assign, ix.assign)
    # export -> from_assign -> search: equal outputs
    c.mc = _one_hot(ni + np.arange(9), ni + NC)
    re = c.e.index_from_assign(ix.assign, ix.centroids)
    for n_probe in (1, 3, 6):
        assert _eq(c.e.topk_index(re, c.mc, c.mi, 10, n_probe), c.e.topk_index(ix, c.mc, c.mi, 10, n_probe))
    del again, other, re
    ix.close(); ix.close()                                                                   # freed once


def test_refusals_leave_the_outputs_untouched():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(62)
    k = 8
    c = Case("mb32", k, rng.normal(0, 0.4, (k, P)), ni=200, ctx=np.arange(5))
    n, K = 5, 4
    ix = c.e.index_build(c.mi, 6, n_iter=1)
    lib = L.lib()
    other_p = engine.Engine(P + 1, mode=L.MODE_MINIBATCH, num_factor=k)      # another feature count
    other_k = engine.Engine(P, mode=L.MODE_MINIBATCH, num_factor=k + 1)      # another factor count than the index's
    fewer = _one_hot(np.arange(199))                                         # not the indexed items
    empty = engine.Matrix.from_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), P)
    bad_x = _excl([np.zeros(0, np.int64)] * 4, 200)
    oi, os_, on = DevBuf.from_numpy(np.full(n * K, 7, np.int64)), DevBuf.from_numpy(np.full(n * K, 7.0)), DevBuf.from_numpy(np.full(n, 7, np.int64))
    hi, hs, hn = np.full((n, K), 7, np.int64), np.full((n, K), 7.0), np.full(n, 7, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    h = lambda o: o.h if o is not None else None     # noqa: E731

    def dev(eng=c.e, index=ix, q=c.mc, r0=0, r1=n, items=c.mi, x=None, top_k=K, n_probe=2, link=0, out_i=oi.ptr, out_s=os_.ptr, out_n=on.ptr):
        return lib.fmx_topk_index_device(h(eng), h(index), h(q), r0, r1, h(items), h(x), top_k, n_probe, link, out_i, out_s, out_n)

    def host(eng=c.e, index=ix, q=c.mc, items=c.mi, x=None, top_k=K, n_probe=2, link=0, out_i=p(hi), out_s=p(hs), out_n=p(hn)):
        return lib.fmx_topk_index(h(eng), h(index), h(q), h(items), h(x), top_k, n_probe, link, out_i, out_s, out_n)
    try:
        for f in (dev, host):
            refused = [f(eng=None), f(index=None), f(q=None), f(items=None), f(out_i=None), f(out_s=None), f(eng=other_p), f(eng=other_k), f(items=fewer),
                       f(x=bad_x), f(top_k=0), f(top_k=1025), f(n_probe=0), f(n_probe=7), f(n_probe=-1), f(link=4), f(link=-1)]
            assert all(st == L.ERR_INVALID for st in refused), (f.__name__, refused)
            assert lib.fmx_last_error().decode()
        assert [dev(r0=-1), dev(r1=n + 1), dev(r0=3, r1=2)] == [L.ERR_INVALID] * 3
        out = ctypes.c_void_p(0x1234)
        asg = np.zeros(200, np.uint32); asg[[150, 60]] = 6
        cen = np.zeros((6, k + 1))
        assert lib.fmx_index_from_assign(c.e.h, 200, 6, p(asg), p(cen), ctypes.byref(out)) == L.ERR_INVALID and out.value is None
        assert "assign[60]" in lib.fmx_last_error().decode()                  # the lowest offending item
        out.value = 0x1234
        assert lib.fmx_index_build(c.e.h, c.mi.h, 201, 1, 0, ctypes.byref(out)) == L.ERR_INVALID and out.value is None
        out.value = 0x1234
        assert lib.fmx_index_build(other_p.h, c.mi.h, 4, 1, 0, ctypes.byref(out)) == L.ERR_INVALID and out.value is None
        assert dev(r0=2, r1=2) == L.OK and dev(r0=2, r1=2, out_i=None, out_s=None, out_n=None) == L.OK and dev(q=empty, r1=0) == L.OK
        assert host(q=empty) == L.OK and host(q=empty, out_i=None, out_s=None, out_n=None) == L.OK
        c.e.sync()
        assert np.all(oi.numpy() == 7) and np.all(os_.numpy() == 7.0) and np.all(on.numpy() == 7)
        assert np.all(hi == 7) and np.all(hs == 7.0) and np.all(hn == 7)
        want = c.e.topk_index(ix, c.mc, c.mi, K, 2)                           # the same buffers take a real call afterwards
        assert dev() == L.OK and host() == L.OK and host(out_n=None) == L.OK
        c.e.sync()
        assert _eq((oi.numpy().reshape(n, K), os_.numpy().reshape(n, K), on.numpy()), want) and _eq((hi, hs, hn), want)
        none = c.e.index_from_assign(np.zeros(0, np.uint32), np.zeros((2, k + 1)))   # an index of no items: every slot is padding
        assert none.non_empty == 0
        got = c.e.topk_index(none, c.mc, empty, K, 1)
        assert np.all(got[0] == -1) and np.all(np.isnan(got[1])) and np.all(got[2] == 0)
    finally:
        oi.free(); os_.free(); on.free()


# ---------------------------------------------------------------------------------------------------------------- end to end

def test_fm_index_fm_recommend_indexed_fm_index_recall_on_the_planted_problem():
    import fmwr_amd as fm
    pl = im.planted()
    ni, nc, k = len(pl["si"]), len(pl["sc"]), pl["si"].shape[1]
    p = ni + nc
    ctl = {"model": fm.model_control("REGRESSION", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    w0 = 0.25
    fit = {"Model": {"w0": w0, "w": np.concatenate([pl["bi"], pl["bc"] - w0]), "v": np.concatenate([pl["si"], pl["sc"]]).T.copy(),
                     "model.control": ctl["model"], "solver.control": ctl["solver"], "track.control": ctl["track"]},
           "Scales": {"mean": None, "std": None, "target.range": (-1e300, 1e300)}}
    items = fm.fm_matrix(sp.eye(ni, p, format="csr"))
    ctx = fm.fm_matrix(sp.eye(nc, p, k=ni, format="csr"))
    emb = fm.fm_embed(fit, items, normalize=False)
    assert np.array_equal(emb["s"], pl["si"]) and np.array_equal(emb["base"], pl["bi"])
    ix = fm.fm_index(fit, items, n_lists=pl["n_lists"], n_iter=pl["n_iter"], seed=pl["seed"], normalize=False)
    want = im.build(im.augment(pl["si"], pl["bi"]), pl["n_lists"], pl["n_iter"], pl["seed"])
    for got, w_ in zip(ix.export(), want):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(w_).view(np.uint8))
    K = pl["top_k"]
    full = fm.fm_recommend(fit, ctx, items, top_k=K, normalize=False)
    one = fm.fm_recommend_indexed(fit, ix, ctx, items, top_k=K, n_probe=1, normalize=False)
    assert set(one) == {"index", "score", "scanned"}
    assert np.array_equal(one["index"], full["index"]) and _same(one["score"], full["score"])
    assert np.all(pl["cluster"][one["index"]] == pl["ctx_cluster"][:, None])
    assert np.array_equal(one["scanned"], np.bincount(pl["cluster"])[pl["ctx_cluster"]])
    rec = fm.fm_index_recall(fit, ix, ctx, items, K, [1, 2, pl["n_lists"]], normalize=False)
    assert list(rec["n_probe"]) == [1, 2, pl["n_lists"]] and np.all(rec["recall"] == 1.0) and rec["scanned"][-1] == ni
    assert np.all(np.diff(rec["scanned"]) > 0)
    excl = [full["index"][c, :3] for c in range(nc)]                               # without each context's three best
    got = fm.fm_recommend_indexed(fit, ix, ctx, items, top_k=K, n_probe=pl["n_lists"], exclude=excl, normalize=False)
    ref = fm.fm_recommend(fit, ctx, items, top_k=K, exclude=excl, normalize=False)
    assert np.array_equal(got["index"], ref["index"]) and _same(got["score"], ref["score"])
    default = fm.fm_index(fit, items, normalize=False)
    assert default.n_lists == int(round(np.sqrt(ni)))
