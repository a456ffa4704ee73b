"""tests/index_model.py (the numpy model of the clustered item index) against a brute-force loop over the contract in plain Python, the consequences
the contract states, the seed order against a restatement of pair_hash, the empty-list and non-finite-item rules, a planted problem on which
one probe already gives the full ranking, the declared surface and every refusal that needs no device.  No GPU."""
import ctypes as C
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import index_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    a = np.where(np.isnan(a), im.QNAN, np.where(a == 0, 0.0, a))   # one NaN, one zero
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _fma(a, b, c):
    """the fp64 fma through Fractions (finite values)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fma64_equals_the_fraction_fma():
    rng = np.random.default_rng(1)
    a, b = rng.normal(0, 1, 3000), rng.normal(0, 1, 3000)
    c = np.concatenate([rng.normal(0, 1, 1000), -(a[1000:2000] * b[1000:2000]), rng.normal(0, 1e-17, 1000)])   # plain, cancelling, a sticky tail
    a[:50] *= 2.0 ** 200; c[50:100] *= 2.0 ** -300
    a[100:110] = 0.0
    got = im.fma64(a, b, c)
    want = np.array([_fma(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.any(got != a * b + c)                                    # the samples tell an fma from two roundings
    with np.errstate(all="ignore"):
        assert np.isnan(im.fma64(np.inf, 0.0, 1.0)) and im.fma64(np.inf, 1.0, 1.0) == np.inf and np.isnan(im.fma64(1.0, 1.0, np.nan))
        assert np.isnan(im.fma64(np.inf, 1.0, -np.inf)) and im.fma64(2.0, 3.0, -np.inf) == -np.inf


def _case(seed, n=200, k=3, n_lists=12, nc=20, dt=np.float32):
    """projections in the state type dt with edge rows: items 8 and 9 are twins, 30 has a NaN factor, 31 an infinite base"""
    rng = np.random.default_rng(seed)
    si = rng.normal(0, 0.5, (n, k)).astype(dt).astype(np.float64)
    bi = rng.normal(0, 0.3, n)
    si[9], bi[9] = si[8], bi[8]
    si[30, 0] = np.nan
    bi[31] = np.inf
    sc = rng.normal(0, 0.5, (nc, k)).astype(dt).astype(np.float64)
    bc = rng.normal(0, 0.3, nc)
    return si, bi, sc, bc


def _before(sa, ia, sb, ib):
    an, bn = sa != sa, sb != sb
    if an != bn:
        return bn
    if not an and sa != sb:
        return sa > sb
    return ia < ib


def _sorted(pairs):
    return sorted(pairs, key=functools.cmp_to_key(lambda x, y: -1 if _before(x[0], x[1], y[0], y[1]) else 1))


def _brute_build(a, n_lists, n_iter, seed):
    n, D = a.shape
    fin = [all(math.isfinite(x) for x in a[i]) for i in range(n)]
    order = sorted((int(_hash(seed, 0, i, 5)), i) for i in range(n) if fin[i])
    mu = [list(a[i]) for _, i in order[:n_lists]]

    def assign():
        out = []
        for i in range(n):
            best, bl = math.inf, 0
            for l in range(n_lists if fin[i] else 0):    # (the centroids of a build are finite: seeds and means of finite items)
                acc = 0.0
                for f in range(D):
                    t = float(a[i, f]) - float(mu[l][f])
                    acc = _fma(t, t, acc)
                if acc < best:
                    best, bl = acc, l
            out.append(bl)
        return out

    for _ in range(n_iter):
        asg = assign()
        for l in range(n_lists):
            mem = [i for i in range(n) if asg[i] == l]
            live = [i for i in mem if fin[i]]
            if not live:
                continue
            for f in range(D):
                mu[l][f] = im.ordered_sum(np.array([a[i, f] if fin[i] else 0.0 for i in mem])) / float(len(live))
    return np.array(mu), np.array(assign(), np.uint32)


def _hash(seed, epoch, t, stream):
    """fm_rank.h's pair_hash restated on Python integers"""
    def mix(x):
        x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
        x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
        return x ^ x >> 31
    h = mix(seed + 0x9E3779B97F4A7C15 & M64)
    h = mix(h ^ (epoch * 0xD6E8FEB86659FD93 + stream & M64))
    return mix(h ^ (t + 0x632BE59BD9B4E019 & M64))


def test_the_seed_order_is_pair_hash_stream_5():
    si, bi, _, _ = _case(3)
    a = im.augment(si, bi)
    for seed in (0, 7, 2 ** 63 + 11):
        want = [i for _, i in sorted((_hash(seed, 0, i, 5), i) for i in range(len(a)) if i not in (30, 31))]
        assert list(im.seed_order(a, seed)) == want
        assert int(im.pair_hash(seed, 0, np.array([17]), 5)[0]) == _hash(seed, 0, 17, 5)
    assert list(im.seed_order(a, 0)) != list(im.seed_order(a, 1))


@pytest.mark.parametrize("n_iter", [0, 2])
def test_the_build_equals_a_brute_force_loop(n_iter):
    si, bi, _, _ = _case(4, n=120)
    a = im.augment(si, bi)
    mu, asg, ptr, item = im.build(a, 12, n_iter, seed=5)
    bmu, basg = _brute_build(a, 12, n_iter, 5)
    assert np.array_equal(mu.view(np.uint64), bmu.view(np.uint64)) and np.array_equal(asg, basg)
    assert asg[30] == 0 and asg[31] == 0                                                  # non-finite items: list 0
    assert ptr[0] == 0 and ptr[-1] == len(a) and all(list(item[ptr[l]:ptr[l + 1]]) == [i for i in range(len(a)) if asg[i] == l] for l in range(12))
    if n_iter == 0:
        assert np.array_equal(mu.view(np.uint64), a[im.seed_order(a, 5)[:12]].view(np.uint64))
    assert np.array_equal(asg, im.assign(a, mu))                                          # the exported assign is the arg-min of the exported centroids


def test_the_search_equals_a_brute_force_loop():
    dt = np.float32
    si, bi, sc, bc = _case(6)
    a = im.augment(si, bi)
    mu, asg, ptr, item = im.build(a, 12, 2, seed=1)
    mu[3] = mu[2]                                                                         # tied g: the lower list first
    mu[5, 0] = np.nan                                                                     # a NaN g: below every number, still probed last
    chain = im.chain_exact(dt)
    finite = ~np.isin(np.arange(len(si)), (30, 31))
    score = np.full((len(sc), len(si)), np.nan)
    score[:, finite] = im.pair_scores(sc, bc, si[finite], bi[finite], chain)
    score[:, 31] = np.inf
    excl = [np.array([], np.int64) if c % 3 else item[ptr[asg[c]]:ptr[asg[c] + 1]][::2] for c in range(len(sc))]
    K = 10
    for n_probe in (1, 2, 5, 12):
        for x in (None, excl):
            got = im.search_scores(score, im.coarse(sc, mu), ptr, item, K, n_probe, x)
            for c in range(len(sc)):
                g = []
                for l in range(12):
                    if ptr[l + 1] == ptr[l]:
                        continue
                    acc = 0.0
                    for f in range(si.shape[1]):
                        acc = _fma(sc[c, f], mu[l, f], acc) if math.isfinite(mu[l, f]) and math.isfinite(acc) else math.nan
                    g.append((float(mu[l, -1]) + acc, l))
                probed = [l for _, l in _sorted(g)[:n_probe]]
                cand = [int(i) for l in probed for i in item[ptr[l]:ptr[l + 1]]]
                assert got[2][c] == len(cand)
                if x is not None:
                    cand = [i for i in cand if i not in set(x[c].tolist())]
                want = _sorted([(score[c, i], i) for i in cand])[:K]
                assert list(got[0][c][:len(want)]) == [i for _, i in want] and np.all(got[0][c][len(want):] == -1)
                assert _same(got[1][c][:len(want)], [s for s, _ in want]) and np.all(np.isnan(got[1][c][len(want):]))


def test_the_stated_consequences():
    si, bi, sc, bc = _case(8, dt=np.float64)
    finite = ~np.isin(np.arange(len(si)), (30, 31))
    si, bi = si[finite], bi[finite]
    a = im.augment(si, bi)
    mu, asg, ptr, item = im.build(a, 12, 3, seed=2)
    score = im.pair_scores(sc, bc, si, bi, im.chain_dot)
    g = im.coarse(sc, mu)
    K = 25
    excl = [np.arange(c, len(si), 7) for c in range(len(sc))]
    for x in (None, excl):
        full = im.full_ranking(score, K, x)
        runs = [im.search_scores(score, g, ptr, item, K, q, x) for q in range(1, 13)]
        assert np.array_equal(runs[-1][0], full[0]) and _same(runs[-1][1], full[1])          # every list probed: the full ranking
        assert np.all(runs[-1][2] == len(si))
        for lo, hi in zip(runs, runs[1:]):                                                   # nested probe sets: slot t never moves back
            assert np.all(hi[2] >= lo[2])
            for c in range(len(sc)):
                for t in range(K):
                    if lo[0][c, t] >= 0:
                        assert hi[0][c, t] >= 0 and not _before(lo[1][c, t], lo[0][c, t], hi[1][c, t], hi[0][c, t])
        rows = [13, 2, 2, 19]                                                                # a row's result does not depend on the other rows
        sub = im.search_scores(score[rows], g[rows], ptr, item, K, 3, None if x is None else [x[r] for r in rows])
        assert np.array_equal(sub[0], runs[2][0][rows]) and _same(sub[1], runs[2][1][rows]) and np.array_equal(sub[2], runs[2][2][rows])


def test_empty_lists_and_non_finite_items():
    rng = np.random.default_rng(9)
    a = rng.integers(-8, 9, (40, 3)) / 8.0
    a[7] = a[3]                                                       # duplicates: identical seeds can leave the higher list empty
    a[11, 1] = np.nan
    a[12, 2] = -np.inf
    mu = np.array([a[3], a[7], a[5], [np.nan, 0, 0], [9.0, 9.0, 9.0]])
    asg = im.assign(a, mu)
    assert asg[3] == 0 and asg[7] == 0 and not np.any(asg == 1)       # identical centroids: the first one takes the items
    assert not np.any(asg == 3)                                       # a NaN centroid attracts nothing
    assert asg[11] == 0 and asg[12] == 0
    ptr, item = im.lists(asg, 5)
    new = im.update(a, mu, ptr, item)
    assert np.array_equal(new[[1, 3]].view(np.uint64), mu[[1, 3]].view(np.uint64))   # lists without finite members keep their bits
    live = [i for i in range(40) if asg[i] == 0 and i not in (11, 12)]
    mean, bar, has = im.update_bars(a, mu, ptr, item)
    assert list(has) == [True, False, True, False, bool(np.any(asg == 4))]
    assert np.all(np.abs(new[0] - a[live].sum(0) / len(live)) <= bar[0]) and np.all(np.isfinite(new[0]))   # non-finite members stay out of the sums
    # an item whose every distance overflows goes to list 0; a search over an index with empty lists never probes them
    big = np.array([[1e200, 0.0, 0.0]])
    assert im.assign(big, np.array([[-1e200, 0, 0], [-1e200, 1, 0]]))[0] == 0
    g = im.coarse(np.zeros((1, 2)), mu)
    assert list(im.probe_set(g[0], ptr, 5)) == [l for l in im.probe_set(g[0], ptr, 5) if ptr[l + 1] > ptr[l]] and len(im.probe_set(g[0], ptr, 5)) == int(np.sum(np.diff(ptr) > 0))
    # ordered_sum: one chunk and several, against fsum within the bar
    x = rng.normal(0, 1, 2500)
    assert abs(im.ordered_sum(x) - math.fsum(x)) <= len(x) * 2.0 ** -53 * math.fsum(np.abs(x))
    assert im.ordered_sum(np.arange(1, 2051, dtype=np.float64)) == 2050 * 2051 / 2


def test_planted_clusters_one_probe_gives_the_full_ranking():
    p = im.planted()
    a = im.augment(p["si"], p["bi"])
    mu, asg, ptr, item = im.build(a, p["n_lists"], p["n_iter"], p["seed"])
    assert all(len(set(p["cluster"][item[ptr[l]:ptr[l + 1]]])) == 1 for l in range(p["n_lists"])) and np.all(np.diff(ptr) > 0)   # the lists are the clusters
    K = p["top_k"]
    assert K <= np.bincount(p["cluster"]).min()
    score = im.pair_scores(p["sc"], p["bc"], p["si"], p["bi"], im.chain_dot)
    full = im.full_ranking(score, K)
    assert np.all(p["cluster"][full[0]] == p["ctx_cluster"][:, None])
    one = im.search_scores(score, im.coarse(p["sc"], mu), ptr, item, K, 1)
    assert np.array_equal(one[0], full[0]) and _same(one[1], full[1])
    assert np.all(one[2] == np.bincount(p["cluster"])[p["ctx_cluster"]])


def test_the_declared_surface():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    names = ("fmx_index_build", "fmx_index_from_assign", "fmx_index_info", "fmx_index_export", "fmx_index_free", "fmx_topk_index", "fmx_topk_index_device")
    from fmwr_amd import _lib as L, api, engine
    import fmwr_amd
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, code) and name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert re.search(r"typedef\s+struct\s+fmx_item_index\s+fmx_item_index\s*;", code)
    assert re.search(r"#define\s+FMX_INDEX_MAX_LISTS\s+65536\b", code) and re.search(r"#define\s+FMX_INDEX_MAX_ITER\s+100\b", code)
    assert (api.INDEX_MAX_LISTS, api.INDEX_MAX_ITER) == (im.MAX_LISTS, im.MAX_ITER) == (65536, 100)
    assert "fmx_debug_index_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_index_limits")
    hooks = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fmwr_amd", "csrc", "fmx_test_hooks.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+fmx_debug_index_limits\s*\(\s*int32_t\s+fine_form\s*,\s*int64_t\s+chunk_rows\s*,\s*int32_t\s+assign_slice_lists\s*\)", hooks)
    for m in ("index_build", "index_from_assign", "topk_index", "topk_index_device"):
        assert callable(getattr(engine.Engine, m)), m
    for attr in ("centroids", "assign", "list_ptr", "list_item"):
        assert isinstance(getattr(engine.ItemIndex, attr), property), attr
    for f in ("fm_index", "fm_recommend_indexed", "fm_index_recall"):
        assert callable(getattr(api, f)) and getattr(fmwr_amd, f) is getattr(api, f), f
    assert "fm_index.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES


def test_refusals_without_a_device_leave_the_outputs_untouched():
    from fmwr_amd import _lib as L
    lib = L.lib()
    none = C.c_void_p(None)
    # a pointer that must not be read: the NULL engine / index / matrix is met first
    fake = C.c_void_p(8)
    out = C.c_void_p(0x1234)
    for n_lists, n_iter in ((0, 1), (65537, 1), (-1, 1), (4, -1), (4, 101), (4, 1)):       # the limits, then the NULL engine
        out.value = 0x1234
        assert lib.fmx_index_build(none, none, n_lists, n_iter, 0, C.byref(out)) == L.ERR_INVALID and out.value is None   # *out = NULL
        assert lib.fmx_last_error()
    assert lib.fmx_index_build(none, none, 4, 1, 0, None) == L.ERR_INVALID
    asg, cen = np.zeros(4, np.uint32), np.zeros((2, 3))
    for n_items, n_lists in ((-1, 2), (2 ** 31 - 1, 2), (4, 0), (4, 65537), (4, 2)):
        out.value = 0x1234
        st = lib.fmx_index_from_assign(none, n_items, n_lists, asg.ctypes.data_as(C.c_void_p), cen.ctypes.data_as(C.c_void_p), C.byref(out))
        assert st == L.ERR_INVALID and out.value is None
    assert lib.fmx_index_from_assign(none, 4, 2, asg.ctypes.data_as(C.c_void_p), cen.ctypes.data_as(C.c_void_p), None) == L.ERR_INVALID
    i64, i32 = C.c_int64(77), C.c_int32(77)
    assert lib.fmx_index_info(none, C.byref(i64), C.byref(i32), C.byref(i32), C.byref(i64)) == L.ERR_INVALID and (i64.value, i32.value) == (77, 77)
    keep = np.full(6, 5.0)
    assert lib.fmx_index_export(none, keep.ctypes.data_as(C.c_void_p), None, None, None) == L.ERR_INVALID and np.all(keep == 5.0)
    assert lib.fmx_index_free(none) == L.OK
    oi, os_, sc = np.full(8, 5, np.int64), np.full(8, 5.0), np.full(2, 5, np.int64)
    ptrs = [x.ctypes.data_as(C.c_void_p) for x in (oi, os_, sc)]
    for n_probe in (0, -3, 1):
        assert lib.fmx_topk_index(none, fake, none, none, none, 4, n_probe, L.LINK_NONE, *ptrs) == L.ERR_INVALID
        assert lib.fmx_topk_index_device(none, fake, none, 0, 2, none, none, 4, n_probe, L.LINK_NONE, *ptrs) == L.ERR_INVALID
    assert np.all(oi == 5) and np.all(os_ == 5.0) and np.all(sc == 5)
    assert lib.fmx_debug_index_limits(3, 0, 0) == L.ERR_INVALID and lib.fmx_debug_index_limits(-1, 0, 0) == L.ERR_INVALID   # no such fine form
    assert lib.fmx_debug_index_limits(2, 0, 0) == L.OK and lib.fmx_debug_index_limits(0, 0, 0) == L.OK


def test_python_refusals_come_before_any_device():
    import scipy.sparse as sp
    import fmwr_amd as fm
    from fmwr_amd import engine
    rng = np.random.default_rng(0)
    p, k = 12, 2
    ctl = {"model": fm.model_control("REGRESSION", **{"factor.number": k}), "solver": fm.solver_control(max_iter=10, solver=fm.SGD_solver()),
           "track": fm.track_control()}
    fit = {"Model": {"w0": 0.25, "w": rng.normal(size=p), "v": rng.normal(size=(k, p)), "model.control": ctl["model"],
                     "solver.control": ctl["solver"], "track.control": ctl["track"]},
           "Scales": {"mean": None, "std": None, "target.range": (-1e300, 1e300)}}
    items = fm.fm_matrix(sp.eye(9, p, format="csr"))
    for kw in ({"n_lists": 0}, {"n_lists": 10}, {"n_lists": 2.5}, {"n_lists": True}, {"n_iter": -1}, {"n_iter": 101}, {"seed": -1}, {"seed": 2 ** 64}):
        with pytest.raises(ValueError):
            fm.fm_index(fit, items, normalize=False, **kw)
    with pytest.raises(TypeError):
        fm.fm_index(fit, np.eye(3), normalize=False)
    with pytest.raises(ValueError):
        fm.fm_index(fit, fm.fm_matrix(sp.eye(9, p + 1, format="csr")), normalize=False)
    with pytest.raises(TypeError):
        fm.fm_recommend_indexed(fit, object(), items, items, normalize=False)
    with pytest.raises(TypeError):
        fm.fm_index_recall(fit, None, items, items, 3, [1], normalize=False)
    ix = engine.ItemIndex.__new__(engine.ItemIndex)                      # a handle-less stand-in: the checks below never reach the library
    ix.h, ix.n_items, ix.n_lists, ix.k, ix.non_empty = None, 9, 3, k, 3
    for kw in ({"top_k": 0}, {"top_k": 1025}, {"top_k": 1.5}, {"n_probe": 0}, {"n_probe": 4}, {"n_probe": 2.5}):
        with pytest.raises(ValueError):
            fm.fm_recommend_indexed(fit, ix, items, items, normalize=False, **kw)
    with pytest.raises(ValueError):
        fm.fm_recommend_indexed(fit, ix, items, fm.fm_matrix(sp.eye(8, p, format="csr")), normalize=False)   # not the indexed items
    for probes in ([0], [1, 4], [1.5]):
        with pytest.raises(ValueError):
            fm.fm_index_recall(fit, ix, items, items, 3, probes, normalize=False)
