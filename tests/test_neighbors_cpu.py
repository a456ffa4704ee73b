"""tests/neighbors_model.py (the numpy model of fmx_neighbors) against a brute-force double loop over the contract, the consequences the contract
promises, a planted problem where the cosine finds what the FM score does not, and the declared surface.  No GPU."""
import functools
import math
import os
import re

import numpy as np
import pytest

from tests import diversify_model as dm
from tests import neighbors_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(a == 0, 0.0, a).view(np.uint64)   # the sign of a zero is canonicalised


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rows(seed, dt, n=200, k=3):
    """n projections in the state type dt with the edge rows: 5 is zero, 9 repeats 8, 11 is -1 times 10"""
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 0.5, (n, k)).astype(dt).astype(np.float64)
    s[5] = 0.0
    s[9] = s[8]
    s[11] = -s[10]
    return s


def _brute(sq, si, top_k, metric, dt, skip_self, row0):
    """the contract pair by pair in plain Python, ordered with a comparison function"""
    def d(a, b):
        return float(dm._chain(a, b, dt))

    def inv(a):
        n = d(a, a)
        return 1.0 / math.sqrt(n) if math.isfinite(n) and n > 0 else 0.0

    def before(x, y):   # (score, index)
        (sx, ix), (sy, iy) = x, y
        nx, ny = math.isnan(sx), math.isnan(sy)
        if nx != ny:
            return -1 if ny else 1
        if not nx and sx != sy:
            return -1 if sx > sy else 1
        return -1 if ix < iy else 1

    oi, os_ = np.full((len(sq), top_k), -1, np.int64), np.full((len(sq), top_k), np.nan)
    for q in range(len(sq)):
        pairs = []
        for i in range(len(si)):
            if skip_self and i == row0 + q:
                continue
            if metric == nm.SIM_DOT:
                sc = d(sq[q], si[i])
            else:
                a, b = inv(sq[q]), inv(si[i])
                sc = 0.0 if a == 0 or b == 0 else float(np.float64(np.float64(d(sq[q], si[i])) * np.float64(a)) * np.float64(b))
            pairs.append((sc, i))
        pairs.sort(key=functools.cmp_to_key(before))
        for t, (sc, i) in enumerate(pairs[:top_k]):
            oi[q, t], os_[q, t] = i, sc
    return oi, os_


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("metric", [nm.SIM_COSINE, nm.SIM_DOT])
def test_the_model_is_the_contract(dt, metric):
    s = _rows(3, dt)
    row0 = 4                                    # queries = rows 4..15 of the items: the zero row, the twins and the negated pair among them
    sq = s[row0:16]
    chain = dm.chain_exact(dt)
    for skip in (False, True):
        got = nm.neighbors(sq, s, 12, metric, chain, skip_self=skip, row0=row0)
        want = _brute(sq, s, 12, metric, dt, skip, row0)
        assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]), (skip, got, want)
    # more slots than items: padding
    got = nm.neighbors(sq[:2], s[:5], 9, metric, chain, skip_self=True, row0=row0)    # row 4 is an item here, row 5 is not
    want = _brute(sq[:2], s[:5], 9, metric, dt, True, row0)
    assert np.array_equal(got[0], want[0]) and np.all(got[0][0, 4:] == -1) and np.all(got[0][1, 5:] == -1) and np.all(got[0][1, :5] >= 0)
    assert np.all(np.isnan(got[1][0, 4:])) and _same(np.nan_to_num(got[1], nan=7.0), np.nan_to_num(want[1], nan=7.0))
    got = nm.neighbors(sq, s[:0], 3, metric, chain)
    assert np.all(got[0] == -1) and np.all(np.isnan(got[1]))


@pytest.mark.parametrize("metric", [nm.SIM_COSINE, nm.SIM_DOT])
def test_consequences(metric):
    s = _rows(8, np.float32, n=120, k=4)
    s[20, 1] = np.nan                           # a NaN factor: the chain of numpy's dot product carries it as the fma chain does
    chain = dm.chain_dot
    sc = nm.scores(s, s, metric, chain)
    K = 15
    full = nm.select(sc, K + 1)
    for K1 in (1, 2, K):                        # the prefix property
        got = nm.select(sc, K1)
        assert np.array_equal(got[0], full[0][:, :K1]) and _same(np.nan_to_num(got[1], nan=7.0), np.nan_to_num(full[1][:, :K1], nan=7.0))
    skip = nm.select(sc, K, skip_self=True)     # skip_self = the K + 1 best without it, the own index dropped
    n_own = 0
    for q in range(len(s)):
        row = [j for j in full[0][q] if j != q][:K]
        assert list(skip[0][q]) == row
        n_own += q in full[0][q]
    assert 0 < n_own
    if metric == nm.SIM_COSINE:
        assert n_own < len(s)                   # the row whose norm is NaN scores 0 everywhere: its 16 best are items 0..15
        assert np.all(sc[5].view(np.uint64) == 0) and np.all(sc[:, 5].view(np.uint64) == 0)   # a zero row scores +0.0 against everything
        assert np.all(sc[20].view(np.uint64) == 0)                                            # and so does a row whose norm is NaN
        assert list(full[0][5]) == list(range(K + 1))                                         # equal scores: the lowest indices
        assert full[0][10][-1] != 11 and nm.select(sc, len(s))[0][10][-1] == 11               # the negated row comes last
        assert full[0][8][0] == 8 and full[0][8][1] == 9 and full[0][9][0] == 8               # the twins tie: the lower index first
    else:
        assert np.all(np.isnan(sc[20])) and np.all(np.isnan(sc[:, 20]))
        last = nm.select(sc, len(s))
        assert np.all(last[0][np.arange(len(s)) != 20, -1] == 20)                             # NaN below every number, and still listed
        assert list(last[0][20]) == list(range(len(s)))
    # the rounded cosine is not exactly symmetric, the dot product is
    t = np.random.default_rng(1).normal(0, 1, (60, 7))
    c = nm.scores(t, t, metric, dm.chain_dot)
    assert np.allclose(c, c.T, rtol=0, atol=1e-15)
    assert np.array_equal(c, c.T) == (metric == nm.SIM_DOT)


def test_planted_clusters():
    """5 clusters of item factors: every item's 10 cosine neighbours are of its own cluster; its 10 best under the FM score base + dot, with a
    popularity-biased w, are mostly the popular items of every cluster"""
    rng = np.random.default_rng(21)
    k, per, n_cl = 8, 20, 5
    ni = per * n_cl
    cluster = np.repeat(np.arange(n_cl), per)
    s = np.eye(k)[cluster] * rng.uniform(0.5, 2.0, (ni, 1)) + rng.normal(0, 0.05, (ni, k))
    s = s.astype(np.float32).astype(np.float64)
    popular = np.concatenate([c * per + np.arange(2) for c in range(n_cl)])      # two popular items per cluster
    base = np.zeros(ni)
    base[popular] = 6.0
    cos_i, _ = nm.neighbors(s, s, 10, nm.SIM_COSINE, dm.chain_dot, skip_self=True)
    fm_score = base[None, :] + nm.scores(s, s, nm.SIM_DOT, dm.chain_dot)
    fm_i, _ = nm.select(fm_score, 10, skip_self=True)
    share_cos = float(np.mean(cluster[cos_i] == cluster[:, None]))
    share_fm = float(np.mean(cluster[fm_i] == cluster[:, None]))
    print(f"own-cluster share of the 10 neighbours: cosine {share_cos:.3f}, FM score {share_fm:.3f}")
    assert share_cos == 1.0
    assert share_fm < 0.5


def test_the_declared_surface():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+fmx_neighbors\s*\(", code) and re.search(r"\bint\s+fmx_neighbors_device\s*\(", code)
    assert re.search(r"#define\s+FMX_SIM_COSINE\s+0\b", code) and re.search(r"#define\s+FMX_SIM_DOT\s+1\b", code)
    from fmwr_amd import _lib as L, api, engine
    import fmwr_amd
    assert "fmx_neighbors" in L.SYMBOLS and "fmx_neighbors_device" in L.SYMBOLS and "fmx_debug_neighbors_limits" in L.TEST_HOOKS
    assert (L.SIM_COSINE, L.SIM_DOT) == (nm.SIM_COSINE, nm.SIM_DOT) == (0, 1)
    assert callable(engine.Engine.neighbors) and callable(engine.Engine.neighbors_device)
    assert callable(api.fm_similar) and fmwr_amd.fm_similar is api.fm_similar
    hooks = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fmx_test_hooks.h")).read()
    assert re.search(r"\bint\s+fmx_debug_neighbors_limits\s*\(\s*int64_t\s+slice_items\s*,\s*int64_t\s+chunk_rows\s*\)", hooks)
