"""tests/diversify_model.py (the numpy model of fmx_diversify) against a brute-force restatement of the contract, the consequences the contract
promises, the min-max edge cases, a planted problem where diversification must show, and the declared surface.  No GPU."""
import math
import os
import re

import numpy as np

from tests import diversify_model as dm
from tests import lists_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH32, CH64 = dm.chain_exact(np.float32), dm.chain_exact(np.float64)


def _bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(a == 0, 0.0, a).view(np.uint64)   # the sign of a zero is canonicalised


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _brute(s, index, score, top_k, lam, mode, dt):
    """the contract once more, slot by slot in plain Python: the largest similarity over the selected set is recomputed from scratch at every
    step and the winner is found with lists_model.before"""
    ni, P = len(s), len(index)
    live = [0 <= int(j) < ni for j in index]

    def d(i, j):
        return float(dm._chain(s[i], s[j], dt))

    def inv(i):
        n = d(i, i)
        return 1.0 / math.sqrt(n) if math.isfinite(n) and n > 0 else 0.0

    def sim(u, v):
        a, b = inv(int(index[u])), inv(int(index[v]))
        return 0.0 if a == 0 or b == 0 else (d(int(index[u]), int(index[v])) * a) * b

    rel = [float(x) for x in score]
    if mode == dm.REL_MINMAX:
        nums = [float(score[u]) for u in range(P) if live[u] and not math.isnan(score[u])]
        hi, lo = (max(nums) + 0.0, min(nums) + 0.0) if nums else (math.nan, math.nan)   # (-0 + 0 = +0)
        ok = math.isfinite(hi) and math.isfinite(lo) and hi > lo
        with np.errstate(all="ignore"):
            rel = [float(score[u]) if math.isnan(score[u]) else (float((np.float64(score[u]) - lo) / np.float64(hi - lo)) if ok else 0.0) for u in range(P)]
    mu = 1.0 - float(lam)
    chosen, out = [], []
    while len(chosen) < top_k:
        best = None
        for u in range(P):
            if not live[u] or u in chosen:
                continue
            pen = max([sim(u, v) for v in chosen]) if chosen else 0.0
            with np.errstate(all="ignore"):
                m = float(np.float64(lam) * np.float64(rel[u]) - np.float64(mu) * np.float64(pen))
            key = (int(index[u]), u)
            if best is None or lists_model.before(m, key, best[0], best[1]):
                best = (m, key)
        if best is None:
            break
        chosen.append(best[1][1])
        out.append((best[1][0], score[best[1][1]], dm.QNAN if math.isnan(best[0]) else best[0]))
    oi, os_, om = np.full(top_k, -1, np.int64), np.full(top_k, dm.QNAN), np.full(top_k, dm.QNAN)
    for t, (i, sc, m) in enumerate(out):
        oi[t], os_[t], om[t] = i, sc, m
    return oi, os_, om


def _random_row(rng, ni, k, dt):
    """one pool with the edge cases mixed in at random: ties, NaN and +-inf scores, zero rows, duplicates, empty slots"""
    P = int(rng.choice([1, 1, 2, 3, 5, 8, 9]))
    index = rng.integers(0, ni, P).astype(np.int64) if rng.random() < 0.5 else rng.permutation(ni)[:P].astype(np.int64)
    score = rng.normal(0, 1, P)
    if rng.random() < 0.4:
        score = np.round(score)           # ties
    for val in (np.nan, np.inf, -np.inf, -0.0, 0.0):
        if rng.random() < 0.15:
            score[rng.integers(0, P)] = val
    if rng.random() < 0.3:
        index[rng.integers(0, P)] = -1    # an empty slot
    if rng.random() < 0.05:
        index[:] = -1
    K = int(rng.choice([1, P, max(1, P // 2)]))
    return index, score, K


def test_the_model_equals_the_brute_force_restatement():
    rng = np.random.default_rng(20)
    n = 0
    for dt, ch in ((np.float32, CH32), (np.float64, CH64)):
        for k in (0, 1, 3, 6):
            ni = 9
            s = rng.normal(0, 1, (ni, k)).astype(dt).astype(np.float64)
            if k:
                s[2] = 0.0                      # a zero row
                s[5] = s[4]                     # two items with one projection
                s[7] = -s[4]
            for _ in range(25):
                index, score, K = _random_row(rng, ni, k, dt)
                for lam in (rng.choice([0.0, 0.3, 0.7, 1.0]),):
                    for mode in (dm.REL_SCORE, dm.REL_MINMAX):
                        got = dm.diversify(s, index, score, K, lam, mode, ch)
                        want = _brute(s, index, score, K, lam, mode, dt)
                        assert np.array_equal(got[0], want[0]), (k, index, score, K, lam, mode, got, want)
                        assert _same(got[1], want[1]) and _same(got[2], want[2]), (k, index, score, K, lam, mode, got, want)
                n += 1
    assert n == 200


def _problem(seed, ni=30, k=4, nrows=8, P=12):
    rng = np.random.default_rng(seed)
    s = rng.normal(0, 1, (ni, k)).astype(np.float32).astype(np.float64)
    index = np.array([rng.permutation(ni)[:P] for _ in range(nrows)], np.int64)
    score = rng.normal(0, 1, (nrows, P))
    return rng, s, index, score


def test_consequence_a_trade_off_one_is_the_ranking_by_score():
    rng, s, index, score = _problem(1)
    score[0, 3] = score[0, 5]; score[1, 2] = np.nan; score[2, 4] = np.inf; score[2, 6] = -np.inf; score[3, :] = 0.0
    index[4, 7] = -1
    for c in range(len(index)):
        dense = np.full(len(s), np.nan)
        live = index[c] >= 0
        dense[index[c][live]] = score[c][live]
        for K in (1, 5, 12):
            oi, os_, om = dm.diversify(s, index[c], score[c], K, 1.0, dm.REL_SCORE, CH32)
            wi, ws = lists_model.topk(dense, index[c][live], K)
            assert np.array_equal(oi, wi) and _same(os_, ws), (c, K)
            assert _same(om[wi >= 0], os_[wi >= 0] - 0.0)    # the margin is 1 * score - 0 * pen


def test_consequence_b_a_row_alone_and_the_slot_order():
    rng, s, index, score = _problem(2)
    for mode in (dm.REL_SCORE, dm.REL_MINMAX):
        whole = dm.diversify_rows(s, index, score, 6, 0.6, mode, CH32)
        for c in range(len(index)):
            alone = dm.diversify(s, index[c], score[c], 6, 0.6, mode, CH32)
            assert all(_same(a, w[c]) for a, w in zip(alone, whole))
            q = rng.permutation(index.shape[1])     # distinct items: the order of the slots does not matter
            moved = dm.diversify(s, index[c][q], score[c][q], 6, 0.6, mode, CH32)
            assert all(_same(a, b) for a, b in zip(alone, moved))


def test_consequence_c_a_smaller_top_k_is_a_prefix():
    rng, s, index, score = _problem(3)
    index[0, :9] = -1    # three candidates only
    for mode in (dm.REL_SCORE, dm.REL_MINMAX):
        full = dm.diversify_rows(s, index, score, 12, 0.4, mode, CH32)
        for K in (1, 2, 7):
            part = dm.diversify_rows(s, index, score, K, 0.4, mode, CH32)
            assert all(_same(p, f[:, :K]) for p, f in zip(part, full))
        assert np.all(full[0][0, 3:] == -1) and np.all(np.isnan(full[1][0, 3:])) and np.all(np.isnan(full[2][0, 3:]))


def test_minmax_edge_cases():
    s = np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [2.0, 0.0]])
    live = np.ones(4, bool)
    # all scores equal: hi == lo, every relevance is +0
    r = dm.relevance(np.full(4, 3.5), live, dm.REL_MINMAX)
    assert _same(r, np.zeros(4)) and not np.signbit(r).any()
    # one candidate
    r = dm.relevance(np.array([7.0]), np.ones(1, bool), dm.REL_MINMAX)
    assert _same(r, [0.0])
    oi, os_, om = dm.diversify(s, [2], [7.0], 1, 0.7, dm.REL_MINMAX, CH64)
    assert oi[0] == 2 and os_[0] == 7.0 and om[0] == 0.0
    # NaN among numbers: the bounds skip it, it stays NaN and is picked last
    r = dm.relevance(np.array([1.0, np.nan, 3.0, 2.0]), live, dm.REL_MINMAX)
    assert r[0] == 0.0 and np.isnan(r[1]) and r[2] == 1.0 and r[3] == 0.5
    oi, os_, om = dm.diversify(s, [0, 1, 2, 3], [1.0, np.nan, 3.0, 2.0], 4, 1.0, dm.REL_MINMAX, CH64)
    assert oi.tolist() == [2, 3, 0, 1] and np.isnan(os_[3]) and np.isnan(om[3])
    # an infinite score: no finite range, every relevance is 0 and the order is the item order
    r = dm.relevance(np.array([1.0, np.inf, 3.0, 2.0]), live, dm.REL_MINMAX)
    assert _same(r, np.zeros(4))
    # an empty slot's score does not enter the bounds
    r = dm.relevance(np.array([1.0, 100.0, 3.0, 2.0]), np.array([True, False, True, True]), dm.REL_MINMAX)
    assert r[2] == 1.0 and r[0] == 0.0
    # zeros of both signs: the bounds are +0
    r = dm.relevance(np.array([-0.0, 0.0, 1.0, -0.0]), live, dm.REL_MINMAX)
    assert _same(r, [0.0, 0.0, 1.0, 0.0])


def planted():
    """items in a few tight clusters, relevance correlated with one of them: (clusters covered, mean relevance) of the top K by score and of
    the K picked at trade_off 0.7"""
    rng = np.random.default_rng(8)
    n_cl, per, k, K, P = 5, 20, 8, 10, 60
    centre = rng.normal(0, 1, (n_cl, k))
    cl = np.repeat(np.arange(n_cl), per)
    s = (centre[cl] + 0.05 * rng.normal(0, 1, (n_cl * per, k))).astype(np.float32).astype(np.float64)
    score = rng.normal(0, 1, n_cl * per) + 1.5 * (cl == 0)      # cluster 0 is liked
    pool = np.argsort(-score, kind="stable")[:P].astype(np.int64)
    top = pool[:K]
    oi, os_, _ = dm.diversify(s, pool, score[pool], K, 0.7, dm.REL_MINMAX, dm.chain_exact(np.float32))
    return (len(set(cl[top])), float(score[top].mean())), (len(set(cl[oi])), float(os_.mean()))


def test_planted_clusters_are_covered():
    (c_top, r_top), (c_div, r_div) = planted()
    print(f"top-K by score: {c_top} clusters, mean relevance {r_top:.4f}; MMR at 0.7: {c_div} clusters, mean relevance {r_div:.4f}")
    assert c_div > c_top and r_div <= r_top


def test_the_declared_surface():
    header = open(os.path.join(ROOT, "include", "fmx.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+fmx_diversify\s*\(", code) and re.search(r"\bint\s+fmx_diversify_device\s*\(", code)
    assert re.search(r"#define\s+FMX_DIV_REL_SCORE\s+0\b", code) and re.search(r"#define\s+FMX_DIV_REL_MINMAX\s+1\b", code)
    from fmwr_amd import _lib as L, api, engine
    import fmwr_amd
    assert "fmx_diversify" in L.SYMBOLS and "fmx_diversify_device" in L.SYMBOLS and "fmx_debug_diversify_limits" in L.TEST_HOOKS
    assert (L.DIV_REL_SCORE, L.DIV_REL_MINMAX) == (dm.REL_SCORE, dm.REL_MINMAX) == (0, 1)
    assert callable(engine.Engine.diversify) and callable(engine.Engine.diversify_device)
    assert callable(api.fm_diversify) and fmwr_amd.fm_diversify is api.fm_diversify
    hooks = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fmx_test_hooks.h")).read()
    assert "fmx_debug_diversify_limits" in hooks
