"""The numpy model of the candidate-list calls (fmx_rank_lists / fmx_topk_lists), the yardstick of tests/test_gpu_lists.py: from one context's
dense raw scores and its list, the positions of the entries and the top-K under fmx_topk's total order -- a higher score first, equal scores
(-0 = +0) by the lower item index, NaN below every number; duplicate entries count once.  tests/test_lists_cpu.py checks it against a
brute-force double loop."""
import numpy as np


def ordered(scores, items):
    """the distinct `items` of one context in the total order (scores: the context's dense raw scores, indexed by item)"""
    d = np.unique(np.asarray(items, np.int64))
    s = np.asarray(scores, np.float64)[d]
    nan = np.isnan(s)
    return d[np.lexsort((d, np.where(nan, 0.0, -s), nan))]   # keys last to first: NaN last, then the score descending, then the index


def positions(scores, items):
    """int64 position of every entry of `items` (duplicates get the same position) among the list's distinct candidates"""
    items = np.asarray(items, np.int64)
    o = ordered(scores, items)
    where = {int(j): t for t, j in enumerate(o)}
    return np.array([where[int(j)] for j in items], np.int64)


def topk(scores, items, K):
    """(index int64[K], raw score float64[K]) of the K first distinct candidates; -1 / NaN beyond them"""
    o = ordered(scores, items)[:K]
    idx = np.full(K, -1, np.int64)
    sc = np.full(K, np.nan)
    idx[:len(o)] = o
    sc[:len(o)] = np.asarray(scores, np.float64)[o]
    return idx, sc


def before(sa, ia, sb, ib):
    """the total order spelled out: does (score sa, item ia) come before (sb, ib)?"""
    an, bn = sa != sa, sb != sb
    if an != bn:
        return bn
    if not an and sa != sb:
        return sa > sb
    return ia < ib


def positions_brute(scores, items):
    """positions by the definition: pos(j) = the number of distinct candidates that come before j"""
    out = []
    for j in items:
        seen, cnt = set(), 0
        for j2 in items:
            if j2 in seen:
                continue
            seen.add(j2)
            cnt += 1 if before(scores[j2], j2, scores[j], j) else 0
        out.append(cnt)
    return np.array(out, np.int64)
