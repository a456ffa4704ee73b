"""The numpy model of fmx_diversify (include/fmx.h), the yardstick of tests/test_gpu_diversify.py: greedy maximal marginal
relevance over one context's pool, steps 1 to 8 of the contract run literally.  The projections come in as float64 arrays (exact widenings of
the state type) and the fma chain as a function, so that the same model serves fp32 and fp64 engines: `chain_exact` for the Fraction emulation
of the kernel's chain, `chain_dot` where every chain is exact anyway.  tests/test_diversify_cpu.py checks it against a brute-force restatement."""
from fractions import Fraction

import numpy as np

REL_SCORE, REL_MINMAX = 0, 1
QNAN = np.array([0x7FF8000000000000], np.uint64).view(np.float64)[0]


def _round_to(x, dt):
    """the Fraction x rounded to the nearest value of the float type dt, ties to even"""
    if dt == np.float64:
        return np.float64(float(x))   # int / int true division: correctly rounded
    f = np.float32(float(x))
    cands = {np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))}
    return min(cands, key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))


def _chain(sa, sb, dt):
    """fma(sa[k-1], sb[k-1], ... fma(sa[0], sb[0], 0)) with one rounding to dt per step"""
    acc = Fraction(0)
    for a, b in zip(sa, sb):
        acc = Fraction(float(_round_to(Fraction(float(a)) * Fraction(float(b)) + acc, dt)))
    return np.float64(float(acc))


def chain_exact(dt):
    """chain(rows [m, k], v [k]) -> float64[m]: the kernel's chain in the state type dt, emulated with Fractions (finite values only)"""
    def chain(rows, v):
        return np.array([_chain(r, v, dt) for r in rows], np.float64).reshape(len(rows))
    return chain


def chain_dot(rows, v):
    """the chain where every partial sum is exact in the state type (small multiples of a power of two): a plain float64 dot product"""
    return np.asarray(rows, np.float64) @ np.asarray(v, np.float64) if len(v) else np.zeros(len(rows))


def norms_inv(s, chain):
    """step 3 for the rows of s: inv = 1 / sqrt(d(i, i)) if that is finite and > 0, else 0"""
    nrm = np.array([chain(s[i:i + 1], s[i])[0] for i in range(len(s))], np.float64).reshape(len(s))
    ok = np.isfinite(nrm) & (nrm > 0)
    with np.errstate(all="ignore"):
        return np.where(ok, 1.0 / np.sqrt(np.where(ok, nrm, 1.0)), 0.0)


def relevance(score, live, mode):
    """step 5 for one pool: score float64[P], live bool[P] (the non-empty slots)"""
    score = np.asarray(score, np.float64)
    if mode == REL_SCORE:
        return score.copy()
    s = score[live & ~np.isnan(score)]
    out = np.where(np.isnan(score), score, 0.0)
    if len(s):
        hi, lo = s.max(), s.min()
        hi = 0.0 if hi == 0 else hi   # a zero bound is +0
        lo = 0.0 if lo == 0 else lo
        if np.isfinite(hi) and np.isfinite(lo) and hi > lo:
            with np.errstate(all="ignore"):
                out = (score - lo) / (hi - lo)
    return out


def first(margin, item, slots):
    """the first of `slots` under the order: a higher margin first (-0 = +0), NaN below every number, then the lower item, then the lower slot"""
    m = margin[slots]
    nan = np.isnan(m)
    o = np.lexsort((slots, item[slots], np.where(nan, 0.0, -m), nan))   # keys last to first
    return int(slots[o[0]])


def diversify(s, index, score, top_k, lam, mode, chain, inv=None):
    """one context's pool -> (index int64[top_k], score float64[top_k], margin float64[top_k]).  s: float64[n_items, k], the items' projections;
    index int64[P], score float64[P]; inv: norms_inv(s, chain) if the caller has it already"""
    index = np.asarray(index, np.int64)
    score = np.asarray(score, np.float64)
    P, ni = len(index), len(s)
    live = (index >= 0) & (index < ni)                                   # 1
    item = np.where(live, index, 0)
    if inv is None:
        inv = np.zeros(ni)
        used = np.unique(item[live])
        inv[used] = norms_inv(s[used], chain)                            # 2, 3
    inv_u = np.where(live, inv[item], 0.0)
    rel = relevance(score, live, mode)                                   # 5
    lam = np.float64(lam)
    mu = np.float64(1.0) - lam                                           # 6
    pen = np.zeros(P)
    left = live.copy()
    oi, os_, om = np.full(top_k, -1, np.int64), np.full(top_k, QNAN), np.full(top_k, QNAN)
    for t in range(top_k):                                               # 7
        slots = np.nonzero(left)[0]
        if not len(slots):
            break
        with np.errstate(all="ignore"):
            margin = lam * rel - mu * pen
        margin = np.where(np.isnan(margin), QNAN, margin)
        v = first(margin, item, slots)
        oi[t], os_[t], om[t] = item[v], score[v], margin[v]              # 8
        left[v] = False
        if t + 1 == top_k:
            break
        sim = np.zeros(P)
        todo = np.nonzero(left & (inv_u != 0) & (inv_u[v] != 0))[0]
        if len(todo):
            d = chain(s[item[todo]], s[item[v]])                         # 2
            with np.errstate(all="ignore"):
                sim[todo] = (d * inv_u[todo]) * inv_u[v]                 # 4
        pen = sim if t == 0 else np.where(sim > pen, sim, pen)
    return oi, os_, om


def diversify_rows(s, index, score, top_k, lam, mode, chain, inv=None):
    """every row of index / score [n, P]: ([n, top_k] index, score, margin)"""
    out = [diversify(s, i, sc, top_k, lam, mode, chain, inv) for i, sc in zip(index, score)]
    return tuple(np.array([o[q] for o in out]).reshape(len(out), top_k) for q in range(3))
