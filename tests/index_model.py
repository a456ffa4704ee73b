"""The numpy model of the clustered item index (include/fmx.h: fmx_index_build, fmx_index_from_assign, fmx_topk_index), the
yardstick of tests/test_gpu_index.py: the contract's steps run literally.  As in tests/neighbors_model.py the projections come in as float64
arrays (exact widenings of the state type) and the score's fma chain as a function -- `chain_exact` for the Fraction emulation of the kernel's
chain, `chain_dot` where every chain is exact anyway.  The two fp64 chains of the index itself (the distance of the assign step and the coarse
score) run through `fma64`, an exact vectorised fma (Boldo and Melquiond's emulation by rounding to odd: finite values far from the ends of the
range; anything else falls back to a * b + c, which is the fma wherever an input is non-finite).  tests/test_index_cpu.py checks it against
Fractions and the model against a brute-force loop."""
import math

import numpy as np

from tests.diversify_model import QNAN, chain_dot, chain_exact  # noqa: F401  (re-exported for the tests)
from tests.neighbors_model import order
from tests.split_model import H

SEED_STREAM = 5
CHUNK = 1024
MAX_LISTS, MAX_ITER = 65536, 100
PLANTED_SEED = 27  # a seed of planted() whose seeds fall into distinct clusters


# ---------------------------------------------------------------------------------------------------------------- the exact fp64 fma

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """Dekker's product with Veltkamp's split: a * b = p + e exactly"""
    p = a * b
    c = 134217729.0  # 2^27 + 1
    t = c * a; ah = t - (t - a); al = a - ah
    t = c * b; bh = t - (t - b); bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_odd(a, b):
    """a + b rounded to odd: the truncated sum with its last bit set if the sum is inexact"""
    s, e = _two_sum(a, b)
    bits = s.view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s)


def fma64(a, b, c):
    """fma(a, b, c) in fp64, one rounding, elementwise on broadcast arrays"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    with np.errstate(all="ignore"):
        plain = a * b + c
        ok = np.isfinite(a) & np.isfinite(b) & np.isfinite(c) & (np.abs(a) < 2.0 ** 400) & (np.abs(b) < 2.0 ** 400) & (np.abs(c) < 2.0 ** 800)
        ok &= ((a == 0) | (np.abs(a) > 2.0 ** -400)) & ((b == 0) | (np.abs(b) > 2.0 ** -400))
        a1, b1, c1 = np.where(ok, a, 0.0), np.where(ok, b, 0.0), np.where(ok, c, 0.0)
        uh, ul = _two_prod(a1, b1)
        th, tl = _two_sum(c1, ul)
        vh, vl = _two_sum(uh, th)
        out = vh + _add_odd(np.ascontiguousarray(tl), np.ascontiguousarray(vl))
    return np.where(ok, out, plain)


# ---------------------------------------------------------------------------------------------------------------- the index

def augment(s, base):
    """a_i = (s_i, base_i): float64[n, k + 1]"""
    s = np.asarray(s, np.float64).reshape(len(base), -1)
    return np.ascontiguousarray(np.concatenate([s, np.asarray(base, np.float64).reshape(-1, 1)], axis=1))


def finite_items(a):
    return np.all(np.isfinite(a), axis=1)


def pair_hash(seed, epoch, t, stream):
    """fm_rank.h's counter hash (tests/split_model.py's H is the same chain)"""
    return H(seed, epoch, t, stream)


def seed_order(a, seed):
    """the finite items in the order of (pair_hash(seed, 0, i, 5), i)"""
    ids = np.nonzero(finite_items(a))[0]
    key = pair_hash(seed, 0, ids, SEED_STREAM)
    return ids[np.lexsort((ids, key))]


def distances(a, mu):
    """d(i, l) float64[n, n_lists]: acc = 0; for f ascending: t = a_i[f] - mu_l[f]; acc = fma(t, t, acc)"""
    acc = np.zeros((len(a), len(mu)))
    with np.errstate(all="ignore"):
        for f in range(a.shape[1]):
            t = a[:, f][:, None] - mu[:, f][None, :]
            acc = fma64(t, t, acc)
    return acc


def assign(a, mu):
    """step 2: the first list whose distance is strictly below the best so far (+inf at the start), list 0 if none is or the item is not finite"""
    d = distances(a, mu)
    out = np.zeros(len(a), np.uint32)
    best = np.full(len(a), np.inf)
    for l in range(len(mu)):
        with np.errstate(all="ignore"):
            lower = d[:, l] < best
        out[lower] = l
        best[lower] = d[lower, l]
    out[~finite_items(a)] = 0
    return out


def lists(assign_, n_lists):
    """(list_ptr int64[n_lists + 1], list_item int32[n]): a stable sort by list"""
    assign_ = np.asarray(assign_, np.int64)
    item = np.argsort(assign_, kind="stable").astype(np.int32)
    ptr = np.searchsorted(assign_[item], np.arange(n_lists + 1)).astype(np.int64)
    return ptr, item


def ordered_sum(x):
    """the stated order over the terms x[position] (0.0 where a member is skipped): chunks of 1 024 positions; lane l adds positions l, l + 64,
    ... from +0.0; an xor butterfly over the 64 lanes (strides 32 .. 1); the chunk sums added ascending from +0.0"""
    total = 0.0
    lanes = np.arange(64)
    for c0 in range(0, len(x), CHUNK):
        part = np.zeros(CHUNK)
        part[: len(x[c0:c0 + CHUNK])] = x[c0:c0 + CHUNK]
        s = np.zeros(64)
        for row in part.reshape(CHUNK // 64, 64):
            s = s + row
        for st in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ st]
        total = total + s[0]
    return total


def update(a, mu, ptr, item):
    """step 3: the new centroids (a list without finite members keeps its bits)"""
    out = np.array(mu, np.float64, copy=True)
    fin = finite_items(a)
    for l in range(len(mu)):
        mem = item[ptr[l]:ptr[l + 1]]
        cnt = int(fin[mem].sum())
        if cnt == 0:
            continue
        for f in range(a.shape[1]):
            out[l, f] = ordered_sum(np.where(fin[mem], a[mem, f], 0.0)) / float(cnt)
    return out


def update_bars(a, mu, ptr, item):
    """the yardstick of one update step: (math.fsum means, bars cnt * 2^-53 * sum |term|, has-finite-member flags) per list and component"""
    fin = finite_items(a)
    mean, bar, live = np.array(mu, np.float64, copy=True), np.zeros(mu.shape), np.zeros(len(mu), bool)
    for l in range(len(mu)):
        mem = item[ptr[l]:ptr[l + 1]]
        mem = mem[fin[mem]]
        if not len(mem):
            continue
        live[l] = True
        for f in range(a.shape[1]):
            mean[l, f] = math.fsum(a[mem, f]) / len(mem)
            bar[l, f] = len(mem) * 2.0 ** -53 * math.fsum(np.abs(a[mem, f]))
    return mean, bar, live


def build(a, n_lists, n_iter, seed):
    """the whole build: (centroid float64[n_lists, k + 1], assign uint32[n], list_ptr, list_item)"""
    mu = a[seed_order(a, seed)[:n_lists]].copy()                                  # 1
    for _ in range(n_iter):                                                       # 4
        ptr, item = lists(assign(a, mu), n_lists)                                 # 2
        mu = update(a, mu, ptr, item)                                             # 3
    asg = assign(a, mu)
    ptr, item = lists(asg, n_lists)
    return mu, asg, ptr, item


def planted(n_cl=6, k=8, seed=PLANTED_SEED):
    """A planted problem: n_cl clusters of 12 .. 20 items along well-separated directions (4 e_cl plus eighths in [-1/2, 1/2], a base in eighths),
    three contexts aligned to every cluster.  Every value is a small multiple of 1/8, so every score chain is exact in either state type.  The
    top_k = 10 <= the smallest cluster of every context lie in its own cluster, and a build of n_cl lists from `seed` recovers the clusters --
    tests/test_index_cpu.py asserts both in the model: one probe then returns exactly the full ranking."""
    rng = np.random.default_rng(41)
    sizes = rng.integers(12, 21, n_cl)
    cluster = np.repeat(np.arange(n_cl), sizes)
    cluster = cluster[rng.permutation(len(cluster))]
    si = 4.0 * np.eye(k)[cluster] + rng.integers(-4, 5, (len(cluster), k)) / 8.0
    bi = rng.integers(-2, 3, len(cluster)) / 8.0
    ctx_cluster = np.repeat(np.arange(n_cl), 3)
    sc = 4.0 * np.eye(k)[ctx_cluster] + rng.integers(-2, 3, (len(ctx_cluster), k)) / 8.0
    bc = rng.integers(-2, 3, len(ctx_cluster)) / 8.0
    return {"si": si, "bi": bi, "sc": sc, "bc": bc, "cluster": cluster, "ctx_cluster": ctx_cluster, "n_lists": n_cl, "n_iter": 5, "seed": seed,
            "top_k": 10}


# ---------------------------------------------------------------------------------------------------------------- the search

def coarse(sc, mu):
    """g(c, l) float64[n_ctx, n_lists] = mu_l[k] + acc; acc = 0; for f ascending: acc = fma(s_c[f], mu_l[f], acc)"""
    k = mu.shape[1] - 1
    acc = np.zeros((len(sc), len(mu)))
    with np.errstate(all="ignore"):
        for f in range(k):
            acc = fma64(sc[:, f][:, None], mu[:, f][None, :], acc)
        return mu[:, k][None, :] + acc


def probe_set(g_row, ptr, n_probe):
    """P_c: the first min(n_probe, non_empty) non-empty lists under the order on (g, l)"""
    non_empty = np.nonzero(np.diff(ptr) > 0)[0]
    return order(g_row, non_empty)[:n_probe]


def pair_scores(sc, bc, si, bi, chain):
    """fmx_topk's raw score of every (context, item) pair: (base_c + base_i) + the chain, float64[n_ctx, n_items]"""
    out = np.zeros((len(sc), len(si)))
    with np.errstate(all="ignore"):
        for c in range(len(sc)):
            if len(si):
                out[c] = (bc[c] + bi) + np.asarray(chain(si, sc[c]), np.float64).reshape(len(si))
    return out


def select(score_row, eligible, top_k):
    o = order(score_row, eligible)[:top_k]
    oi, os_ = np.full(top_k, -1, np.int64), np.full(top_k, QNAN)
    oi[: len(o)], os_[: len(o)] = o, score_row[o]
    return oi, os_


def search_scores(score, g, ptr, item, top_k, n_probe, exclude=None):
    """steps 2-4 on the pair scores [n_ctx, n_items] and the coarse scores [n_ctx, n_lists]: (index, score, scanned)"""
    nc = len(score)
    oi, os_, scanned = np.full((nc, top_k), -1, np.int64), np.full((nc, top_k), QNAN), np.zeros(nc, np.int64)
    for c in range(nc):
        probed = probe_set(g[c], ptr, n_probe)
        cand = np.concatenate([item[ptr[l]:ptr[l + 1]] for l in probed]).astype(np.int64) if len(probed) else np.zeros(0, np.int64)
        scanned[c] = len(cand)
        if exclude is not None:
            cand = cand[~np.isin(cand, np.asarray(exclude[c], np.int64))]
        oi[c], os_[c] = select(score[c], cand, top_k)
    return oi, os_, scanned


def search(sc, bc, si, bi, mu, ptr, item, top_k, n_probe, chain, exclude=None):
    """the whole call (link NONE)"""
    return search_scores(pair_scores(sc, bc, si, bi, chain), coarse(sc, mu), ptr, item, top_k, n_probe, exclude)


def full_ranking(score, top_k, exclude=None):
    """fmx_topk on the same pair scores"""
    nc, ni = score.shape
    oi, os_ = np.full((nc, top_k), -1, np.int64), np.full((nc, top_k), QNAN)
    for c in range(nc):
        cand = np.arange(ni)
        if exclude is not None:
            cand = cand[~np.isin(cand, np.asarray(exclude[c], np.int64))]
        oi[c], os_[c] = select(score[c], cand, top_k)
    return oi, os_
