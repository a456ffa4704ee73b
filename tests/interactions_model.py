"""The definition of fmx_interactions* (include/fmx.h) in numpy, to the bit: the pair values as ONE fp64 chain per pair, the order of a row's
pairs, the top_m table, and the group summary with exact (math.fsum) sums.  `v` is the factor table [k][p] as the engine stores it
(get_params: fp32 tables come back widened, so the products below are the kernel's)."""
import math

import numpy as np

NAN = np.float64(np.nan)   # the canonical quiet NaN, 0x7ff8000000000000


def pair_values(v, cols, vals):
    """(a int64[P], b int64[P], I float64[P]) of one row, every pair a < b in (a, b) order"""
    m = len(cols)
    k = v.shape[0]
    t = v.T[np.asarray(cols, np.int64)].astype(np.float64) * np.asarray(vals, np.float32).astype(np.float64)[:, None]   # one rounded product each
    a, b = np.triu_indices(m, 1)
    acc = np.zeros(len(a))
    with np.errstate(all="ignore"):
        for f in range(k):   # the chain: the product is rounded, then the sum
            prod = t[a, f] * t[b, f]
            acc = acc + prod
    return a.astype(np.int64), b.astype(np.int64), np.where(np.isnan(acc), NAN, acc)


def order(a, b, val):
    """the permutation that puts a row's pairs strongest first: larger |I| (NaN last), then the lower a, then the lower b"""
    mag = np.abs(val)
    nan = np.isnan(mag)
    key = np.where(nan, 0.0, -mag)   # -|I|: -0.0 and +0.0 compare equal
    return np.lexsort((b, a, key, nan))


def top_m(v, rp, col, val, m_top):
    """(a, b, value) [n][m_top] as fmx_interactions returns them"""
    n = len(rp) - 1
    oa = np.full((n, m_top), -1, np.int64)
    ob = np.full((n, m_top), -1, np.int64)
    ov = np.full((n, m_top), NAN)
    for r in range(n):
        a, b, I = pair_values(v, col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]])
        o = order(a, b, I)[:m_top]
        oa[r, :len(o)], ob[r, :len(o)], ov[r, :len(o)] = a[o], b[o], I[o]
    return oa, ob, ov


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def summary(v, rp, col, val, groups, G):
    """{"sum", "abs_sum" float64[G][G], "count" int64[G][G]}: the exactly rounded sums of the model's pair values per group cell"""
    cellv = [[[] for _ in range(G)] for _ in range(G)]
    groups = np.arange(v.shape[1]) if groups is None else np.asarray(groups, np.int64)
    for r in range(len(rp) - 1):
        c = np.asarray(col[rp[r]:rp[r + 1]], np.int64)
        a, b, I = pair_values(v, c, val[rp[r]:rp[r + 1]])
        ga, gb = groups[c[a]], groups[c[b]]
        for g, h, x in zip(ga, gb, I):
            cellv[g][h].append(x)
            if g != h:
                cellv[h][g].append(x)
    out = {"sum": np.zeros((G, G)), "abs_sum": np.zeros((G, G)), "count": np.zeros((G, G), np.int64)}
    for g in range(G):
        for h in range(G):
            out["sum"][g, h] = math.fsum(cellv[g][h])
            out["abs_sum"][g, h] = math.fsum(abs(x) for x in cellv[g][h])
            out["count"][g, h] = len(cellv[g][h])
    return out


def brute_pairs(v, cols, vals):
    """the same values by a plain double loop over Python floats (the check of pair_values)"""
    k = v.shape[0]
    out = []
    for a in range(len(cols)):
        for b in range(a + 1, len(cols)):
            acc = 0.0
            for f in range(k):
                ta = float(v[f, cols[a]]) * float(np.float32(vals[a]))
                tb = float(v[f, cols[b]]) * float(np.float32(vals[b]))
                acc = acc + ta * tb
            out.append((a, b, acc))
    return out


def planted(rng, n=300, fields=6, vocab=5, k=4):
    """one-hot rows over `fields` fields; the factor rows are small noise, except that fields 1 and 4 share the direction of factor 0"""
    p = fields * vocab
    groups = np.repeat(np.arange(fields), vocab).astype(np.uint32)
    v = rng.normal(0, 0.01, (k, p))
    shared = (groups == 1) | (groups == 4)
    v[0, shared] = rng.choice([-1.0, 1.0], int(shared.sum())) * rng.uniform(0.8, 1.2, int(shared.sum()))
    v = v.astype(np.float32).astype(np.float64)
    col = (np.arange(fields)[None, :] * vocab + rng.integers(0, vocab, (n, fields))).astype(np.uint32).ravel()
    rp = (np.arange(n + 1) * fields).astype(np.int64)
    return p, groups, v, rp, col, np.ones(len(col), np.float32)
