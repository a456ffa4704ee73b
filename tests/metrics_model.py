"""The numpy definition of fmx_metrics (include/fmx.h): per row group the integer counts (Python ints), the six values with every sum taken by
math.fsum, and each sum's sum of |term| (the scale of the summation bound).  Fed with z (the raw scores) and p (the linked predictions)."""
import math

import numpy as np

LINK_NONE, LINK_LOGISTIC, LINK_CLAMP, LINK_PROBIT = 0, 1, 2, 3
CLS_NAMES = ("auc", "logloss", "accuracy", "brier", "mean_pred", "mean_label")
REG_NAMES = ("mse", "rmse", "mae", "mean_err", "mean_pred", "mean_label")
NAN = float("nan")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def order_key(z):
    """uint64, ascending in z: -0 and +0 share a key, every NaN has key 0, below every number"""
    z = np.array(z, np.float64)
    z[z == 0] = 0.0
    u = z.view(np.uint64)
    key = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    key[np.isnan(z)] = 0
    return key


def pairs2(z, pos):
    """sum over (positive i, negative j) of 2 [z_i > z_j] + [z_i == z_j], by sorting the negatives' keys"""
    k = order_key(z)
    kn = np.sort(k[~pos])
    lt = np.searchsorted(kn, k[pos], "left")
    le = np.searchsorted(kn, k[pos], "right")
    return 2 * int(lt.sum()) + int((le - lt).sum())


def auc_from(p2, P, N):
    return float(p2) / float(2 * P * N) if P and N else NAN   # both integers rounded to nearest, one division


def _mean(terms):
    """(fsum / rows, sum |term|)"""
    t = [float(x) for x in terms]
    if any(math.isnan(x) for x in t) or (math.inf in t and -math.inf in t):
        return NAN, NAN
    return math.fsum(t) / float(len(t)), math.fsum(abs(x) for x in t)


def group(z, p, y, classification, link):
    """one group's rows: {"count": [rows, positives, pairs2, correct], "value": [6 floats], "abs": [6 floats, sum |term| of the summed columns]}"""
    z, p, y = np.asarray(z, np.float64), np.asarray(p, np.float64), np.asarray(y, np.float64)
    n = len(z)
    if n == 0:
        return {"count": [0, 0, 0, 0], "value": [NAN] * 6, "abs": [NAN] * 6}
    with np.errstate(all="ignore"):
        if classification:
            pos = y > 0
            P = int(pos.sum())
            p2 = pairs2(z, pos)
            correct = int(np.sum(~np.isnan(p) & ((p >= 0.5) == pos)))
            if link == LINK_LOGISTIC:
                t = np.where(pos, z, -z)
                ll = np.maximum(-t, 0.0) + np.log1p(np.exp(-np.abs(t)))
            else:
                ll = -np.log(np.where(pos, p, 1.0 - p))
            d = p - pos.astype(np.float64)
            cols = [None, _mean(ll), None, _mean(d * d), _mean(p), None]
            value = [auc_from(p2, P, n - P), cols[1][0], float(correct) / float(n), cols[3][0], cols[4][0], float(P) / float(n)]
            count = [n, P, p2, correct]
        else:
            d = p - y
            cols = [_mean(d * d), None, _mean(np.abs(d)), _mean(d), _mean(p), _mean(y)]
            value = [cols[0][0], NAN, cols[2][0], cols[3][0], cols[4][0], cols[5][0]]   # RMSE is held to the sqrt of the RETURNED MSE
            count = [n, 0, 0, 0]
    return {"count": count, "value": value, "abs": [c[1] if c else NAN for c in cols]}


def metrics(z, p, y, groups, n_groups, classification, link):
    """every group: (count list[G] of 4 ints, value float64[G, 6], abs float64[G, 6]); groups None = one group; an id >= n_groups is in no group"""
    z, p, y = np.asarray(z, np.float64), np.asarray(p, np.float64), np.asarray(y, np.float64)
    g = np.zeros(len(z), np.int64) if groups is None else np.asarray(groups, np.int64)
    order = np.argsort(g, kind="stable")
    lo = np.searchsorted(g[order], np.arange(n_groups), "left")
    hi = np.searchsorted(g[order], np.arange(n_groups), "right")
    out = [group(z[order[a:b]], p[order[a:b]], y[order[a:b]], classification, link) for a, b in zip(lo, hi)]
    return [o["count"] for o in out], np.array([o["value"] for o in out]).reshape(n_groups, 6), np.array([o["abs"] for o in out]).reshape(n_groups, 6)


def rank_sum_auc(score, pos):
    """the textbook AUC from average ranks (NaN-free scores): (R_pos - P (P + 1) / 2) / (P N)"""
    from scipy.stats import rankdata
    r = rankdata(score)
    P = int(pos.sum())
    return (r[pos].sum() - P * (P + 1) / 2) / (P * (len(score) - P))


def planted_gauc(rng, users=40, per_user=30):
    """scores that are a user offset plus nothing else: inside a user every score ties (AUC 1/2), while across users the offset follows the
    user's positive rate, so the pooled AUC is high.  Returns (z, y in {-1, 1}, user id per row)."""
    rate = np.linspace(0.05, 0.95, users)
    user = np.repeat(np.arange(users), per_user)
    y = np.where(rng.random(users * per_user) < rate[user], 1.0, -1.0)
    for u in range(users):   # both classes in every user
        y[u * per_user], y[u * per_user + 1] = 1.0, -1.0
    return 4.0 * (rate[user] - 0.5), y, user
