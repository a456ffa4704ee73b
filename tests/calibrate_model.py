"""The numpy definition of the calibration calls (include/fmx.h: fmx_predict_calibrated, fmx_reliability, fmx_calibrate_platt,
fmx_calibrate_isotonic).  Fed with the device's own z (raw scores) and, for the uncalibrated map, its own p, as tests/metrics_model.py is: integers
are Python ints, sums are math.fsum (with each sum's sum of |term|, the scale of the summation bound), ECE and MCE are the literal operation
sequence, the Platt fit runs in any float type and any summation order."""
import math

import numpy as np

from tests.metrics_model import bits, order_key  # noqa: F401  (order_key: ascending in z, -0 == +0, NaN = 0)

NAN = float("nan")
BINS_WIDTH, BINS_MASS = 0, 1


def bits_key(z):
    """uint64, a total order on the bits of numbers: -0 below +0 (what lo_z / hi_z are the minimum / maximum of)"""
    u = np.ascontiguousarray(z, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def apply_map(cal, z, group=None, p_link=None):
    """p per row.  cal: None / {"kind": "none"} (p_link, the device's own link(z)), {"kind": "platt", "ab"}, {"kind": "steps", "n_steps", "thr",
    "val"}; a map with one row applies to every row, else row r takes the map of group[r]."""
    z = np.asarray(z, np.float64)
    n = len(z)
    if cal is None or cal["kind"] == "none":
        out = np.array(p_link, np.float64)
    elif cal["kind"] == "platt":
        ab = np.asarray(cal["ab"], np.float64).reshape(-1, 2)
        g = np.zeros(n, np.int64) if len(ab) == 1 else np.asarray(group, np.int64)
        with np.errstate(all="ignore"):
            t = ab[g, 0] * z + ab[g, 1]      # two rounded operations
            out = 1.0 / (1.0 + np.exp(-t))
        out[np.isnan(ab[g, 0]) | np.isnan(ab[g, 1])] = NAN
    else:
        ns = np.asarray(cal["n_steps"]).ravel()
        thr = np.asarray(cal["thr"], np.float64).reshape(len(ns), -1)
        val = np.asarray(cal["val"], np.float64).reshape(len(ns), -1)
        g = np.zeros(n, np.int64) if len(ns) == 1 else np.asarray(group, np.int64)
        out = np.full(n, NAN)
        kz = order_key(z)
        for r in range(n):
            k = order_key(thr[g[r], :ns[g[r]]])
            s = int(np.searchsorted(k, kz[r], "right"))   # the first step above z
            if s > 0:
                out[r] = val[g[r], s - 1]
    out[np.isnan(z)] = NAN
    return out


def width_bins(p, B):
    """bin per row of one group's valid rows"""
    with np.errstate(all="ignore"):
        t = np.floor(np.asarray(p, np.float64) * float(B))
    return np.where(~(t >= 0), 0, np.where(~(t < B), B - 1, np.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0))).astype(np.int64)


def mass_bins(z, B):
    """bin per row of one group's valid rows (in the order given: ties of the key go by position, which does not move a bin)"""
    k = order_key(z)
    s = len(k)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    head = np.searchsorted(ks, ks, "left")          # the first position of every row's run
    out = np.empty(s, np.int64)
    out[order] = [int(h) * B // s for h in head]    # exact integers
    return out


def _fsum(terms):
    t = [float(x) for x in terms]
    if any(math.isnan(x) for x in t) or (math.inf in t and -math.inf in t):
        return NAN, NAN
    return math.fsum(t), math.fsum(abs(x) for x in t)


def ece_mce(count, sum_p):
    """one group's (ECE, MCE) from its table: count [B][2] ints, sum_p [B] floats; the literal sequence of rounded operations"""
    s = sum(int(c[0]) for c in count)
    if s == 0:
        return NAN, NAN
    ece, mce = 0.0, 0.0
    for (rows, pos), sp in zip(count, sum_p):
        rows, pos = int(rows), int(pos)
        if rows == 0:
            continue
        with np.errstate(all="ignore"):
            gap = float(abs(np.float64(sp) / np.float64(rows) - np.float64(pos) / np.float64(rows)))
            ece = float(np.float64(ece) + (np.float64(rows) / np.float64(s)) * np.float64(gap))
        mce = gap if gap > mce else mce
    return ece, mce


def table(z, p, y, group, G, B, binning):
    """every group's table: {"count": int list [G][B][2], "sum_p", "sum_p_abs": float64[G, B] (fsum and sum |term|), "lo_z", "hi_z": float64[G, B],
    "nan_rows": int list [G], "bin": int64[n] (-1: in no bin), "brier", "logloss": [G] of (mean, sum |term|), "s": int list [G]}"""
    z, p, y = np.asarray(z, np.float64), np.asarray(p, np.float64), np.asarray(y, np.float64)
    n = len(z)
    g = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    out = {"count": [[[0, 0] for _ in range(B)] for _ in range(G)], "sum_p": np.zeros((G, B)), "sum_p_abs": np.zeros((G, B)), "lo_z": np.full((G, B), NAN),
           "hi_z": np.full((G, B), NAN), "nan_rows": [0] * G, "bin": np.full(n, -1, np.int64), "brier": [(NAN, NAN)] * G, "logloss": [(NAN, NAN)] * G, "s": [0] * G}
    for q in range(G):
        rows = np.nonzero(g == q)[0]
        valid = rows[~np.isnan(p[rows])]
        out["nan_rows"][q] = int(len(rows) - len(valid))
        out["s"][q] = s = int(len(valid))
        if s == 0:
            continue
        b = width_bins(p[valid], B) if binning == BINS_WIDTH else mass_bins(z[valid], B)
        out["bin"][valid] = b
        pos = y[valid] > 0
        for j in range(B):
            sel = valid[b == j]
            if len(sel) == 0:
                continue
            out["count"][q][j] = [int(len(sel)), int((y[sel] > 0).sum())]
            out["sum_p"][q, j], out["sum_p_abs"][q, j] = _fsum(p[sel])
            k = bits_key(z[sel])
            out["lo_z"][q, j], out["hi_z"][q, j] = z[sel][np.argmin(k)], z[sel][np.argmax(k)]
        with np.errstate(all="ignore"):
            d = p[valid] - pos.astype(np.float64)
            ll = -np.log(np.where(pos, p[valid], 1.0 - p[valid]))
        for name, terms in (("brier", d * d), ("logloss", ll)):
            t, a = _fsum(terms)
            out[name][q] = (t / float(s), a)
    return out


def pav(count, lo_z):
    """one group's isotonic steps from its MASS table: (n_steps, thr float64[B], val float64[B]); integer arithmetic, equal pools too"""
    B = len(count)
    blocks = []   # [pos, rows, thr]
    for b in range(B):
        rows, pos = int(count[b][0]), int(count[b][1])
        if rows == 0:
            continue
        t0 = float(lo_z[b])
        while blocks and blocks[-1][0] * rows >= pos * blocks[-1][1]:
            ppos, prow, pt = blocks.pop()
            pos, rows, t0 = pos + ppos, rows + prow, pt
        blocks.append([pos, rows, t0])
    thr, val = np.full(B, NAN), np.full(B, NAN)
    for t, (pos, rows, t0) in enumerate(blocks):
        thr[t] = -math.inf if t == 0 else t0
        val[t] = float(pos) / float(rows)
    return len(blocks), thr, val


def platt(z, y, lam, steps, dtype=np.longdouble, order=None):
    """one group's (a, b, rows, status) by `steps` undamped Newton steps from (1, 0) in `dtype`; the rows with a finite z take part, summed in the
    order `order` (a permutation of the participating rows; None: as given)"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    keep = np.isfinite(z)
    z, y = z[keep], y[keep]
    if order is not None:
        z, y = z[order], y[order]
    T = dtype
    zz, yy = z.astype(T), np.where(y > 0, T(1), T(-1)).astype(T)
    lam = T(lam)
    a, b = T(1), T(0)

    def tot(x):   # left to right
        return np.cumsum(x, dtype=T)[-1] if len(x) else T(0)
    status = 0
    with np.errstate(all="ignore"):
        for _ in range(steps):
            m = yy * (a * zz + b)
            sg, ng = T(1) / (T(1) + np.exp(-m)), T(1) / (T(1) + np.exp(m))
            w, d = sg * ng, -yy * ng
            g0, g1 = tot(d * zz) + lam * (a - T(1)), tot(d) + lam * b
            h00, h01, h11 = tot(w * zz * zz) + lam, tot(w * zz), tot(w) + lam
            if not (h00 > 0 and np.isfinite(h00)):
                status = 1
                break
            l00 = np.sqrt(h00)
            l10 = h01 / l00
            d1 = h11 - l10 * l10
            if not (d1 > 0 and np.isfinite(d1)):
                status = 1
                break
            l11 = np.sqrt(d1)
            y0 = -g0 / l00
            y1 = (-g1 - l10 * y0) / l11
            x1 = y1 / l11
            x0 = (y0 - l10 * x1) / l00
            a, b = a + x0, b + x1
    if status:
        return NAN, NAN, int(len(z)), 1
    return a, b, int(len(z)), 0


def planted(rng, n=5000):
    """z = 2 z_true + 1 with labels Bernoulli(sigma(z_true)): a model that is twice too sure and shifted.  Returns (z, y in {-1, 1})."""
    zt = rng.normal(0, 1.0, n)
    y = np.where(rng.random(n) < 1.0 / (1.0 + np.exp(-zt)), 1.0, -1.0)
    return 2.0 * zt + 1.0, y


def platt_cases():
    """the Platt cases of the CPU and the GPU tests: (name, w float64[p], cols int[n], y in {-1, 1}[n], lambda); row r is the one-hot row of column
    cols[r], so with zero factors and no w0 its score is w[cols[r]].  At least two distinct finite scores each; both classes wherever lambda is 0,
    and there the lowest and the highest score hold both classes (the optimum exists)."""
    rng = np.random.default_rng(2024)
    out = []
    for n, distinct in ( (64, 9), (65, 63), (1025, 40), (5000, 4998)):
        zt = rng.normal(0, 1.5 if n > 1000 else 0.4, distinct)   # (few rows: mild scores, or the undamped steps run away)
        cols = np.concatenate([np.arange(distinct), rng.integers(0, distinct, n - distinct)])
        y = np.where(rng.random(n) < 1.0 / (1.0 + np.exp(-zt[cols])), 1.0, -1.0)
        lo, hi = int(np.argmin(zt)), int(np.argmax(zt))
        if n >= distinct + 2:   # the lowest and the highest score hold both classes: the unpenalised optimum exists
            cols[n - 2], cols[n - 1] = lo, hi
            y[lo], y[n - 2], y[hi], y[n - 1] = -1.0, 1.0, 1.0, -1.0
        w = 2.0 * zt + 1.0
        order = rng.permutation(n)
        for lam in ((0.0, 0.1) if n >= distinct + 2 else (0.1,)):
            out.append((f"n{n}_lam{lam}", w, cols[order], y[order], lam))
    out.append(("n3_lam0.1", np.array([-0.5, 1.0]), np.array([0, 1, 1]), np.array([-1.0, 1.0, -1.0]), 0.1))
    for lam in (0.0, 0.1):
        out.append((f"n5_lam{lam}", np.array([-1.0, 0.5, 2.0]), np.array([2, 0, 1, 0, 2]), np.array([1.0, -1.0, 1.0, 1.0, -1.0]), lam))
    w = np.array([-1.0, 0.25, 3.0])
    out.append(("one_class_lam0.1", w, np.array([0, 1, 2, 1, 0, 2, 2, 1]), np.ones(8), 0.1))
    return out
