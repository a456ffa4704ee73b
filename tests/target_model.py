"""The numpy restatement of the target-encoding calls (include/fmx.h: fmx_target_stats, fmx_matrix_encode_targets).  It is the
definition: the counts are integers, the kept entries copied bits, every floating-point sum has one stated order (tests/columns_model.py: tree_sum)
and every value is a fixed chain of IEEE operations, so the device's outputs are compared with these by exact equality of bits."""
import numpy as np

from tests.columns_model import tree_sum

MAX_SEGMENTS = 4096
MAX_TERMS = 64
MAX_PARTS = 64
POSITIVE, LABEL = 0, 1
MEAN, COUNT = 1, 2
NAN32 = 0x7FC00000
NAN64 = 0x7FF8000000000000
MAX_WIDTH = 2**32 - 2
MAX_CELLS = 2**31 - 1


def canon64(x):
    """every NaN of a float64 array as 0x7FF8000000000000"""
    x = np.array(x, np.float64)
    b = x.view(np.uint64)
    b[np.isnan(x)] = NAN64
    return x


def layout(p, segment_base, term_segment, n_parts=1, target=POSITIVE):
    """(lo, hi, term_base) as int64 arrays: term t covers the columns [lo[t], hi[t]) and the slots [term_base[t], term_base[t + 1]).  Raises
    ValueError where the calls refuse."""
    base = np.asarray(segment_base).astype(np.int64)
    seg = np.asarray(term_segment).astype(np.int64)
    n_seg = len(base) - 1
    if not 1 <= n_seg <= MAX_SEGMENTS or not 1 <= len(seg) <= MAX_TERMS or not 1 <= n_parts <= MAX_PARTS:
        raise ValueError("n_segments, n_terms or n_parts out of range")
    if base[0] != 0 or base[-1] != p or np.any(np.diff(base) < 0):
        raise ValueError("segment_base must ascend from 0 to p")
    if np.any(seg < 0) or np.any(seg >= n_seg) or np.any(np.diff(seg) <= 0):
        raise ValueError("term_segment must ascend strictly inside 0 .. n_segments - 1")
    if target not in (POSITIVE, LABEL):
        raise ValueError("unknown target")
    lo, hi = base[seg], base[seg + 1]
    term_base = np.concatenate([[0], np.cumsum(hi - lo)]).astype(np.int64)
    if int(term_base[-1]) * n_parts > MAX_CELLS:
        raise ValueError("W * n_parts is above 2^31 - 1")
    return lo, hi, term_base


def entry_slots(col, lo, hi, term_base):
    """(term, slot) of every entry, -1 for an entry outside every encoded segment"""
    col = np.asarray(col).astype(np.int64)
    t = np.searchsorted(lo, col, side="right") - 1                     # the last term with lo <= c: an empty one is never hit inside its range
    inside = (t >= 0) & (col < hi[np.maximum(t, 0)])
    term = np.where(inside, t, -1)
    slot = np.where(inside, term_base[np.maximum(t, 0)] + col - lo[np.maximum(t, 0)], -1)
    return term, slot


def target_stats(rp, col, y, p, segment_base, term_segment, n_parts=1, target=POSITIVE, part=None):
    """(count int64[W][n_parts][2] = rows, positive rows; sum float64[W][n_parts], or None under POSITIVE)"""
    if y is None:
        raise ValueError("the matrix has no labels")
    rp = np.asarray(rp, np.int64)
    y = np.asarray(y, np.float32)
    lo, hi, term_base = layout(p, segment_base, term_segment, n_parts, target)
    W, P, n = int(term_base[-1]), int(n_parts), len(rp) - 1
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    _, slot = entry_slots(col, lo, hi, term_base)
    f = np.zeros(n, np.int64) if part is None else np.asarray(part).astype(np.int64)
    ok = (slot >= 0) & (f[row] < P)
    count = np.zeros((W * P, 2), np.int64)
    total = np.zeros(W * P, np.float64) if target == LABEL else None
    if np.any(ok):
        key = slot[ok] * P + f[row[ok]]
        pairs = np.unique(key * max(n, 1) + row[ok])                   # (cell, row) once each, rows ascending inside a cell
        cell, r = pairs // max(n, 1), pairs % max(n, 1)
        count[:, 0] = np.bincount(cell, minlength=W * P)
        count[:, 1] = np.bincount(cell[y[r] > 0], minlength=W * P)
        if target == LABEL:
            off = np.searchsorted(cell, np.arange(W * P + 1))
            for k in np.flatnonzero(count[:, 0]):
                with np.errstate(all="ignore"):
                    total[k] = tree_sum(y[r[off[k]:off[k + 1]]].astype(np.float64))
            total = canon64(total)
    return count.reshape(W, P, 2), None if total is None else total.reshape(W, P)


def totals(count, total):
    """(N int64[W], A int64[W], T float64[W] or None): the sums over the parts; T is the chain from +0.0, parts ascending, a NaN canonical"""
    count = np.asarray(count, np.int64)
    with np.errstate(over="ignore"):
        N, A = count[:, :, 0].sum(axis=1), count[:, :, 1].sum(axis=1)
    T = None
    if total is not None:
        T = np.zeros(count.shape[0], np.float64)
        with np.errstate(all="ignore"):
            for g in range(count.shape[1]):
                T = T + np.asarray(total, np.float64)[:, g]
        T = canon64(T)
    return N, A, T


def encode_values(rp, col, p, segment_base, term_segment, count, total, target, part, prior, strength):
    """(present bool[rows][terms], n int64[rows][terms], mean bits uint32[rows][terms], count bits uint32[rows][terms])"""
    rp = np.asarray(rp, np.int64)
    count = np.asarray(count, np.int64)
    P = count.shape[1]
    lo, hi, term_base = layout(p, segment_base, term_segment, P, target)
    n_rows, n_terms = len(rp) - 1, len(lo)
    row = np.repeat(np.arange(n_rows, dtype=np.int64), np.diff(rp))
    term, slot = entry_slots(col, lo, hi, term_base)
    ok = term >= 0
    row, term, slot = row[ok], term[ok], slot[ok]                      # source order is kept
    N, A, T = totals(count, total if target == LABEL else None)
    if part is None:
        own = np.zeros(len(row), bool)
        f = np.zeros(len(row), np.int64)
    else:
        f = np.asarray(part).astype(np.int64)[row]
        own = f < P
        f = np.where(own, f, 0)
    with np.errstate(all="ignore"):
        dn = N[slot] - np.where(own, count[slot, f, 0], 0)
        da = A[slot] - np.where(own, count[slot, f, 1], 0)
        n = np.zeros((n_rows, n_terms), np.int64)
        np.add.at(n, (row, term), dn)
        seen = np.zeros((n_rows, n_terms), np.int64)
        np.add.at(seen, (row, term), 1)
        if target == POSITIVE:
            ai = np.zeros((n_rows, n_terms), np.int64)
            np.add.at(ai, (row, term), da)
            a = ai.astype(np.float64)
        else:
            tot = np.asarray(total, np.float64)
            x = np.where(own, T[slot] - tot[slot, f], T[slot])
            a = np.zeros((n_rows, n_terms), np.float64)
            group = row * n_terms + term
            order = np.argsort(group, kind="stable")
            g = group[order]
            first = np.searchsorted(g, g, side="left")
            rank = np.arange(len(g)) - first
            for k in range(int(rank.max()) + 1 if len(g) else 0):      # the k-th entry of every (row, term), one rounded addition each
                at = order[rank == k]
                a[row[at], term[at]] = a[row[at], term[at]] + x[at]
        den = n.astype(np.float64) + np.float64(strength)
        pm = np.float64(prior) * np.float64(strength)
        mean = np.where(den == 0, np.float32(np.float64(prior)), ((a + pm) / den).astype(np.float32)).astype(np.float32)
        cnt = n.astype(np.float32)
    mbits = mean.view(np.uint32).copy()
    mbits[np.isnan(mean)] = NAN32
    return seen > 0, n, mbits, cnt.view(np.uint32).copy()


def enc_bases(p, kinds, keep_source=True):
    kinds = [int(k) for k in kinds]
    if any(k not in (MEAN, COUNT, MEAN | COUNT) for k in kinds):
        raise ValueError("kinds must be MEAN, COUNT or both")
    eb = [int(p) if keep_source else 0]
    for k in kinds:
        eb.append(eb[-1] + bin(k).count("1"))
    if eb[-1] > MAX_WIDTH:
        raise ValueError("the widths sum above 2^32 - 2")
    return eb


def encode(rp, col, val, p, segment_base, term_segment, count, total, target=POSITIVE, part=None, kinds=None, prior=0.0, strength=0.0, keep_source=True):
    """(row_ptr int64, col uint32, val float32, enc_base uint32[n_terms + 1]) of fmx_matrix_encode_targets' output; the labels are the source's"""
    if not (np.isfinite(prior) and np.isfinite(strength) and strength >= 0):
        raise ValueError("prior and strength must be finite, strength not negative")
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col).astype(np.int64)
    vbits = np.ascontiguousarray(val, np.float32).view(np.uint32)
    n_terms = len(term_segment)
    kinds = [MEAN] * n_terms if kinds is None else [int(k) for k in kinds]
    if len(kinds) != n_terms:
        raise ValueError("one kind per term")
    eb = enc_bases(p, kinds, keep_source)
    present, _, mbits, cbits = encode_values(rp, col, p, segment_base, term_segment, count, total, target, part, prior, strength)
    n = len(rp) - 1
    lens = np.diff(rp)
    rows, order, ids, bits = [], [], [], []
    if keep_source:
        row = np.repeat(np.arange(n, dtype=np.int64), lens)
        rows.append(row); order.append(np.arange(len(col), dtype=np.int64) - rp[row]); ids.append(col); bits.append(vbits)
    far = np.int64(1) << 40
    for t, k in enumerate(kinds):
        r = np.flatnonzero(present[:, t])
        at = 0
        for kind, src in ((MEAN, mbits), (COUNT, cbits)):
            if k & kind:
                rows.append(r); order.append(np.full(len(r), far + 2 * t + at)); ids.append(np.full(len(r), eb[t] + at, np.int64)); bits.append(src[r, t])
                at += 1
    rows, order, ids, bits = (np.concatenate(x) if x else np.zeros(0, np.int64) for x in (rows, order, ids, bits))
    o = np.lexsort((order, rows))
    orp = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))]).astype(np.int64)
    if orp[-1] > 2**31 - 1:
        raise ValueError("the output would hold more than 2^31 - 1 entries")
    return orp, ids[o].astype(np.uint32), bits[o].astype(np.uint32).view(np.float32), np.array(eb, np.uint64).astype(np.uint32)
