"""The numpy restatement of fmx_matrix_cross (include/fmx.h).  It is the definition: ids are integers, the value is the IEEE
binary32 product, so the device's outputs are compared with these by exact equality of bits.  Vectorised: np.searchsorted for the segments,
np.repeat for the pairs, H from tests/split_model.py for the hashed ids."""
import numpy as np

from tests.split_model import H

MAX_SEGMENTS = 4096
MAX_TERMS = 64
STREAM0 = 128
NAN_BITS = 0x7FC00000
MAX_WIDTH = 2**32 - 2
U = np.uint64


def mulhi64(h, n):
    """floor(h * n / 2^64) for uint64 h and 0 < n < 2^32, in uint64 without overflow"""
    h = np.asarray(h, np.uint64)
    n = U(int(n))
    with np.errstate(over="ignore"):
        return (((h >> U(32)) * n + (((h & U(0xFFFFFFFF)) * n) >> U(32))) >> U(32)).astype(np.uint64)


def widths(p, segment_base, terms, keep_source=True):
    """(cross_base as Python ints [n_terms + 1], the term widths): W_t = n_buckets, or width(a) * width(b)"""
    base = [int(b) for b in segment_base]
    w = []
    for term in terms:
        a, b = int(term[0]), int(term[1])
        nb = int(term[2]) if len(term) > 2 else 0
        w.append(nb if nb > 0 else (base[a + 1] - base[a]) * (base[b + 1] - base[b]))
    cb = [int(p) if keep_source else 0]
    for x in w:
        cb.append(cb[-1] + x)
    return cb, w


def product_bits(x, y):
    """the bits of the binary32 product, every NaN as 0x7FC00000"""
    with np.errstate(all="ignore"):
        z = (np.asarray(x, np.float32) * np.asarray(y, np.float32)).astype(np.float32)
    bits = z.view(np.uint32).copy()
    bits[np.isnan(z)] = NAN_BITS
    return bits


def pair_ids(u, v, t, width_b, n_buckets, base, self_cross, seed=0, salt=0):
    """the column ids of term t for local ids (u, v) (int64 arrays)"""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    if self_cross:
        u, v = np.minimum(u, v), np.maximum(u, v)
    if n_buckets > 0:
        key = (u.astype(np.uint64) << U(32)) | v.astype(np.uint64)
        return int(base) + mulhi64(H(seed, salt, key, STREAM0 + t), n_buckets).astype(np.int64)
    return int(base) + u * int(width_b) + v


def term_pairs(rp, seg, a, b, row_of=None):
    """(row, left, right): for every row the pairs of entry positions of term (a, b), rows ascending, i-major inside a row"""
    n = len(rp) - 1
    if row_of is None:
        row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    ia = np.flatnonzero(seg == a)
    ra = row_of[ia]
    na = np.bincount(ra, minlength=n).astype(np.int64)
    start_a = np.concatenate([[0], np.cumsum(na)])[:-1]
    if a == b:
        rank = np.arange(len(ia), dtype=np.int64) - start_a[ra]        # the entry's rank inside E_a of its row
        reps = na[ra] - 1 - rank                                       # partners: the later entries of E_a
        ib, start_b, first = ia, start_a, rank + 1
    else:
        ib = np.flatnonzero(seg == b)
        rb = row_of[ib]
        nb = np.bincount(rb, minlength=n).astype(np.int64)
        start_b = np.concatenate([[0], np.cumsum(nb)])[:-1]
        reps = nb[ra]
        first = np.zeros(len(ia), np.int64)
    total = int(reps.sum())
    left = np.repeat(ia, reps)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(reps) - reps, reps)
    prow = np.repeat(ra, reps)
    right = ib[start_b[prow] + np.repeat(first, reps) + within] if total else np.zeros(0, np.int64)
    return prow, left, right


def cross(rp, col, val, p, segment_base, terms, seed=0, salt=0, keep_source=True):
    """(row_ptr int64, col uint32, val float32, cross_base uint32[n_terms + 1]) of fmx_matrix_cross' output; the labels are the source's.
    Raises ValueError where the call refuses."""
    rp = np.asarray(rp, np.int64)
    col = np.asarray(col).astype(np.int64)
    vbits = np.ascontiguousarray(val, np.float32).view(np.uint32)
    base = np.asarray(segment_base).astype(np.int64)
    n_seg = len(base) - 1
    if not 1 <= n_seg <= MAX_SEGMENTS or not 1 <= len(terms) <= MAX_TERMS:
        raise ValueError("n_segments or n_terms out of range")
    if base[0] != 0 or base[-1] != p or np.any(np.diff(base) < 0):
        raise ValueError("segment_base must ascend from 0 to p")
    for term in terms:
        if not 0 <= int(term[0]) <= int(term[1]) < n_seg:
            raise ValueError("a term's segments must satisfy 0 <= a <= b < n_segments")
    cb, w = widths(p, base, terms, keep_source)
    if cb[-1] > MAX_WIDTH:
        raise ValueError("the widths sum above 2^32 - 2")
    n = len(rp) - 1
    lens = np.diff(rp)
    seg = np.searchsorted(base, col, side="right") - 1                 # the last s with base[s] <= c: an empty segment is never the answer
    parts = []
    counts = np.zeros((len(terms), n), np.int64)
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    for t, term in enumerate(terms):
        a, b = int(term[0]), int(term[1])
        nb = int(term[2]) if len(term) > 2 else 0
        prow, left, right = term_pairs(rp, seg, a, b, row_of)
        ids = pair_ids(col[left] - base[a], col[right] - base[b], t, base[b + 1] - base[b], nb, cb[t], a == b, seed, salt)
        bits = product_bits(vbits[left].view(np.float32), vbits[right].view(np.float32))
        counts[t] = np.bincount(prow, minlength=n)
        parts.append((prow, ids, bits))
    kept = lens if keep_source else np.zeros(n, np.int64)
    olen = kept + counts.sum(axis=0)
    if n and olen.max() > 2**31 - 1:
        raise ValueError(f"row {int(np.argmax(olen > 2**31 - 1))} would hold more than 2^31 - 1 entries")
    orp = np.concatenate([[0], np.cumsum(olen)]).astype(np.int64)
    if orp[-1] > 2**31 - 1:
        raise ValueError("the output would hold more than 2^31 - 1 entries")
    ocol = np.zeros(int(orp[-1]), np.int64)
    obits = np.zeros(int(orp[-1]), np.uint32)
    if keep_source and len(col):
        at = orp[row_of] + (np.arange(len(col), dtype=np.int64) - rp[row_of])
        ocol[at] = col
        obits[at] = vbits
    before = kept.copy()                                               # entries of the row in front of term t
    for t, (prow, ids, bits) in enumerate(parts):
        start = np.concatenate([[0], np.cumsum(counts[t])])[:-1]       # the first pair of every row in the term's list
        at = orp[prow] + before[prow] + (np.arange(len(prow), dtype=np.int64) - start[prow])
        ocol[at] = ids
        obits[at] = bits
        before += counts[t]
    return orp, ocol.astype(np.uint32), obits.view(np.float32), np.array(cb, np.uint64).astype(np.uint32)


def cross_loops(rp, col, val, p, segment_base, terms, seed=0, salt=0, keep_source=True):
    """the same in a plain Python triple loop (rows, terms, pairs), integers and one product at a time: the check of the vectorised model"""
    base = [int(b) for b in segment_base]
    cb, _ = widths(p, base, terms, keep_source)
    vals = np.ascontiguousarray(val, np.float32)
    orp, ocol, obits = [0], [], []

    def seg_of(c):
        s = 0
        for k in range(len(base) - 1):
            if base[k] <= c:
                s = k
        return s
    for r in range(len(rp) - 1):
        entries = [(int(col[e]), vals[e]) for e in range(int(rp[r]), int(rp[r + 1]))]
        if keep_source:
            for c, x in entries:
                ocol.append(c)
                obits.append(int(np.float32(x).view(np.uint32)))
        for t, term in enumerate(terms):
            a, b = int(term[0]), int(term[1])
            nb = int(term[2]) if len(term) > 2 else 0
            ea = [e for e in entries if seg_of(e[0]) == a]
            eb = [e for e in entries if seg_of(e[0]) == b]
            pairs = [(ea[i], ea[j]) for i in range(len(ea)) for j in range(i + 1, len(ea))] if a == b else [(x, y) for x in ea for y in eb]
            for (ci, xi), (cj, xj) in pairs:
                u, v = ci - base[a], cj - base[b]
                if a == b:
                    u, v = min(u, v), max(u, v)
                if nb > 0:
                    h = int(H(seed, salt, np.array([(u << 32) | v], np.uint64), STREAM0 + t)[0])
                    ocol.append(cb[t] + ((h * nb) >> 64))
                else:
                    ocol.append(cb[t] + u * (base[b + 1] - base[b]) + v)
                with np.errstate(all="ignore"):
                    z = np.float32(xi) * np.float32(xj)
                obits.append(NAN_BITS if np.isnan(z) else int(np.float32(z).view(np.uint32)))
        orp.append(len(ocol))
    return (np.array(orp, np.int64), np.array(ocol, np.uint64).astype(np.uint32), np.array(obits, np.uint32).view(np.float32),
            np.array(cb, np.uint64).astype(np.uint32))
