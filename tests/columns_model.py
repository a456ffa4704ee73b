"""The numpy restatement of the column-selection calls (include/fmx.h: fmx_matrix_column_stats, fmx_column_map_select, fmx_column_map_hash,
fmx_matrix_remap_columns).  It is the definition: the counts, the maps and the remapped matrix are integers and copied
bits, and every floating-point sum has one stated order, so the device's outputs are compared with these by exact equality."""
import numpy as np

from tests.split_model import H

BY_ROWS, BY_ENTRIES = 0, 1
RARE_DROP, RARE_BUCKET = 0, 1
COMBINE_KEEP, COMBINE_SUM, COMBINE_FIRST = 0, 1, 2
DROP = 0xFFFFFFFF
CHUNK = 1024      # positions of a column's entry list per chunk of the sums
LANES = 64


def tree_sum(terms):
    """THE order of a column's sums.  The column's terms, in ascending (row, position) order, are cut into chunks of 1 024 positions.  Inside a
    chunk lane l of 64 adds the terms at positions l, l + 64, l + 128, ... in that order from +0.0; the 64 lane sums meet in an xor butterfly
    v[l] = v[l] + v[l ^ s] for s = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits).  The chunk sums are added in ascending order from
    +0.0.  Every step is one rounded fp64 addition."""
    terms = np.asarray(terms, np.float64)
    total = np.float64(0.0)
    lane = np.arange(LANES)
    for c0 in range(0, len(terms), CHUNK):
        pad = np.zeros(CHUNK, np.float64)
        chunk = terms[c0:c0 + CHUNK]
        pad[:len(chunk)] = chunk
        v = np.zeros(LANES, np.float64)
        for step in pad.reshape(CHUNK // LANES, LANES):
            v = v + step
        for s in (32, 16, 8, 4, 2, 1):
            v = v + v[lane ^ s]
        total = total + v[0]
    return total


def column_stats(rp, col, val, y, p):
    """(count int64[p][3] = entries, rows, positive rows; value float64[p][2] = sum, sum of squares).  y None: no labels."""
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64); val = np.asarray(val, np.float32)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    count = np.zeros((p, 3), np.int64)
    value = np.zeros((p, 2), np.float64)
    order = np.argsort(col, kind="stable")          # (column, entry index): rows ascend inside a column, same-row duplicates adjacent
    cs, rs = col[order], row[order]
    head = np.ones(len(cs), bool)
    head[1:] = (cs[1:] != cs[:-1]) | (rs[1:] != rs[:-1])
    count[:, 0] = np.bincount(cs, minlength=p)
    count[:, 1] = np.bincount(cs[head], minlength=p)
    if y is not None:
        pos = np.asarray(y, np.float32)[rs] > 0
        count[:, 2] = np.bincount(cs[head & pos], minlength=p)
    x = val[order].astype(np.float64)
    off = np.searchsorted(cs, np.arange(p + 1))
    for j in range(p):
        if off[j + 1] > off[j]:
            xs = x[off[j]:off[j + 1]]
            value[j, 0] = tree_sum(xs)
            value[j, 1] = tree_sum(xs * xs)
    return count, value


def map_select(p, count, by=BY_ROWS, min_count=0, max_count=0, max_features=0, keep_prefix=0, rare=RARE_DROP, segment_base=None):
    """(map uint32[p], new_p, new_segment_base uint32[segments + 1]) -- a function of (count, rule) alone, all in integers."""
    c = np.asarray(count, np.int64).reshape(p, 3)[:, 1 if by == BY_ROWS else 0]
    j = np.arange(p, dtype=np.int64)
    keep = (c >= min_count) & ((c <= max_count) if max_count > 0 else True)
    keep = np.asarray(keep, bool) & (j >= keep_prefix)
    if max_features > 0 and keep.sum() > max_features:
        ck = np.clip(c, 0, 0xFFFFFFFF)
        cand = j[keep]
        best = cand[np.lexsort((cand, -ck[cand]))][:max_features]     # the largest counts, ties to the lower id
        keep = np.zeros(p, bool)
        keep[best] = True
    keep |= j < keep_prefix
    base = np.array([0, p], np.int64) if segment_base is None or len(segment_base) < 2 else np.asarray(segment_base, np.int64)
    nseg = len(base) - 1
    bucket = 1 if rare == RARE_BUCKET else 0
    pos = np.zeros(p + 1, np.int64)
    pos[1:] = np.cumsum(keep)
    out = np.full(p, DROP, np.int64)
    nsb = np.zeros(nseg + 1, np.int64)
    for s in range(nseg):
        a, b = int(base[s]), int(base[s + 1])
        nsb[s] = pos[a] + bucket * s
        seg = np.arange(a, b)
        out[seg] = np.where(keep[seg], pos[seg] + bucket * s, (pos[b] + s) if bucket else DROP)
    nsb[nseg] = pos[p] + bucket * nseg
    return out.astype(np.uint32), int(nsb[nseg]), nsb.astype(np.uint32)


def map_hash(p, n_buckets, seed=0, salt=0, keep_prefix=0):
    """(map uint32[p], new_p): j below keep_prefix stays, every other id goes to keep_prefix + mulhi64(H(seed, salt, j, 4), n_buckets)"""
    h = H(seed, salt, np.arange(p, dtype=np.uint64), 4)
    out = np.array([keep_prefix + ((int(x) * int(n_buckets)) >> 64) for x in h], np.int64).reshape(p)
    out[:min(keep_prefix, p)] = np.arange(min(keep_prefix, p))
    return out.astype(np.uint32), int(keep_prefix) + int(n_buckets)


def remap(rp, col, val, cmap, new_p, combine):
    """(row_ptr, col, val) of fmx_matrix_remap_columns' output; labels are the source's.  A map value that is neither < new_p nor DROP raises."""
    rp = np.asarray(rp, np.int64); col = np.asarray(col, np.int64); val = np.asarray(val, np.float32)
    cmap = np.asarray(cmap, np.uint32).astype(np.int64)
    if np.any((cmap != DROP) & (cmap >= new_p)):
        raise ValueError("a map value is out of range")
    nid = cmap[col] if len(col) else np.zeros(0, np.int64)
    orp = [0]
    ocol, oval = [], []
    for r in range(len(rp) - 1):
        a, b = int(rp[r]), int(rp[r + 1])
        ids, xs = nid[a:b], val[a:b]
        kept = ids != DROP
        ids, xs = ids[kept], xs[kept]
        if combine == COMBINE_KEEP:
            ocol.append(ids); oval.append(xs)
        else:
            order = np.argsort(ids, kind="stable")      # (new id, position in the row)
            ids, xs = ids[order], xs[order]
            head = np.ones(len(ids), bool)
            head[1:] = ids[1:] != ids[:-1]
            starts = np.flatnonzero(head)
            ocol.append(ids[starts])
            if combine == COMBINE_FIRST:
                oval.append(xs[starts])
            else:
                ends = np.r_[starts[1:], len(ids)]
                merged = np.zeros(len(starts), np.float32)
                for t, (s, e) in enumerate(zip(starts, ends)):
                    acc = np.float64(xs[s])
                    for x in xs[s + 1:e]:
                        acc = acc + np.float64(x)
                    merged[t] = np.float32(acc)
                oval.append(merged)
        orp.append(orp[-1] + len(ocol[-1]))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return np.array(orp, np.int64), cat(ocol, np.uint32), cat(oval, np.float32)
