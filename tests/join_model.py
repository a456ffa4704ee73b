"""The numpy restatement of matrix composition (include/fmx.h: fmx_matrix_join, fmx_matrix_stack).  It is the definition:
everything is copied bits, so the device's outputs are compared with these by exact equality.  Fancy indexing and np.repeat, nothing else.

A matrix is (row_ptr int64[n + 1], col uint32[nnz], val float32[nnz], y float32[n] or None).  A block of a join is (source, rows, col_base):
source a matrix, or an int n_ids for an INDICATOR block; rows an int64 array of n_out ids, or None for the identity."""
import numpy as np

MAX_BLOCKS = 16
MAX_PARTS = 1024


def _spread(start, lens):
    """start[t], start[t] + 1, ..., start[t] + lens[t] - 1 for every t, one after the other"""
    first = np.cumsum(lens) - lens
    return np.repeat(start - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def join(blocks, n_out, out_p, labels_from=None):
    """(row_ptr, col, val, y) of the join; ValueError names the lowest (t, b) whose id is out of range"""
    if not 1 <= len(blocks) <= MAX_BLOCKS or n_out < 0:
        raise ValueError("1 to 16 blocks, n_out >= 0")
    ids, lens, bad = [], [], []
    for b, (src, rows, base) in enumerate(blocks):
        indicator = isinstance(src, (int, np.integer))
        n_src = int(src) if indicator else len(src[0]) - 1
        width = int(src) if indicator else None
        if rows is None:
            if indicator or n_src != n_out:
                raise ValueError(f"block {b}: the identity needs a source of exactly n_out rows")
            rows = np.arange(n_out, dtype=np.int64)
        rows = np.asarray(rows, np.int64)
        if len(rows) != n_out:
            raise ValueError(f"block {b}: one id per output row")
        if indicator and int(base) + width > out_p:
            raise ValueError(f"block {b}: col_base + n_ids exceeds out_p")
        wrong = np.flatnonzero((rows < 0) | (rows >= n_src))
        if len(wrong):
            bad.append((int(wrong[0]), b))
        ok = np.where((rows < 0) | (rows >= n_src), 0, rows)
        ids.append(ok)
        if indicator:
            lens.append(np.ones(n_out, np.int64))
        elif n_src == 0:                                          # (n_out > 0 rows of a source of none: every id is out of range)
            lens.append(np.zeros(n_out, np.int64))
        else:
            rp = np.asarray(src[0], np.int64)
            lens.append((rp[1:] - rp[:-1])[ok])
    if bad:
        t, b = min(bad)
        raise ValueError(f"rows[{t}] of block {b} is out of range")
    lens = np.array(lens, np.int64).reshape(len(blocks), n_out)
    orp = np.zeros(n_out + 1, np.int64)
    orp[1:] = np.cumsum(lens.sum(axis=0))
    if lens.sum(axis=0).max(initial=0) > 2**31 - 1:
        raise ValueError("a joined row of more than 2^31 - 1 entries")
    before = np.cumsum(lens, axis=0) - lens                       # entries of row t in the blocks before b
    ocol = np.zeros(int(orp[-1]), np.uint32)
    oval = np.zeros(int(orp[-1]), np.float32)
    for b, (src, _, base) in enumerate(blocks):
        dst = _spread(orp[:-1] + before[b], lens[b])
        if isinstance(src, (int, np.integer)):
            ocol[dst] = (ids[b] + int(base)).astype(np.uint32)
            oval[dst] = np.float32(1.0)
        else:
            rp, col, val = np.asarray(src[0], np.int64), np.asarray(src[1], np.uint32), np.asarray(src[2], np.float32)
            if len(col) and int(col.max()) + int(base) >= out_p:
                raise ValueError(f"block {b}: a column id + col_base reaches out_p")
            from_ = _spread(rp[ids[b]], lens[b])
            ocol[dst] = (col[from_].astype(np.int64) + int(base)).astype(np.uint32)
            oval[dst] = val[from_]
    oy = None
    if labels_from is not None and labels_from >= 0:
        src = blocks[labels_from][0]
        if isinstance(src, (int, np.integer)) or src[3] is None:
            raise ValueError("labels_from names a block without labels")
        oy = np.asarray(src[3], np.float32)[ids[labels_from]]
    return orp, ocol, oval, oy


def stack(parts):
    """(row_ptr, col, val, y) of the parts' rows one after the other; y iff every part has labels, a mix is refused"""
    if not 1 <= len(parts) <= MAX_PARTS:
        raise ValueError("1 to 1024 parts")
    labelled = [m[3] is not None for m in parts]
    if any(labelled) and not all(labelled):
        raise ValueError("parts with and without labels")
    first = np.cumsum([0] + [int(m[0][-1]) for m in parts]).astype(np.int64)
    orp = np.concatenate([np.asarray(m[0], np.int64)[:-1] + first[k] for k, m in enumerate(parts)] + [first[-1:]])
    ocol = np.concatenate([np.asarray(m[1], np.uint32) for m in parts])
    oval = np.concatenate([np.asarray(m[2], np.float32) for m in parts])
    oy = np.concatenate([np.asarray(m[3], np.float32) for m in parts]) if all(labelled) else None
    return orp, ocol, oval, oy


def bases(widths):
    """the disjoint col_bases of blocks of these widths, and the joined feature count as the last element"""
    return np.concatenate([[0], np.cumsum(np.asarray(widths, np.int64))]).astype(np.int64)
