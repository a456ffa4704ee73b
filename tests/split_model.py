"""The numpy restatement of the row-selection calls (include/fmx.h: fmx_matrix_take, fmx_split_assign, fmx_matrix_select,
fmx_matrix_split_entries, fmx_row_permutation).  It is the definition: everything is integers and copied bits, so the
device's outputs are compared with these by exact equality.  mix64 in uint64, np.lexsort for the ranks, fancy indexing for the gather."""
import numpy as np

ROWS, WITHIN_GROUPS, GROUPS = 0, 1, 2
ORDER_HASH, ORDER_TAIL = 0, 1
NO_PART = 0xFFFFFFFF
U = np.uint64


def mix64(x):
    """splitmix64's finaliser on a uint64 array (wrapping)"""
    with np.errstate(over="ignore"):
        x = np.array(x, np.uint64)
        x ^= x >> U(30); x *= U(0xBF58476D1CE4E5B9)
        x ^= x >> U(27); x *= U(0x94D049BB133111EB)
        x ^= x >> U(31)
    return x


def H(seed, salt, t, stream):
    """the key of counter t (an array) on `stream`: the pair sampler's chain"""
    with np.errstate(over="ignore"):
        seed = np.array([int(seed) & (2**64 - 1)], np.uint64)
        salt = np.array([int(salt) & (2**64 - 1)], np.uint64)
        h = mix64(seed + U(0x9E3779B97F4A7C15))
        h = mix64(h ^ (salt * U(0xD6E8FEB86659FD93) + U(stream)))
        return mix64(h ^ (np.asarray(t).astype(np.uint64) + U(0x632BE59BD9B4E019)))


def key_row(seed, salt, r):
    return H(seed, salt, r, 0)


def key_group(seed, salt, g):
    return H(seed, salt, g, 1)


def key_entry(seed, salt, r, c):
    return H(seed, salt, (np.asarray(r).astype(np.uint64) << U(32)) | np.asarray(c).astype(np.uint64), 2)


def ranks(item, seg, key):
    """(rho, s) of every item: its 0-based rank inside its segment under (key, item) ascending -- key None: item DESCENDING -- and the
    segment's size"""
    item = np.asarray(item, np.int64); seg = np.asarray(seg, np.int64)
    N = len(item)
    if N == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    order = np.lexsort((-item, seg)) if key is None else np.lexsort((item, key, seg))
    ss = seg[order]
    head = np.r_[True, ss[1:] != ss[:-1]]
    starts = np.flatnonzero(head)
    run = np.cumsum(head) - 1
    sizes = np.diff(np.r_[starts, N])
    rho = np.empty(N, np.int64); s = np.empty(N, np.int64)
    rho[order] = np.arange(N) - starts[run]
    s[order] = sizes[run]
    return rho, s


def part_of(rho, s, n_folds=0, hold_count=0, hold_fraction=0.0, min_keep=0):
    rho = np.asarray(rho, np.int64); s = np.asarray(s, np.int64)
    if n_folds > 0:
        return ((rho * np.int64(n_folds)) // np.maximum(s, 1)).astype(np.uint32)
    c = np.full(len(s), hold_count, np.int64) if hold_count > 0 else np.floor(np.float64(hold_fraction) * s.astype(np.float64)).astype(np.int64)
    q = np.minimum(c, np.maximum(s - np.int64(min(int(min_keep), 2**62)), 0))
    return (rho < q).astype(np.uint32)


def assign(n, groups=None, n_groups=1, scope=ROWS, order=ORDER_HASH, n_folds=0, hold_count=0, hold_fraction=0.0, min_keep=0, seed=0, salt=0):
    """uint32[n]: fmx_split_assign_device's output (a group id >= n_groups gives NO_PART; the host form refuses it)"""
    rule = dict(n_folds=n_folds, hold_count=hold_count, hold_fraction=hold_fraction, min_keep=min_keep)
    r = np.arange(n, dtype=np.int64)
    if scope == ROWS:
        rho, s = ranks(r, np.zeros(n, np.int64), key_row(seed, salt, r) if order == ORDER_HASH else None)
        return part_of(rho, s, **rule)
    groups = np.asarray(groups, np.int64)
    ok = groups < n_groups
    out = np.full(n, NO_PART, np.uint32)
    if scope == WITHIN_GROUPS:
        rr = r[ok]
        rho, s = ranks(rr, groups[ok], key_row(seed, salt, rr) if order == ORDER_HASH else None)
        out[ok] = part_of(rho, s, **rule)
        return out
    g = np.arange(n_groups, dtype=np.int64)
    rho, s = ranks(g, np.zeros(n_groups, np.int64), key_group(seed, salt, g) if order == ORDER_HASH else None)
    out[ok] = part_of(rho, s, **rule)[groups[ok]]
    return out


def take(rp, col, val, y, rows):
    """(row_ptr, col, val, y) of the matrix whose row t is row rows[t]"""
    rp = np.asarray(rp, np.int64); rows = np.asarray(rows, np.int64)
    lens = (rp[1:] - rp[:-1])[rows]
    orp = np.zeros(len(rows) + 1, np.int64)
    orp[1:] = np.cumsum(lens)
    src = np.repeat(rp[rows] - orp[:-1], lens) + np.arange(int(orp[-1]), dtype=np.int64)
    return orp, np.asarray(col)[src], np.asarray(val)[src], (None if y is None else np.asarray(y)[rows])


def select_rows(part, which, complement=False):
    part = np.asarray(part, np.uint32)
    keep = (part != which) & (part != NO_PART) if complement else part == which
    return np.flatnonzero(keep).astype(np.int64)


def entries_held(rp, col, order=ORDER_HASH, hold_count=1, hold_fraction=0.0, min_keep=1, seed=0, salt=0):
    """bool[nnz]: the entries fmx_matrix_split_entries moves to the held output"""
    rp = np.asarray(rp, np.int64)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    e = np.arange(len(row), dtype=np.int64)
    rho, s = ranks(e, row, key_entry(seed, salt, row, col) if order == ORDER_HASH else None)
    return part_of(rho, s, 0, hold_count, hold_fraction, min_keep).astype(bool)


def split_entries(rp, col, val, **rule):
    """((row_ptr, col, val) kept, (row_ptr, col, val) held)"""
    rp = np.asarray(rp, np.int64)
    held = entries_held(rp, col, **rule)
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))
    out = []
    for mask in (~held, held):
        orp = np.zeros(len(rp), np.int64)
        orp[1:] = np.cumsum(np.bincount(row[mask], minlength=len(rp) - 1))
        out.append((orp, np.asarray(col)[mask], np.asarray(val)[mask]))
    return out[0], out[1]


def permutation(n, seed, epoch):
    r = np.arange(n, dtype=np.int64)
    return np.lexsort((r, H(seed, epoch, r, 3))).astype(np.int64)
