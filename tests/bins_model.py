"""The numpy restatement of the value-binning calls (include/fmx.h: fmx_matrix_column_quantiles, fmx_matrix_bin_columns).
It is the definition: values are only ever compared, through the 32-bit order key vkey, so the device's outputs are compared with these by exact
equality of bits."""
import numpy as np

MAX_BINS = 65536
MAX_EDGES = 65535
NAN_KEY = 0xFFFFFFFF


def vkey(x):
    """THE order of values: the float's bits with -0 taken as +0; a set sign bit gives the complement, otherwise the bits with the top bit set;
    every NaN of either sign gives 0xFFFFFFFF, above +inf's 0xFF800000."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[b == np.uint32(0x80000000)] = 0
    k = np.where(b >> np.uint32(31) != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = NAN_KEY
    return k


def unkey(k):
    """the float32 whose key is k (k not the NaN key)"""
    k = np.asarray(k, np.uint32)
    return np.where(k >> np.uint32(31) != 0, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def column_quantiles(col, val, cols, n_bins):
    """(edges float32[len(cols)][n_bins - 1] padded with +0.0, n_edges int32, count int64[.][2], range float32[.][2]) of the stored entries
    (col, val); cols ascending."""
    col = np.asarray(col, np.int64)
    key = vkey(val)
    nc = len(cols)
    edges = np.zeros((nc, n_bins - 1), np.float32)
    n_edges = np.zeros(nc, np.int32)
    count = np.zeros((nc, 2), np.int64)
    rng = np.zeros((nc, 2), np.float32)
    for s, c in enumerate(cols):
        k = key[col == int(c)]
        L = k[np.argsort(k, kind="stable")]
        L = L[L != NAN_KEY]
        cnt = len(L)
        count[s] = (cnt, len(k) - cnt)
        if cnt == 0:
            continue
        idx = (np.arange(1, n_bins, dtype=np.int64) * cnt) // n_bins
        cand = np.unique(L[idx])
        cand = cand[cand > L[0]]
        n_edges[s] = len(cand)
        edges[s, :len(cand)] = unkey(cand)
        rng[s] = (unkey(L[:1])[0], unkey(L[-1:])[0])
    return edges, n_edges, count, rng


def new_base(p, cols, edges):
    """uint32[p + 1]: the exclusive prefix sum of the widths -- 1 for an unbinned column, edges + 2 for a binned one"""
    width = np.ones(p, np.int64)
    for c, e in zip(cols, edges):
        width[int(c)] = len(e) + 2
    base = np.zeros(p + 1, np.int64)
    np.cumsum(width, out=base[1:])
    return base.astype(np.uint32)


def bin_columns(col, val, p, cols, edges):
    """(new column ids uint32, new values float32, new_base uint32[p + 1]) of the stored entries (col, val) in their order; edges: one float32
    array per column of cols, strictly ascending, no NaN."""
    col = np.asarray(col, np.int64)
    val = np.ascontiguousarray(val, np.float32)
    base = new_base(p, cols, edges).astype(np.int64)
    ocol = base[col] if len(col) else np.zeros(0, np.int64)
    oval = val.copy()
    for c, e in zip(cols, edges):
        e = np.ascontiguousarray(e, np.float32)
        at = col == int(c)
        x = val[at]
        nan = np.isnan(x)
        b = np.searchsorted(e, np.where(nan, np.float32(0), x), side="right")
        ocol[at] = base[int(c)] + np.where(nan, len(e) + 1, b)
        oval[at] = np.float32(1.0)
    return ocol.astype(np.uint32), oval, base.astype(np.uint32)
