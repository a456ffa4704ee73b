"""Thin object wrappers over the C ABI handles (fmx_engine, fmx_matrix).  numpy in, numpy out."""
import ctypes as C

import numpy as np

from . import _lib as L


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _dp(x):
    """a device pointer given as an integer, a ctypes pointer or None"""
    return x if isinstance(x, C.c_void_p) else C.c_void_p(x)


def _hv(h):
    """a handle as the integer a ctypes field takes"""
    return h.value if isinstance(h, C.c_void_p) else h


def fields_spec(n_dense, field_vocab, skew, seed):
    """(fmx_fields_spec, the numpy array it points to -- keep it alive for the call)."""
    vocab = np.ascontiguousarray(field_vocab, np.uint32)
    spec = L.FieldsSpec(C.sizeof(L.FieldsSpec), int(n_dense), len(vocab), 0, vocab.ctypes.data, float(skew), int(seed))
    return spec, vocab


# BASELINE.json configs[3]: 13 dense + 26 categorical fields, 33 000 000 features in all.  Vocabulary sizes follow the spread
# of the Criteo click logs' 26 categorical columns (a few fields of millions of values, many of a handful).
CRITEO_VOCAB = [9_900_000, 7_900_000, 6_700_000, 4_900_000, 2_200_000, 590_000, 400_000, 250_000, 72404, 39_000, 17_000, 12_000, 7_400, 7_100,
                2_200, 1_500, 980, 160, 110, 63, 36, 14, 10, 4, 3, 3]
assert 13 + sum(CRITEO_VOCAB) == 33_000_000


class Matrix:
    """A device-resident fm.matrix (fmx_matrix*)."""

    def __init__(self, handle, n, p, nnz):
        self.h, self.n, self.p, self.nnz = handle, n, p, nnz

    @classmethod
    def _wrap(cls, handle):
        n, p, nnz = C.c_int64(), C.c_uint32(), C.c_int64()
        L.check(L.lib().fmx_matrix_info(handle, C.byref(n), C.byref(p), C.byref(nnz)))
        return cls(handle, n.value, p.value, nnz.value)

    @classmethod
    def from_csr(cls, row_ptr, col, val, p, y=None, device=0):
        row_ptr = np.ascontiguousarray(row_ptr, np.int64)
        col = np.ascontiguousarray(col, np.uint32)
        val = np.ascontiguousarray(val, np.float32)
        y = None if y is None else np.ascontiguousarray(y, np.float32)
        n = len(row_ptr) - 1
        if len(col) != len(val) or (n >= 0 and len(col) != int(row_ptr[-1])):
            raise ValueError("col/val length does not match row_ptr")
        if y is not None and len(y) != n:
            raise ValueError("target's length is not equal the number of cases...")  # core/Data.h:75-76
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_from_csr(C.c_int(device), C.c_int64(n), C.c_uint32(p), _p(row_ptr), _p(col), _p(val), _p(y),
                                            C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def from_rlist(cls, value, col_idx, row_size, p, labels=None, device=0):
        """R's fm.matrix$features layout (R/fm_matrix.R:25-34)."""
        value = np.ascontiguousarray(value, np.float64)
        col_idx = np.ascontiguousarray(col_idx, np.int32)
        row_size = np.ascontiguousarray(row_size, np.int32)
        labels = None if labels is None else np.ascontiguousarray(labels, np.float64)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_from_rlist(C.c_int(device), C.c_int64(len(row_size)), C.c_uint32(p), C.c_int64(len(value)),
                                              _p(value), _p(col_idx), _p(row_size), _p(labels), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def from_dgc(cls, x, i, p, nrow, ncol, labels=None, device=0):
        """A dgCMatrix's slots as they lie in R (x, i = 0-based row indices, p = column pointers): transposed to rows on the device (fmx_matrix_from_dgc;
        R/fm_matrix.R:26-33 does it with Matrix::t on the host).  scipy: `c = scipy.sparse.csc_matrix(...); from_dgc(c.data, c.indices, c.indptr, *c.shape)`."""
        x = np.ascontiguousarray(x, np.float64)
        i = np.ascontiguousarray(i, np.int32)
        p = np.ascontiguousarray(p, np.int32)
        if len(p) != ncol + 1:
            raise ValueError("p must hold ncol + 1 column pointers")
        if len(i) != len(x):
            raise ValueError("the lengths of i and x differ")
        labels = None if labels is None else np.ascontiguousarray(labels, np.float64)
        if labels is not None and len(labels) != nrow:
            raise ValueError("target's length is not equal the number of cases...")
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_from_dgc(C.c_int(device), C.c_int64(nrow), C.c_uint32(ncol), C.c_int64(len(x)), _p(x), _p(i), _p(p), _p(labels), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def synthetic(cls, n, p, nnz_per_row, seed, row_offset=0, device=0):
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_synthetic(C.c_int(device), C.c_int64(n), C.c_uint32(p), C.c_int32(nnz_per_row), C.c_uint64(seed),
                                             C.c_int64(row_offset), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def synthetic_iid(cls, n, p, nnz_per_row, seed, law=L.COLUMNS_UNIFORM, zipf_s=1.05, row_offset=0, device=0):
        """i.i.d. columns (uniform or Zipf), sorted inside the row (fmx_matrix_synthetic_iid)."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_synthetic_iid(C.c_int(device), C.c_int64(n), C.c_uint32(p), C.c_int32(nnz_per_row), C.c_uint64(seed), C.c_int64(row_offset),
                                                 C.c_int32(law), C.c_double(zipf_s), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def synthetic_ragged(cls, n, p, mean_nnz, seed, min_nnz=1, max_nnz=64, row_offset=0, device=0):
        """Row lengths Poisson(mean_nnz) clipped to [min_nnz, max_nnz], i.i.d. uniform sorted columns (fmx_matrix_synthetic_ragged: SURVEY 8(d)'s ragged variant)."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_synthetic_ragged(C.c_int(device), C.c_int64(n), C.c_uint32(p), C.c_double(mean_nnz), C.c_int32(min_nnz), C.c_int32(max_nnz),
                                                    C.c_uint64(seed), C.c_int64(row_offset), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def synthetic_fields(cls, n, n_dense, field_vocab, skew, seed, row_offset=0, device=0):
        """Criteo-shaped rows: n_dense always-present features + one feature of each categorical field (fmx_matrix_synthetic_fields)."""
        spec, keep = fields_spec(n_dense, field_vocab, skew, seed)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_synthetic_fields(C.c_int(device), C.c_int64(n), C.byref(spec), C.c_int64(row_offset), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def pairs(cls, context, items, positives, n_neg=1, seed=0, epoch=0):
        """The pair matrix of sampled preference pairs for FMX_TASK_RANKING (fmx_matrix_pairs): for every distinct (context c, positive item i) of
        `positives` (a Matrix with one row per context row and one column per item row; stored column ids = positive items), n_neg negatives j drawn
        exactly uniformly from c's non-positives; rows 2t = context(c) + item(i), 2t + 1 = context(c) + item(j), in a shuffled order.  The same
        inputs, seed and epoch give the same bits."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_pairs(context.h, items.h, positives.h, C.c_int32(int(n_neg)), C.c_uint64(int(seed)), C.c_int64(int(epoch)), C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def pairs_hard(cls, engine, context, items, positives, n_neg=1, n_cand=8, seed=0, epoch=0):
        """Hard negatives (fmx_matrix_pairs_hard): the pair matrix of Matrix.pairs(context, items, positives, n_neg, seed, epoch) -- same rows,
        order, positives and shuffle -- except that each negative is the best of n_cand (1..64) candidates drawn uniformly from c's
        non-positives (candidate 0 = Matrix.pairs' negative), best under fmx_topk's order and raw score with `engine`'s current parameters.
        The engine is not modified."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_pairs_hard(engine.h, context.h, items.h, positives.h, C.c_int32(int(n_neg)), C.c_int32(int(n_cand)),
                                              C.c_uint64(int(seed)), C.c_int64(int(epoch)), C.byref(h)))
        return cls._wrap(h)

    def set_fields(self, n_dense, field_base):
        """Vouch for a field layout (fmx_matrix_set_fields): n_dense always-present columns, then one id of every field c in
        [field_base[c], field_base[c + 1]) with value 1; checked on the device."""
        fb = np.ascontiguousarray(field_base, np.uint32)
        L.check(L.lib().fmx_matrix_set_fields(self.h, C.c_int32(int(n_dense)), C.c_int32(len(fb) - 1), _p(fb)))

    def synthetic_values(self, seed, row_offset=0):
        """Redraw every stored value uniform in (0, 1) on the device (fmx_matrix_synthetic_values: SURVEY 8(d)'s value variant); the matrix stops being one-hot."""
        L.check(L.lib().fmx_matrix_synthetic_values(self.h, C.c_uint64(seed), C.c_int64(row_offset)))
        return self

    def set_labels(self, y):
        y = np.ascontiguousarray(y, np.float32)
        if len(y) != self.n:
            raise ValueError("target's length is not equal the number of cases...")
        L.check(L.lib().fmx_matrix_set_labels(self.h, _p(y)))

    def scales(self, norm_columns):
        """SMatrix::scales: z-score the listed columns in place; returns (mean[p], std[p])."""
        nc = np.ascontiguousarray(norm_columns, np.int32)
        mean = np.zeros(max(self.p, 1)); std = np.zeros(max(self.p, 1))
        L.check(L.lib().fmx_matrix_scales(self.h, _p(nc), C.c_int64(len(nc)), _p(mean), _p(std)))
        return mean[: self.p], std[: self.p]

    def normalize(self, mean, std):
        """SMatrix::normalize: apply a model's Scales."""
        mean = np.ascontiguousarray(mean, np.float64); std = np.ascontiguousarray(std, np.float64)
        if len(mean) != self.p or len(std) != self.p:
            raise ValueError("the length of scale:mean or scale:std is not equal")  # util/Smatrix.h:143-145
        L.check(L.lib().fmx_matrix_normalize(self.h, _p(mean), _p(std)))

    def rows_form(self):
        """0 / 1 / 2: the form of phase 1 that large steps take on this matrix (fmx_matrix_rows_form: per-row lane groups, flat, pulled)."""
        f = C.c_int32()
        L.check(L.lib().fmx_matrix_rows_form(self.h, C.byref(f)))
        return f.value

    def export(self, r0=0, r1=None):
        """rows [r0, r1) -> (row_ptr, col, val, y) numpy arrays (row_ptr rebased to 0)."""
        r1 = self.n if r1 is None else r1
        rp = np.zeros(r1 - r0 + 1, np.int64)
        L.check(L.lib().fmx_matrix_export(self.h, C.c_int64(r0), C.c_int64(r1), _p(rp), None, None, None))
        cnt = int(rp[-1])
        col = np.zeros(max(cnt, 1), np.uint32); val = np.zeros(max(cnt, 1), np.float32); y = np.zeros(max(r1 - r0, 1), np.float32)
        L.check(L.lib().fmx_matrix_export(self.h, C.c_int64(r0), C.c_int64(r1), _p(rp), _p(col), _p(val), _p(y)))
        return rp, col[:cnt], val[:cnt], y[: r1 - r0]

    def take(self, rows):
        """fmx_matrix_take: a new Matrix whose row t is row rows[t] of this one (any order, repeats allowed, any length; column ids, value bits and
        label bits copied).  rows: an integer array on the host.  An id outside 0..n-1 is refused."""
        rows = np.asarray(rows)
        if rows.ndim != 1 or (rows.size and rows.dtype.kind not in "iu"):
            raise ValueError("rows must be a one-dimensional integer array")
        rows = np.ascontiguousarray(rows, np.int64)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_take(self.h, _p(rows), len(rows), C.byref(h)))
        return Matrix._wrap(h)

    def take_device(self, dev_rows, n_take):
        """fmx_matrix_take_device: the same from a device buffer of n_take int64 row ids (an integer or a pointer)."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_take_device(self.h, _dp(dev_rows), int(n_take), C.byref(h)))
        return Matrix._wrap(h)

    def select(self, part, which, complement=False, return_rows=False):
        """fmx_matrix_select: the rows r with part[r] == which in ascending r, or with complement every other row that has a part (part[r] !=
        0xFFFFFFFF).  part: uint32[n] (split_assign's output).  return_rows=True returns (Matrix, int64 source rows of its rows)."""
        part = np.ascontiguousarray(part, np.uint32).ravel()
        if len(part) != self.n:
            raise ValueError(f"part must hold one part id per row ({self.n}), got {len(part)}")
        rows = np.zeros(max(self.n, 1), np.int64) if return_rows else None
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_select(self.h, _p(part), int(which), int(bool(complement)), C.byref(h), _p(rows)))
        out = Matrix._wrap(h)
        return (out, rows[: out.n].copy()) if return_rows else out

    def select_device(self, dev_part, which, complement=False):
        """fmx_matrix_select_device: part a device uint32 buffer; returns (Matrix, device pointer of its int64 source rows -- an integer, to be
        released with free_device)."""
        h, rows = C.c_void_p(), C.c_void_p()
        L.check(L.lib().fmx_matrix_select_device(self.h, _dp(dev_part), int(which), int(bool(complement)), C.byref(h), C.byref(rows)))
        return Matrix._wrap(h), rows.value

    def split_entries(self, hold=1, fraction=None, order=L.SPLIT_ORDER_HASH, min_keep=1, seed=0, salt=0):
        """fmx_matrix_split_entries: (kept, held) -- every row's stored entries split in two, `hold` of them held per row (or floor(fraction *
        entries) with fraction given), never more than leave min_keep behind; order SPLIT_ORDER_HASH picks them by a hash of (row, column),
        SPLIT_ORDER_TAIL takes the row's last ones."""
        hk, hh = C.c_void_p(), C.c_void_p()
        count, frac = (0, float(fraction)) if fraction is not None else (int(hold), 0.0)
        L.check(L.lib().fmx_matrix_split_entries(self.h, int(order), count, frac, int(min_keep), int(seed), int(salt), C.byref(hk), C.byref(hh)))
        return Matrix._wrap(hk), Matrix._wrap(hh)

    def column_stats(self, values=True):
        """fmx_matrix_column_stats: (count int64[p][3] = entries, rows, positive rows of every column; value float64[p][2] = the sum and the sum
        of squares of its values, in the fixed order include/fmx.h states -- None with values=False)."""
        count = np.zeros((max(self.p, 1), 3), np.int64)
        value = np.zeros((max(self.p, 1), 2), np.float64) if values else None
        L.check(L.lib().fmx_matrix_column_stats(self.h, _p(count), _p(value)))
        return count[: self.p], (value[: self.p] if values else None)

    def column_stats_device(self, dev_count, dev_value=None):
        """fmx_matrix_column_stats_device: count i64[p][3] and value f64[p][2] (or None) are device buffers."""
        L.check(L.lib().fmx_matrix_column_stats_device(self.h, _dp(dev_count), _dp(dev_value) if dev_value is not None else None))

    def remap_columns(self, cmap, new_p, combine=L.COMBINE_KEEP):
        """fmx_matrix_remap_columns: this matrix under a map of its feature ids (uint32[p]; COLUMN_DROP removes a column's entries) as a new
        Matrix of new_p features.  COMBINE_KEEP relabels in source order, COMBINE_SUM and COMBINE_FIRST sort every row by new id and merge
        equal ids (the fp64 sum rounded once to fp32, or the first entry's bits)."""
        cmap = np.asarray(cmap)
        if cmap.ndim != 1 or len(cmap) != self.p or (cmap.size and cmap.dtype.kind not in "iu"):
            raise ValueError(f"the map must hold one integer id per feature ({self.p})")
        if cmap.size and (int(cmap.min()) < 0 or int(cmap.max()) > L.COLUMN_DROP):
            raise ValueError("the map's values must fit 32 unsigned bits")
        cmap = np.ascontiguousarray(cmap, np.uint32)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_remap_columns(self.h, _p(cmap), int(new_p), int(combine), C.byref(h)))
        return Matrix._wrap(h)

    def remap_columns_device(self, dev_map, new_p, combine=L.COMBINE_KEEP):
        """fmx_matrix_remap_columns_device: the map is a device buffer of uint32[p]."""
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_remap_columns_device(self.h, _dp(dev_map), int(new_p), int(combine), C.byref(h)))
        return Matrix._wrap(h)

    def _bin_cols(self, cols):
        """the column list of the two binning calls, checked on the host: uint32, strictly ascending, below the feature count"""
        cols = np.asarray(cols)
        if cols.ndim != 1 or (cols.size and cols.dtype.kind not in "iu"):
            raise ValueError("cols must be a one-dimensional integer array")
        if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= self.p or np.any(np.diff(cols.astype(np.int64)) <= 0)):
            raise ValueError(f"cols must ascend strictly inside 0..{self.p - 1}")
        return np.ascontiguousarray(cols, np.uint32)

    def column_quantiles(self, cols, bins):
        """fmx_matrix_column_quantiles: equal-mass bin edges of the stored, non-NaN values of the columns `cols` (strictly ascending ids), at most
        bins - 1 of them per column.  Returns (edges: a list of float32 arrays, one per column; count int64[len(cols)][2] = non-NaN and NaN stored
        entries; range float32[len(cols)][2] = the lowest and the highest non-NaN value, +0.0 for a column without one)."""
        cols = self._bin_cols(cols)
        if isinstance(bins, (bool, np.bool_)) or not isinstance(bins, (int, np.integer)) or not 1 <= int(bins) <= L.BINS_MAX_BINS:
            raise ValueError(f"bins must be an integer in 1..{L.BINS_MAX_BINS} (got {bins!r})")
        nc, bins = len(cols), int(bins)
        edges = np.zeros((max(nc, 1), max(bins - 1, 1)), np.float32)
        n_edges = np.zeros(max(nc, 1), np.int32)
        count = np.zeros((max(nc, 1), 2), np.int64)
        rng = np.zeros((max(nc, 1), 2), np.float32)
        keep = cols if nc else np.zeros(1, np.uint32)
        L.check(L.lib().fmx_matrix_column_quantiles(self.h, _p(keep), nc, bins, _p(edges), _p(n_edges), _p(count), _p(rng)))
        return [edges[s, : n_edges[s]].copy() for s in range(nc)], count[:nc], rng[:nc]

    def bin_columns(self, cols, edges):
        """fmx_matrix_bin_columns: this matrix with the columns `cols` (strictly ascending ids) replaced by one-hot bucket ids under `edges` (one
        array per column: strictly ascending, no NaN; the fit's or the caller's).  A binned column of e edges becomes e + 2 features: e + 1 bins
        (the bin of x is the number of edges <= x) and one for NaN.  Returns (Matrix, new_base uint32[p + 1]: the first new id of every old
        column, new_base[p] the new feature count)."""
        cols = self._bin_cols(cols)
        edges = [np.ascontiguousarray(e, np.float32).ravel() for e in edges]
        if len(edges) != len(cols):
            raise ValueError(f"edges must hold one array per column ({len(cols)}), got {len(edges)}")
        for s, e in enumerate(edges):
            if len(e) > L.BINS_MAX_EDGES or np.any(np.isnan(e)) or np.any(e[1:] <= e[:-1]):
                raise ValueError(f"the edges of column {int(cols[s])} must ascend strictly, hold no NaN and at most {L.BINS_MAX_EDGES} values")
        off = np.zeros(len(cols) + 1, np.int64)
        off[1:] = np.cumsum([len(e) for e in edges])
        flat = np.concatenate(edges + [np.zeros(1, np.float32)]).astype(np.float32)
        keep = cols if len(cols) else np.zeros(1, np.uint32)
        spec = L.BinSpec(C.sizeof(L.BinSpec), len(cols), keep.ctypes.data, off.ctypes.data, flat.ctypes.data, 0)
        base = np.zeros(self.p + 1, np.uint32)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_bin_columns(self.h, C.byref(spec), _p(base), C.byref(h)))
        return Matrix._wrap(h), base

    @staticmethod
    def _cross_args(p, segment_base, terms):
        """the segment list and the terms of fmx_matrix_cross, checked on the host: (uint32[n_segments + 1], [(a, b, n_buckets)])"""
        base = np.asarray(segment_base)
        if base.ndim != 1 or not 2 <= len(base) <= L.CROSS_MAX_SEGMENTS + 1 or base.dtype.kind not in "iu":
            raise ValueError(f"segment_base must be a one-dimensional integer array of 2..{L.CROSS_MAX_SEGMENTS + 1} values")
        base = base.astype(np.int64)
        if base[0] != 0 or base[-1] != p or np.any(np.diff(base) < 0):
            raise ValueError(f"segment_base must ascend from 0 to the feature count ({p})")
        terms = list(terms)
        if not 1 <= len(terms) <= L.CROSS_MAX_TERMS:
            raise ValueError(f"terms must hold 1..{L.CROSS_MAX_TERMS} terms (got {len(terms)})")
        out, total = [], 0
        for t, term in enumerate(terms):
            term = tuple(term) if isinstance(term, (tuple, list, np.ndarray)) else ()
            if len(term) not in (2, 3) or any(isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) for x in term):
                raise ValueError(f"term {t} must be (a, b) or (a, b, n_buckets) in integers")
            a, b, nb = int(term[0]), int(term[1]), int(term[2]) if len(term) == 3 else 0
            if not 0 <= a <= b < len(base) - 1:
                raise ValueError(f"term {t} must name segments 0 <= a <= b < {len(base) - 1} (got {a}, {b})")
            if not 0 <= nb <= 0xFFFFFFFF:
                raise ValueError(f"term {t}: n_buckets must be in 0..2^32 - 1")
            total += nb if nb else int(base[a + 1] - base[a]) * int(base[b + 1] - base[b])
            out.append((a, b, nb))
        return base.astype(np.uint32), out, total

    def cross(self, segment_base, terms, seed=0, salt=0, keep_source=True):
        """fmx_matrix_cross: this matrix (keep_source) followed by the crosses `terms` of the column segments [segment_base[s], segment_base[s + 1]).
        A term is (a, b) -- one exact id u * width(b) + v per pair of an entry of segment a and one of segment b -- or (a, b, n_buckets) -- the
        pair hashed into that many ids; a == b crosses a segment with itself (pairs of positions i < j).  The value is the product of the two.
        Returns (Matrix, cross_base uint32[len(terms) + 1]: the first id of every term, cross_base[-1] the new feature count)."""
        base, terms, total = Matrix._cross_args(self.p, segment_base, terms)
        if total + (self.p if keep_source else 0) > 2**32 - 2:
            raise ValueError("the widths of the terms (and of the source) sum above 2^32 - 2")
        arr = (L.CrossTerm * len(terms))(*[L.CrossTerm(a, b, nb, 0) for a, b, nb in terms])
        spec = L.CrossSpec(C.sizeof(L.CrossSpec), len(base) - 1, base.ctypes.data, len(terms), 1 if keep_source else 0, C.addressof(arr),
                           int(seed) & (2**64 - 1), int(salt) & (2**64 - 1), 0)
        cross_base = np.zeros(len(terms) + 1, np.uint32)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_cross(self.h, C.byref(spec), _p(cross_base), C.byref(h)))
        return Matrix._wrap(h), cross_base

    def _parts(self, part):
        """the part array of the target calls: None, or uint32[rows] on the host"""
        if part is None:
            return None
        part = np.asarray(part)
        if part.ndim != 1 or len(part) != self.n or (part.size and part.dtype.kind not in "iu"):
            raise ValueError(f"part must hold one integer part id per row ({self.n})")
        if part.size and (int(part.min()) < 0 or int(part.max()) > 0xFFFFFFFF):
            raise ValueError("the part ids must fit 32 unsigned bits")
        return np.ascontiguousarray(part, np.uint32)

    def target_stats(self, part, segment_base, term_segment, n_parts=1, target=L.TARGET_POSITIVE):
        """fmx_target_stats: the TargetTable of the encoded segments term_segment (strictly ascending indices into the segments [segment_base[s],
        segment_base[s + 1])): per column and part the rows that store the column, the positive ones among them and, under TARGET_LABEL, the sum
        of their labels.  part: uint32[rows] (split_assign's output; a row whose part is >= n_parts is counted nowhere), or None -- every row
        is part 0."""
        spec, keep = TargetTable._spec(segment_base, term_segment, n_parts, target, self.p)
        part = self._parts(part)
        h = C.c_void_p()
        L.check(L.lib().fmx_target_stats(self.h, _p(part), C.byref(spec), C.byref(h)))
        return TargetTable(h)

    def target_stats_device(self, dev_part, segment_base, term_segment, n_parts=1, target=L.TARGET_POSITIVE):
        """fmx_target_stats_device: part is a device uint32 buffer (an integer or a pointer), or None."""
        spec, keep = TargetTable._spec(segment_base, term_segment, n_parts, target, self.p)
        h = C.c_void_p()
        L.check(L.lib().fmx_target_stats_device(self.h, _dp(dev_part) if dev_part is not None else None, C.byref(spec), C.byref(h)))
        return TargetTable(h)

    def encode_targets(self, table, part=None, kinds=None, prior=0.0, strength=20.0, keep_source=True, dev_part=None):
        """fmx_matrix_encode_targets: this matrix (keep_source) followed, per encoded segment of `table` that the row holds, by MEAN -- (a +
        prior * strength) / (n + strength) over the table's cells, the row's own part left out -- and / or COUNT -- n.  kinds: one of
        ENCODE_MEAN, ENCODE_COUNT or both per term (None: MEAN).  part None (and dev_part None): every row is encoded with the totals, the form
        for validation and serving data.  Returns (Matrix, enc_base uint32[terms + 1]: the first new id of every term, enc_base[-1] the new
        feature count)."""
        if not isinstance(table, TargetTable) or not table.h:
            raise TypeError("table must be an open TargetTable")
        kinds = np.full(table.n_terms, L.ENCODE_MEAN, np.uint32) if kinds is None else np.asarray(kinds)
        if kinds.ndim != 1 or len(kinds) != table.n_terms or kinds.dtype.kind not in "iu" or np.any((kinds < 1) | (kinds > 3)):
            raise ValueError(f"kinds must hold ENCODE_MEAN, ENCODE_COUNT or both for each of the {table.n_terms} terms")
        kinds = np.ascontiguousarray(kinds, np.uint32)
        prior, strength = float(prior), float(strength)
        if not (np.isfinite(prior) and np.isfinite(strength) and strength >= 0):
            raise ValueError("prior and strength must be finite and strength must not be negative")
        spec = L.EncodeSpec(C.sizeof(L.EncodeSpec), 1 if keep_source else 0, kinds.ctypes.data, prior, strength, 0)
        enc_base = np.zeros(table.n_terms + 1, np.uint32)
        h = C.c_void_p()
        if dev_part is not None:
            L.check(L.lib().fmx_matrix_encode_targets_device(self.h, table.h, _dp(dev_part), C.byref(spec), _p(enc_base), C.byref(h)))
        else:
            L.check(L.lib().fmx_matrix_encode_targets(self.h, table.h, _p(self._parts(part)), C.byref(spec), _p(enc_base), C.byref(h)))
        return Matrix._wrap(h), enc_base

    @staticmethod
    def _join_blocks(blocks, n, p, labels_from, device_rows):
        """the checks Matrix.join and Matrix.join_device share, on the host: (fmx_join_block array, what it points to, n, p, labels_from)"""
        blocks = list(blocks)
        if not 1 <= len(blocks) <= L.JOIN_MAX_BLOCKS:
            raise ValueError(f"a join takes 1 to {L.JOIN_MAX_BLOCKS} blocks (got {len(blocks)})")
        arr = (L.JoinBlock * len(blocks))()
        keep, fit = [], 0
        for b, blk in enumerate(blocks):
            if not isinstance(blk, (tuple, list)) or len(blk) != 3:
                raise ValueError(f"block {b} must be (Matrix or vocabulary size, rows or None, col_base)")
            src, rows, base = blk
            if isinstance(src, Matrix):
                width = src.p
            elif isinstance(src, (int, np.integer)) and not isinstance(src, (bool, np.bool_)) and int(src) >= 0:
                width = int(src)
                if rows is None:
                    raise ValueError(f"block {b} is an indicator block and needs its ids")
            else:
                raise ValueError(f"block {b}: the source must be a Matrix or a vocabulary size >= 0 (got {src!r})")
            if isinstance(base, (bool, np.bool_)) or not isinstance(base, (int, np.integer)) or not 0 <= int(base) <= 0xFFFFFFFF:
                raise ValueError(f"block {b}: col_base must be an integer in 0..2^32 - 1 (got {base!r})")
            if rows is not None and not device_rows:
                rows = np.asarray(rows)
                if rows.ndim != 1 or (rows.size and rows.dtype.kind not in "iu"):
                    raise ValueError(f"block {b}: rows must be a one-dimensional integer array")
                rows = np.ascontiguousarray(rows, np.int64)
                keep.append(rows)
                if n is None:
                    n = len(rows)
                elif len(rows) != n:
                    raise ValueError(f"block {b} lists {len(rows)} rows, the join has {n}")
            elif rows is None and n is None:
                n = src.n
            arr[b].m = _hv(src.h) if isinstance(src, Matrix) else None
            arr[b].rows = None if rows is None else (_dp(rows) if device_rows else rows.ctypes.data)
            arr[b].n_ids = 0 if isinstance(src, Matrix) else width
            arr[b].col_base = int(base)
            fit = max(fit, int(base) + width)
        if n is None:
            raise ValueError("n is needed: no block lists its rows on the host or is an identity block")
        if p is None:
            p = fit
        if not 0 <= int(p) <= 0xFFFFFFFF:
            raise ValueError(f"the joined feature count {p} does not fit 32 bits")
        return arr, keep, int(n), int(p), -1 if labels_from is None else int(labels_from)

    @classmethod
    def join(cls, blocks, n=None, p=None, labels_from=None, device=0):
        """fmx_matrix_join: a new Matrix whose row t holds, block after block, the entries of row rows_b[t] of block b with col_base_b added to the
        column ids.  blocks: a list of (Matrix | int vocabulary, rows | None, col_base) -- a Matrix contributes its rows' entries, an int an
        INDICATOR block of that many ids (the one entry (col_base + rows[t], 1.0)); rows is an integer array on the host (any order, repeats
        allowed), or None for the identity on a Matrix of exactly n rows.  n=None takes the length of the row lists, p=None the smallest feature
        count that fits, labels_from the block whose rows' labels the output carries (None: no labels)."""
        arr, keep, n, p, lf = cls._join_blocks(blocks, n, p, labels_from, False)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_join(int(device), arr, len(arr), n, p, lf, C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def join_device(cls, blocks, n, p=None, labels_from=None, device=0):
        """fmx_matrix_join_device: the same with every block's rows a device buffer of n int64 ids (an integer or a pointer), or None."""
        arr, keep, n, p, lf = cls._join_blocks(blocks, int(n), p, labels_from, True)
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_join_device(int(device), arr, len(arr), n, p, lf, C.byref(h)))
        return cls._wrap(h)

    @classmethod
    def stack(cls, parts):
        """fmx_matrix_stack: the rows of parts[0], then parts[1], and so on as a new Matrix (1 .. 1024 parts of one feature count on one device;
        labels iff every part has them, a mix is refused)."""
        parts = list(parts)
        if not 1 <= len(parts) <= L.STACK_MAX_PARTS or not all(isinstance(m, Matrix) for m in parts):
            raise ValueError(f"stack takes 1 to {L.STACK_MAX_PARTS} Matrix objects")
        arr = (C.c_void_p * len(parts))(*[_hv(m.h) for m in parts])
        h = C.c_void_p()
        L.check(L.lib().fmx_matrix_stack(arr, len(parts), C.byref(h)))
        return cls._wrap(h)

    def shuffled(self, seed, epoch=0, device=0):
        """This matrix with its rows in the order of row_permutation(n, seed, epoch, device) -- row t of the result is row perm[t] of this one:
        an epoch shuffle for the mini-batch learner, which visits consecutive batches.  device: the matrix's."""
        return self.take(row_permutation(self.n, seed, epoch, device=device))

    def close(self):
        if self.h:
            L.lib().fmx_matrix_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def split_assign(n, groups=None, n_groups=None, scope=L.SPLIT_ROWS, order=L.SPLIT_ORDER_HASH, n_folds=0, hold_count=0, hold_fraction=0.0,
                 min_keep=0, seed=0, salt=0, device=0):
    """fmx_split_assign: the part of every one of n rows as uint32[n] -- hold-out (n_folds = 0: 1 = held, 0 = kept) or folds 0 .. n_folds-1 --
    over all rows (SPLIT_ROWS), inside every group (SPLIT_WITHIN_GROUPS) or by whole groups (SPLIT_GROUPS); include/fmx.h has the rule to the
    bit.  groups: uint32[n] with values < n_groups, or None."""
    n = int(n)
    if groups is not None:
        groups = np.ascontiguousarray(groups, np.uint32).ravel()
        if len(groups) != n:
            raise ValueError(f"groups must hold one group id per row ({n}), got {len(groups)}")
        if n_groups is None:
            n_groups = int(groups.max()) + 1 if len(groups) else 1
    spec = L.SplitSpec(C.sizeof(L.SplitSpec), int(scope), int(order), int(n_folds), int(hold_count), float(hold_fraction), int(min_keep),
                       int(seed), int(salt))
    part = np.zeros(max(n, 1), np.uint32)
    L.check(L.lib().fmx_split_assign(int(device), n, _p(groups), int(n_groups or 1), C.byref(spec), _p(part)))
    return part[:n]


def split_assign_device(n, dev_groups, n_groups, dev_part, device=0, **spec):
    """fmx_split_assign_device: groups (or None) and parts are device uint32 buffers; spec as split_assign's keywords.  A row whose id is
    >= n_groups gets part 0xFFFFFFFF."""
    sp = L.SplitSpec(C.sizeof(L.SplitSpec), int(spec.get("scope", L.SPLIT_ROWS)), int(spec.get("order", L.SPLIT_ORDER_HASH)), int(spec.get("n_folds", 0)),
                     int(spec.get("hold_count", 0)), float(spec.get("hold_fraction", 0.0)), int(spec.get("min_keep", 0)), int(spec.get("seed", 0)),
                     int(spec.get("salt", 0)))
    L.check(L.lib().fmx_split_assign_device(int(device), int(n), _dp(dev_groups), int(n_groups), C.byref(sp), _dp(dev_part)))


def row_permutation(n, seed, epoch=0, device=0):
    """fmx_row_permutation: int64[n], the rows 0 .. n-1 in the order of a hash of (seed, epoch, row); another epoch gives another order."""
    out = np.zeros(max(int(n), 1), np.int64)
    L.check(L.lib().fmx_row_permutation(int(device), int(n), int(seed), int(epoch), _p(out)))
    return out[: int(n)]


def row_permutation_device(n, seed, epoch, dev_rows, device=0):
    L.check(L.lib().fmx_row_permutation_device(int(device), int(n), int(seed), int(epoch), _dp(dev_rows)))


def column_rule(by=L.COLUMNS_BY_ROWS, min_count=0, max_count=0, max_features=0, keep_prefix=0, rare=L.RARE_DROP, segment_base=None):
    """(fmx_column_rule, the numpy array it points to -- keep it alive for the call)"""
    base = None if segment_base is None else np.ascontiguousarray(segment_base, np.uint32)
    rule = L.ColumnRule(C.sizeof(L.ColumnRule), int(by), int(min_count), int(max_count), int(max_features), int(keep_prefix), int(rare),
                        0 if base is None else len(base) - 1, 0, None if base is None else base.ctypes.data)
    return rule, base


def column_map_select(p, count, device=0, **rule):
    """fmx_column_map_select: (map uint32[p], new_p, new_segment_base uint32[segments + 1]) from a count table (Matrix.column_stats) and a
    rule (column_rule's keywords): the columns whose count lies in [min_count, max_count], at most max_features of them (the largest counts),
    renumbered segment by segment, every other column dropped (RARE_DROP) or sent to its segment's bucket (RARE_BUCKET)."""
    p = int(p)
    count = np.ascontiguousarray(count, np.int64)
    if count.shape != (p, 3):
        raise ValueError(f"count must be an int64 table of shape ({p}, 3)")
    ru, base = column_rule(**rule)
    cmap = np.zeros(max(p, 1), np.uint32)
    nsb = np.zeros(max(ru.n_segments, 1) + 1, np.uint32)
    new_p = C.c_uint32()
    L.check(L.lib().fmx_column_map_select(int(device), p, _p(count), C.byref(ru), _p(cmap), C.byref(new_p), _p(nsb)))
    return cmap[:p], new_p.value, nsb


def column_map_select_device(p, dev_count, dev_map, device=0, **rule):
    """fmx_column_map_select_device: count and map are device buffers; returns (new_p, new_segment_base)."""
    ru, base = column_rule(**rule)
    nsb = np.zeros(max(ru.n_segments, 1) + 1, np.uint32)
    new_p = C.c_uint32()
    L.check(L.lib().fmx_column_map_select_device(int(device), int(p), _dp(dev_count), C.byref(ru), _dp(dev_map), C.byref(new_p), _p(nsb)))
    return new_p.value, nsb


def column_map_hash(p, n_buckets, seed=0, salt=0, keep_prefix=0, device=0):
    """fmx_column_map_hash: (map uint32[p], new_p) -- the ids below keep_prefix stay, every other id goes to one of n_buckets ids behind them
    by a hash of (seed, salt, id)."""
    p = int(p)
    cmap = np.zeros(max(p, 1), np.uint32)
    new_p = C.c_uint32()
    L.check(L.lib().fmx_column_map_hash(int(device), p, int(n_buckets), int(seed), int(salt), int(keep_prefix), _p(cmap), C.byref(new_p)))
    return cmap[:p], new_p.value


def column_map_hash_device(p, n_buckets, dev_map, seed=0, salt=0, keep_prefix=0, device=0):
    """fmx_column_map_hash_device: the map is a device buffer of uint32[p]; returns new_p."""
    new_p = C.c_uint32()
    L.check(L.lib().fmx_column_map_hash_device(int(device), int(p), int(n_buckets), int(seed), int(salt), int(keep_prefix), _dp(dev_map), C.byref(new_p)))
    return new_p.value


def join_bases(blocks):
    """The disjoint col_bases of a join: the cumulative feature counts of the blocks (Matrix objects, or vocabulary sizes for indicator blocks),
    int64[len(blocks) + 1]; the last element is the joined feature count."""
    widths = [int(b.p) if isinstance(b, Matrix) else int(b) for b in blocks]
    if any(w < 0 for w in widths):
        raise ValueError("a vocabulary size must not be negative")
    return np.concatenate([[0], np.cumsum(widths, dtype=np.int64)]).astype(np.int64)


def free_device(ptr):
    """fmx_free_device: releases the row list Matrix.select_device returned."""
    L.check(L.lib().fmx_free_device(_dp(ptr)))


class ItemIndex:
    """fmx_item_index: a clustered index over the items' projections (include/fmx.h), made by Engine.index_build or
    Engine.index_from_assign and read by Engine.topk_index.  Plain data on the device; freed with the object."""

    def __init__(self, handle):
        self.h = handle
        n, nl, k, ne = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64()
        L.check(L.lib().fmx_index_info(self.h, C.byref(n), C.byref(nl), C.byref(k), C.byref(ne)))
        self.n_items, self.n_lists, self.k, self.non_empty = n.value, nl.value, k.value, ne.value

    def export(self):
        """(centroids float64[n_lists, k + 1], assign uint32[n_items], list_ptr int64[n_lists + 1], list_item int32[n_items])"""
        cen = np.zeros((self.n_lists, self.k + 1))
        assign = np.zeros(max(self.n_items, 1), np.uint32)
        lp = np.zeros(self.n_lists + 1, np.int64)
        li = np.zeros(max(self.n_items, 1), np.int32)
        L.check(L.lib().fmx_index_export(self.h, _p(cen), _p(assign), _p(lp), _p(li)))
        return cen, assign[: self.n_items], lp, li[: self.n_items]

    centroids = property(lambda self: self.export()[0])
    assign = property(lambda self: self.export()[1])
    list_ptr = property(lambda self: self.export()[2])
    list_item = property(lambda self: self.export()[3])

    def close(self):
        if self.h:
            L.lib().fmx_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TargetTable:
    """fmx_target_table: the per-(column, part) target statistics of the encoded segments (include/fmx.h), made by
    Matrix.target_stats or TargetTable.from_arrays and read by Matrix.encode_targets.  Plain data on the device; freed with the object."""

    def __init__(self, handle):
        self.h = handle
        info = np.zeros(8, np.int64)
        L.check(L.lib().fmx_target_table_info(self.h, _p(info)))
        self.device, self.p, self.n_segments, self.n_terms, self.n_parts, self.target, self.width, self.device_bytes = (int(x) for x in info)

    @staticmethod
    def _spec(segment_base, term_segment, n_parts, target, p=None):
        """(fmx_target_spec, the arrays it points to -- keep them alive for the call), checked on the host"""
        base = np.asarray(segment_base)
        if base.ndim != 1 or not 2 <= len(base) <= L.CROSS_MAX_SEGMENTS + 1 or base.dtype.kind not in "iu":
            raise ValueError(f"segment_base must be a one-dimensional integer array of 2..{L.CROSS_MAX_SEGMENTS + 1} values")
        base = base.astype(np.int64)
        if base[0] != 0 or np.any(np.diff(base) < 0) or base[-1] > 0xFFFFFFFF or (p is not None and base[-1] != p):
            raise ValueError("segment_base must ascend from 0 to the feature count" + (f" ({p})" if p is not None else ""))
        seg = np.asarray(term_segment)
        if seg.ndim != 1 or not 1 <= len(seg) <= L.TARGET_MAX_TERMS or seg.dtype.kind not in "iu":
            raise ValueError(f"term_segment must be a one-dimensional integer array of 1..{L.TARGET_MAX_TERMS} segment indices")
        seg = seg.astype(np.int64)
        if seg[0] < 0 or seg[-1] >= len(base) - 1 or np.any(np.diff(seg) <= 0):
            raise ValueError(f"term_segment must ascend strictly inside 0..{len(base) - 2}")
        if isinstance(n_parts, (bool, np.bool_)) or not isinstance(n_parts, (int, np.integer)) or not 1 <= int(n_parts) <= L.TARGET_MAX_PARTS:
            raise ValueError(f"n_parts must be an integer in 1..{L.TARGET_MAX_PARTS} (got {n_parts!r})")
        if target not in (L.TARGET_POSITIVE, L.TARGET_LABEL):
            raise ValueError("target must be TARGET_POSITIVE or TARGET_LABEL")
        if int((base[seg + 1] - base[seg]).sum()) * int(n_parts) > 2**31 - 1:
            raise ValueError("the encoded segments times n_parts hold more than 2^31 - 1 cells")
        base, seg = base.astype(np.uint32), seg.astype(np.uint32)
        spec = L.TargetSpec(C.sizeof(L.TargetSpec), len(base) - 1, base.ctypes.data, len(seg), seg.ctypes.data, int(n_parts), int(target), 0)
        return spec, (base, seg)

    @classmethod
    def from_arrays(cls, segment_base, term_segment, count, sum=None, target=L.TARGET_POSITIVE, device=0):
        """fmx_target_table_from_arrays: a table from count int64[W][n_parts][2] (rows, positive rows) and, under TARGET_LABEL, sum
        float64[W][n_parts]; the bits are copied."""
        count = np.ascontiguousarray(count, np.int64)
        if count.ndim != 3 or count.shape[2] != 2:
            raise ValueError("count must be an int64 array of shape (W, n_parts, 2)")
        spec, keep = cls._spec(segment_base, term_segment, int(count.shape[1]), target)
        W = int((keep[0].astype(np.int64)[keep[1].astype(np.int64) + 1] - keep[0].astype(np.int64)[keep[1]]).sum())
        if count.shape[0] != W:
            raise ValueError(f"count must hold one row per column of the encoded segments ({W}), got {count.shape[0]}")
        if target == L.TARGET_LABEL:
            if sum is None:
                raise ValueError("a TARGET_LABEL table needs the sums")
            sum = np.ascontiguousarray(sum, np.float64)
            if sum.shape != count.shape[:2]:
                raise ValueError(f"sum must be a float64 array of shape {count.shape[:2]}")
        else:
            sum = None
        h = C.c_void_p()
        L.check(L.lib().fmx_target_table_from_arrays(int(device), C.byref(spec), _p(count), _p(sum), C.byref(h)))
        return cls(h)

    def info(self):
        """fmx_target_table_info as a dict: device, p, n_segments, n_terms, n_parts, target, width (W) and the bytes the table takes on the device"""
        return dict(device=self.device, p=self.p, n_segments=self.n_segments, n_terms=self.n_terms, n_parts=self.n_parts, target=self.target,
                    width=self.width, device_bytes=self.device_bytes)

    def layout(self):
        """(segment_base uint32[n_segments + 1], term_segment uint32[n_terms])"""
        base, seg = np.zeros(self.n_segments + 1, np.uint32), np.zeros(self.n_terms, np.uint32)
        L.check(L.lib().fmx_target_table_export(self.h, _p(base), _p(seg), None, None))
        return base, seg

    def export(self):
        """(count int64[W][n_parts][2] = rows, positive rows; sum float64[W][n_parts], None under TARGET_POSITIVE)"""
        count = np.zeros((max(self.width, 1), self.n_parts, 2), np.int64)
        total = np.zeros((max(self.width, 1), self.n_parts), np.float64) if self.target == L.TARGET_LABEL else None
        L.check(L.lib().fmx_target_table_export(self.h, None, None, _p(count), _p(total)))
        return count[: self.width], (None if total is None else total[: self.width])

    def free(self):
        if self.h:
            L.lib().fmx_target_table_free(self.h)
            self.h = None

    close = free

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Source:
    """fmx_source: generated rows handed out one step at a time (each a Matrix of one batch, owned by the source)."""

    def __init__(self, engine, total_rows, nnz_per_row=0, seed=0, row_offset=0, fields=None):
        spec = None
        if fields is not None:
            spec, self._keep = fields_spec(fields[0], fields[1], fields[2], seed)
        self.h = C.c_void_p()
        L.check(L.lib().fmx_source_open(engine.h, C.byref(spec) if spec is not None else None, C.c_int32(nnz_per_row), C.c_uint64(seed), C.c_int64(row_offset),
                                        C.c_int64(total_rows), C.byref(self.h)))
        self.batch_rows = int(engine.cfg.batch_rows)
        self.steps = -(-int(total_rows) // self.batch_rows)
        # fmx_source holds a raw fmx_engine* and fmx_source_close waits on that engine's stream: the engine must outlive the source.  The source keeps
        # it alive (so `Engine(...).source(...)` and interpreter shutdown order are safe) and registers itself so that Engine.close() closes it first.
        self._engine = engine
        engine._sources.append(self)

    def next(self):
        """the next step's Matrix (a borrowed handle: never close it; it holds the source alive) or None at the end"""
        if not self.h:
            raise ValueError("the source is closed")
        mh, rows = C.c_void_p(), C.c_int64()
        L.check(L.lib().fmx_source_next(self.h, C.byref(mh), C.byref(rows)))
        if not mh.value:
            return None
        m = Matrix._wrap(mh)
        m.close = lambda: None   # owned by the source
        m.__dict__["_borrowed"] = True
        m.__dict__["_source"] = self
        return m

    def close(self):
        """waits for the engine's stream; returns the host seconds spent waiting for tiles' counts"""
        wait = C.c_double()
        if self.h:
            h, self.h = self.h, None
            eng, self._engine = self._engine, None
            if eng is not None and self in eng._sources:
                eng._sources.remove(self)
            L.check(L.lib().fmx_source_close(h, C.byref(wait)))
        return wait.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def measure_gather(table_bytes, row_bytes, n_groups=262_144, per_group=32, in_flight=4, reps=30, device=0):
    """rows/s the memory system serves for uniformly random rows of `row_bytes` from a `table_bytes` table (fmx_measure_gather)."""
    out = C.c_double()
    L.check(L.lib().fmx_measure_gather(C.c_int(device), C.c_int64(table_bytes), C.c_int32(row_bytes), C.c_int64(n_groups), C.c_int32(per_group),
                                       C.c_int32(in_flight), C.c_int32(reps), C.byref(out)))
    return out.value


def measure_gather_matrix(m, r0, nrows, table_rows, row_bytes, in_flight=4, reps=20):
    """rows/s of the bare gather of the table rows that rows [r0, r0 + nrows) of matrix `m` name (fmx_measure_gather_matrix)."""
    out = C.c_double()
    L.check(L.lib().fmx_measure_gather_matrix(m.h, C.c_int64(r0), C.c_int64(nrows), C.c_int64(table_rows), C.c_int32(row_bytes), C.c_int32(in_flight),
                                              C.c_int32(reps), C.byref(out)))
    return out.value


class Engine:
    """Parameters + optimizer state on one GPU (fmx_engine*)."""

    def __init__(self, num_features, **kw):
        cfg = L.default_config()
        for key, value in kw.items():
            if not hasattr(cfg, key):
                raise TypeError(f"unknown engine option {key!r}")
            setattr(cfg, key, value)
        self.cfg = cfg
        self.p = int(num_features)
        self.k = int(cfg.num_factor)
        self.h = C.c_void_p()
        self._sources = []   # open Source objects (they point at this engine)
        L.check(L.lib().fmx_engine_create(C.byref(cfg), C.c_uint64(self.p), C.byref(self.h)))

    def k_padded(self):
        """padded factor count of the mini-batch tables (4 * 2^m floats, or 2 * 2^m doubles with state_fp64)"""
        kp = 2 if self.cfg.state_fp64 else 4
        while kp < self.k:
            kp *= 2
        return kp

    def set_params(self, w0=0.0, w=None, v=None):
        """v: (k, p) array as R holds it (k x p matrix); stored column-major for the ABI."""
        w = None if w is None else np.ascontiguousarray(w, np.float64)
        vv = None
        if v is not None:
            v = np.asarray(v, np.float64)
            if v.shape != (self.k, self.p):
                raise ValueError(f"v must have shape ({self.k}, {self.p})")
            vv = np.ascontiguousarray(v.T).ravel()  # element (f, j) at f + j*k
        if w is not None and w.shape != (self.p,):
            raise ValueError(f"w must have shape ({self.p},)")
        L.check(L.lib().fmx_set_params(self.h, C.c_double(w0), _p(w), _p(vv)))

    def get_params(self):
        w0 = C.c_double()
        w = np.zeros(self.p)
        vv = np.zeros(max(self.k * self.p, 1))
        L.check(L.lib().fmx_get_params(self.h, C.byref(w0), _p(w), _p(vv)))
        v = vv[: self.k * self.p].reshape(self.p, self.k).T.copy()
        return w0.value, w, v

    def get_w0(self):
        """the global bias alone (waits for the engine's stream; no table is copied)"""
        w0 = C.c_double()
        L.check(L.lib().fmx_get_params(self.h, C.byref(w0), None, None))
        return w0.value

    def init_normal(self, seed, mean=0.0, stdev=0.01):
        """w0 = 0, w = 0, V ~ N(mean, stdev) drawn on the device (synthetic workloads; not R's generator)."""
        L.check(L.lib().fmx_init_normal(self.h, C.c_uint64(seed), C.c_double(mean), C.c_double(stdev)))

    def get_rows(self, ids):
        """(w[n], v[k][n]) of the listed features."""
        ids = np.ascontiguousarray(ids, np.uint32)
        w = np.zeros(max(len(ids), 1)); vv = np.zeros(max(len(ids) * self.k, 1))
        L.check(L.lib().fmx_get_rows(self.h, _p(ids), C.c_int64(len(ids)), _p(w), _p(vv)))
        return w[: len(ids)], vv[: len(ids) * self.k].reshape(len(ids), self.k).T.copy()

    def set_rows(self, ids, w=None, v=None):
        ids = np.ascontiguousarray(ids, np.uint32)
        w = None if w is None else np.ascontiguousarray(w, np.float64)
        vv = None if v is None else np.ascontiguousarray(np.asarray(v, np.float64).T).ravel()
        L.check(L.lib().fmx_set_rows(self.h, _p(ids), C.c_int64(len(ids)), _p(w), _p(vv)))

    def fold_in(self, m, ids, l2_w, l2_v, newton_steps=8, apply=False):
        """fmx_fold_in: the rows of the features `ids` solved against the frozen model from the rows of m that store them (squared loss for
        REGRESSION engines, newton_steps Newton steps of the logistic loss for CLASSIFICATION ones): (w float64[n], v float64[k, n],
        rows int64[n], status int32[n]); status 1 = not solved (w, v NaN).  With apply the solved rows are written as set_rows would."""
        ids = np.ascontiguousarray(ids, np.uint32)
        n = len(ids)
        w = np.zeros(max(n, 1)); vv = np.zeros(max(n * self.k, 1))
        rows = np.zeros(max(n, 1), np.int64); status = np.zeros(max(n, 1), np.int32)
        L.check(L.lib().fmx_fold_in(self.h, m.h, _p(ids), n, float(l2_w), float(l2_v), int(newton_steps), 1 if apply else 0, _p(w), _p(vv), _p(rows),
                                    _p(status)))
        return w[:n], vv[: n * self.k].reshape(n, self.k).T.copy(), rows[:n], status[:n]

    def fold_in_pairs(self, m, ids, lambda_w, lambda_v, newton_steps=8, apply=False):
        """fmx_fold_in_pairs: the rows of the features `ids` of a RANKING engine solved against the frozen model from the pairs of the pair
        matrix m (rows 2t, 2t + 1; row 2t preferred) that store them, newton_steps Newton steps of the pairwise logistic loss:
        (w float64[n], v float64[k, n], pairs int64[n], status int32[n]); status 1 = not solved (w, v NaN).  A user-side fold-in (the
        feature in both rows of its pairs) needs lambda_w > 0 or keep_w1 = 0.  With apply the solved rows are written as set_rows would."""
        ids = np.ascontiguousarray(ids, np.uint32)
        n = len(ids)
        w = np.zeros(max(n, 1)); vv = np.zeros(max(n * self.k, 1))
        pairs = np.zeros(max(n, 1), np.int64); status = np.zeros(max(n, 1), np.int32)
        L.check(L.lib().fmx_fold_in_pairs(self.h, m.h, _p(ids), n, float(lambda_w), float(lambda_v), int(newton_steps), 1 if apply else 0, _p(w), _p(vv),
                                          _p(pairs), _p(status)))
        return w[:n], vv[: n * self.k].reshape(n, self.k).T.copy(), pairs[:n], status[:n]

    def save(self, path):
        L.check(L.lib().fmx_engine_save(self.h, str(path).encode()))

    def load(self, path):
        L.check(L.lib().fmx_engine_load(self.h, str(path).encode()))

    def predict(self, m, link=L.LINK_NONE):
        out = np.zeros(max(m.n, 1))
        L.check(L.lib().fmx_predict(self.h, m.h, _p(out), C.c_int(link)))
        return out[: m.n]

    def topk(self, context, items, top_k, exclude=None, link=L.LINK_NONE):
        """The top_k item rows of `items` for every row of `context` under the FM score of the concatenated row (fmx_topk):
        (index int64[n, top_k], score float64[n, top_k]); index -1 / score NaN where a context has fewer eligible items."""
        n, k = context.n, int(top_k)
        idx = np.empty((max(n, 1), max(k, 1)), np.int64)
        score = np.empty((max(n, 1), max(k, 1)), np.float64)
        L.check(L.lib().fmx_topk(self.h, context.h, items.h, exclude.h if exclude is not None else None, C.c_int32(k), C.c_int(link),
                                 _p(idx), _p(score)))
        return idx[:n], score[:n]

    def topk_device(self, context, r0, r1, items, top_k, dev_index, dev_score, exclude=None, link=L.LINK_NONE):
        """fmx_topk_device: rows [r0, r1) of `context` into device buffers (int64 / float64 [r1 - r0][top_k], as integers or pointers)."""
        L.check(L.lib().fmx_topk_device(self.h, context.h, C.c_int64(r0), C.c_int64(r1), items.h, exclude.h if exclude is not None else None,
                                        C.c_int32(int(top_k)), C.c_int(link), C.c_void_p(dev_index), C.c_void_p(dev_score)))

    def contrib(self, m):
        """The exact Shapley value of every stored entry for the raw score, the empty row as baseline (fmx_contrib): float64[nnz] in the
        matrix's entry order; keep_w0 * w0 + the sum over a row's entries = that row's raw prediction."""
        out = np.zeros(max(m.nnz, 1))
        L.check(L.lib().fmx_contrib(self.h, m.h, _p(out)))
        return out[: m.nnz]

    def contrib_device(self, m, r0, r1, dev_out):
        """fmx_contrib_device: the contributions of rows [r0, r1) into a device float64 buffer (an integer or pointer), entry row_ptr[r0] at index 0."""
        L.check(L.lib().fmx_contrib_device(self.h, m.h, C.c_int64(r0), C.c_int64(r1), C.c_void_p(dev_out)))

    def contrib_summary(self, m):
        """fmx_contrib_summary: per feature, over every row of m, {"sum": sum of phi, "abs_sum": sum of |phi|, "count": entries} (fp64 sums in a
        fixed order: the same bits every call)."""
        s, a, c = np.zeros(max(self.p, 1)), np.zeros(max(self.p, 1)), np.zeros(max(self.p, 1), np.int64)
        L.check(L.lib().fmx_contrib_summary(self.h, m.h, _p(s), _p(a), _p(c)))
        return {"sum": s[: self.p], "abs_sum": a[: self.p], "count": c[: self.p]}

    def interactions(self, m, top_m):
        """fmx_interactions: per row of m its top_m strongest pair terms I(a, b) = sum_f (x_a v_a,f)(x_b v_b,f): (a int64[n, top_m], b int64[n, top_m],
        value float64[n, top_m]) -- the two entries' 0-based positions inside the row (a < b) and the value; -1 / -1 / NaN beyond the row's
        m (m - 1) / 2 pairs.  Strongest first: the larger |I|, ties by the lower a, then b.  include/fmx.h has the contract to the bit."""
        n, k = m.n, int(top_m)
        a = np.empty((max(n, 1), max(k, 1)), np.int64)
        b = np.empty((max(n, 1), max(k, 1)), np.int64)
        v = np.empty((max(n, 1), max(k, 1)), np.float64)
        L.check(L.lib().fmx_interactions(self.h, m.h, k, _p(a), _p(b), _p(v)))
        return a[:n], b[:n], v[:n]

    def interactions_device(self, m, r0, r1, top_m, dev_a, dev_b, dev_value):
        """fmx_interactions_device: rows [r0, r1) of m into device buffers (int64 / int64 / float64 [r1 - r0][top_m], as integers or pointers)."""
        L.check(L.lib().fmx_interactions_device(self.h, m.h, int(r0), int(r1), int(top_m), C.c_void_p(dev_a), C.c_void_p(dev_b), C.c_void_p(dev_value)))

    def interactions_summary(self, m, groups, n_groups):
        """fmx_interactions_summary: every pair term of every row of m, summed by the groups of its two entries' features -- {"sum", "abs_sum"
        float64[G, G], "count" int64[G, G]}, symmetric, the diagonal holding the pairs inside one group.  groups: uint32[p] with values
        < n_groups, or None (every feature its own group: needs p <= n_groups).  fp64 sums in a fixed order: the same bits every call."""
        G = int(n_groups)
        if groups is not None:
            groups = np.ascontiguousarray(groups, np.uint32).ravel()
            if len(groups) != self.p:
                raise ValueError(f"groups must hold one group per feature ({self.p}), got {len(groups)}")
        g = max(G, 1)
        s, a, c = np.zeros((g, g)), np.zeros((g, g)), np.zeros((g, g), np.int64)
        L.check(L.lib().fmx_interactions_summary(self.h, m.h, _p(groups), G, _p(s), _p(a), _p(c)))
        return {"sum": s, "abs_sum": a, "count": c}

    def _metrics_link(self, link):
        if link is not None:
            return int(link)
        return L.LINK_LOGISTIC if self.cfg.task == L.TASK_CLASSIFICATION else L.LINK_NONE

    def metrics(self, m, groups=None, n_groups=None, link=None):
        """fmx_metrics: the standard pointwise metrics of the labelled matrix m per row group -- (value float64[G, 6], count int64[G, 4]).
        value columns (_lib.MET_*): AUC, LOGLOSS, ACCURACY, BRIER, MEAN_PRED, MEAN_LABEL for a CLASSIFICATION engine (link LOGISTIC, the
        default, or PROBIT), MSE, RMSE, MAE, MEAN_ERR, MEAN_PRED, MEAN_LABEL for a REGRESSION engine (link NONE, the default, or CLAMP);
        count columns: rows, positives, pairs2 (twice the Mann-Whitney U), correct.  groups: uint32[n] with values < n_groups, or None (one
        group).  An empty group has zero counts and NaN values.  include/fmx.h has the contract to the bit."""
        if groups is not None:
            groups = np.ascontiguousarray(groups, np.uint32).ravel()
            if len(groups) != m.n:
                raise ValueError(f"groups must hold one group id per row ({m.n}), got {len(groups)}")
            if n_groups is None:
                n_groups = int(groups.max()) + 1 if len(groups) else 1
        G = 1 if n_groups is None else int(n_groups)
        value = np.full((max(G, 1), L.MET_VALUES), np.nan)
        count = np.zeros((max(G, 1), L.MET_COUNTS), np.int64)
        L.check(L.lib().fmx_metrics(self.h, m.h, _p(groups), G, self._metrics_link(link), _p(value), _p(count)))
        return value, count

    def metrics_device(self, m, r0, r1, dev_groups, n_groups, dev_value, dev_count=None, link=None):
        """fmx_metrics_device: rows [r0, r1) of m; dev_groups a device uint32 buffer indexed from row r0 (or None: one group), the results
        into device buffers float64[n_groups][6] / int64[n_groups][4] (integers or pointers; dev_count may be None).  A row whose id is
        >= n_groups is ignored."""
        L.check(L.lib().fmx_metrics_device(self.h, m.h, int(r0), int(r1), C.c_void_p(dev_groups), int(n_groups), self._metrics_link(link),
                                           C.c_void_p(dev_value), C.c_void_p(dev_count)))

    @staticmethod
    def _calibrator(cal):
        """the ctypes fmx_calibrator of a calibration dict ({"kind": "none" | "platt" | "steps", ...}; None: NULL) and the arrays it points into"""
        if cal is None:
            return None, ()
        c = L.Calibrator()
        c.struct_size = C.sizeof(L.Calibrator)
        kind = cal["kind"]
        if kind == "none":
            c.kind, c.n_groups, c.link = L.CAL_NONE, 1, int(cal["link"])
            return c, ()
        if kind == "platt":
            ab = np.ascontiguousarray(cal["ab"], np.float64).reshape(-1, 2)
            c.kind, c.n_groups, c.platt = L.CAL_PLATT, len(ab), ab.ctypes.data
            return c, (ab,)
        if kind != "steps":
            raise ValueError(f"unknown calibration kind {kind!r}")
        ns = np.ascontiguousarray(cal["n_steps"], np.int32).ravel()
        thr = np.ascontiguousarray(cal["thr"], np.float64).reshape(len(ns), -1)
        val = np.ascontiguousarray(cal["val"], np.float64).reshape(len(ns), -1)
        if thr.shape != val.shape:
            raise ValueError("thr and val must have one shape")
        c.kind, c.n_groups, c.max_steps = L.CAL_STEPS, len(ns), thr.shape[1]
        c.n_steps, c.thr, c.val = ns.ctypes.data, thr.ctypes.data, val.ctypes.data
        return c, (ns, thr, val)

    def _cal_groups(self, m, groups, n_groups):
        if groups is not None:
            groups = np.ascontiguousarray(groups, np.uint32).ravel()
            if len(groups) != m.n:
                raise ValueError(f"groups must hold one group id per row ({m.n}), got {len(groups)}")
            if n_groups is None:
                n_groups = int(groups.max()) + 1 if len(groups) else 1
        return groups, 1 if n_groups is None else int(n_groups)

    def predict_calibrated(self, m, cal=None, groups=None, n_groups=None, link=L.LINK_LOGISTIC):
        """fmx_predict_calibrated: float64[n], the calibrated probability of every row of m under the calibration dict `cal` (None: the plain
        `link`): {"kind": "platt", "ab": float64[G, 2]}, {"kind": "steps", "n_steps": int32[G], "thr", "val": float64[G, S]} or {"kind": "none",
        "link"}.  A calibration with one map applies to every row; one with G > 1 maps needs groups (uint32[n]) and n_groups == G."""
        groups, G = self._cal_groups(m, groups, n_groups)
        c, keep = self._calibrator(cal)
        out = np.full(max(m.n, 1), np.nan)
        L.check(L.lib().fmx_predict_calibrated(self.h, m.h, _p(groups), G, C.byref(c) if c is not None else None, int(link), _p(out)))
        del keep
        return out[: m.n]

    def predict_calibrated_device(self, m, r0, r1, dev_groups, n_groups, dev_out, cal=None, link=L.LINK_LOGISTIC):
        """fmx_predict_calibrated_device: rows [r0, r1) of m into a device float64 buffer; dev_groups a device uint32 buffer indexed from row r0, or None."""
        c, keep = self._calibrator(cal)
        L.check(L.lib().fmx_predict_calibrated_device(self.h, m.h, int(r0), int(r1), C.c_void_p(dev_groups), int(n_groups), C.byref(c) if c is not None else None,
                                                      int(link), C.c_void_p(dev_out)))
        del keep

    def reliability(self, m, groups=None, n_groups=None, bins=10, binning=L.BINS_WIDTH, cal=None, link=L.LINK_LOGISTIC):
        """fmx_reliability: the reliability table of the labelled matrix m per row group -- {"count" int64[G, B, 2] (rows, positives), "sum_p",
        "lo_z", "hi_z" float64[G, B], "nan_rows" int64[G], "value" float64[G, 4] (_lib.CAL_ECE, CAL_MCE, CAL_BRIER, CAL_LOGLOSS)}.  binning:
        _lib.BINS_WIDTH (equal-width bins of the calibrated probability) or BINS_MASS (equal-mass bins of the raw score, ties kept together).
        include/fmx.h has the contract to the bit."""
        groups, G = self._cal_groups(m, groups, n_groups)
        c, keep = self._calibrator(cal)
        g, B = max(G, 1), max(int(bins), 1)
        out = {"count": np.zeros((g, B, 2), np.int64), "sum_p": np.zeros((g, B)), "lo_z": np.full((g, B), np.nan), "hi_z": np.full((g, B), np.nan),
               "nan_rows": np.zeros(g, np.int64), "value": np.full((g, L.CAL_VALUES), np.nan)}
        L.check(L.lib().fmx_reliability(self.h, m.h, _p(groups), G, int(bins), int(binning), C.byref(c) if c is not None else None, int(link), _p(out["count"]),
                                        _p(out["sum_p"]), _p(out["lo_z"]), _p(out["hi_z"]), _p(out["nan_rows"]), _p(out["value"])))
        del keep
        return out

    def reliability_device(self, m, r0, r1, dev_groups, n_groups, bins, binning, dev_count=None, dev_sum_p=None, dev_lo_z=None, dev_hi_z=None, dev_nan_rows=None,
                           dev_value=None, cal=None, link=L.LINK_LOGISTIC):
        """fmx_reliability_device: rows [r0, r1) of m, the outputs into device buffers (integers or pointers; each may be None)."""
        c, keep = self._calibrator(cal)
        L.check(L.lib().fmx_reliability_device(self.h, m.h, int(r0), int(r1), C.c_void_p(dev_groups), int(n_groups), int(bins), int(binning),
                                               C.byref(c) if c is not None else None, int(link), C.c_void_p(dev_count), C.c_void_p(dev_sum_p), C.c_void_p(dev_lo_z),
                                               C.c_void_p(dev_hi_z), C.c_void_p(dev_nan_rows), C.c_void_p(dev_value)))
        del keep

    def calibrate_platt(self, m, groups=None, n_groups=None, l2=0.1, newton_steps=8):
        """fmx_calibrate_platt: per row group (a, b) of p = logistic(a z + b) by newton_steps Newton steps from (1, 0) under the ridge
        l2 / 2 ((a - 1)^2 + b^2) -- {"kind": "platt", "ab" float64[G, 2], "rows" int64[G], "status" int32[G] (1: not solved, a and b NaN)}."""
        groups, G = self._cal_groups(m, groups, n_groups)
        g = max(G, 1)
        ab, rows, status = np.full((g, 2), np.nan), np.zeros(g, np.int64), np.zeros(g, np.int32)
        L.check(L.lib().fmx_calibrate_platt(self.h, m.h, _p(groups), G, float(l2), int(newton_steps), _p(ab), _p(rows), _p(status)))
        return {"kind": "platt", "ab": ab, "rows": rows, "status": status}

    def calibrate_platt_device(self, m, r0, r1, dev_groups, n_groups, l2, newton_steps, dev_ab=None, dev_rows=None, dev_status=None):
        """fmx_calibrate_platt_device: rows [r0, r1) of m; float64[G][2] / int64[G] / int32[G] device buffers (each may be None)."""
        L.check(L.lib().fmx_calibrate_platt_device(self.h, m.h, int(r0), int(r1), C.c_void_p(dev_groups), int(n_groups), float(l2), int(newton_steps),
                                                   C.c_void_p(dev_ab), C.c_void_p(dev_rows), C.c_void_p(dev_status)))

    def calibrate_isotonic(self, m, groups=None, n_groups=None, bins=256):
        """fmx_calibrate_isotonic: per row group the isotonic step map over `bins` equal-mass bins of the raw score -- {"kind": "steps", "n_steps"
        int32[G], "thr", "val" float64[G, bins]}: p = val[s] for the last step s with thr[s] <= z; unused slots hold NaN."""
        groups, G = self._cal_groups(m, groups, n_groups)
        g, B = max(G, 1), max(int(bins), 1)
        ns, thr, val = np.zeros(g, np.int32), np.full((g, B), np.nan), np.full((g, B), np.nan)
        L.check(L.lib().fmx_calibrate_isotonic(self.h, m.h, _p(groups), G, int(bins), _p(ns), _p(thr), _p(val)))
        return {"kind": "steps", "n_steps": ns, "thr": thr, "val": val}

    def calibrate_isotonic_device(self, m, r0, r1, dev_groups, n_groups, bins, dev_n_steps=None, dev_thr=None, dev_val=None):
        """fmx_calibrate_isotonic_device: rows [r0, r1) of m; int32[G] / float64[G][bins] / float64[G][bins] device buffers (each may be None)."""
        L.check(L.lib().fmx_calibrate_isotonic_device(self.h, m.h, int(r0), int(r1), C.c_void_p(dev_groups), int(n_groups), int(bins), C.c_void_p(dev_n_steps),
                                                      C.c_void_p(dev_thr), C.c_void_p(dev_val)))

    def heldout_rank(self, context, items, heldout, exclude=None):
        """fmx_heldout_rank: (rank int64[nnz], score float64[nnz]) of every held-out entry, in heldout's entry order -- the 0-based position of
        the item in the context's full ranking of the eligible items (fmx_topk's order and raw score, excluded items left out)."""
        nnz = heldout.nnz
        rank = np.zeros(max(nnz, 1), np.int64)
        score = np.zeros(max(nnz, 1))
        L.check(L.lib().fmx_heldout_rank(self.h, context.h, items.h, heldout.h, exclude.h if exclude is not None else None, _p(rank), _p(score)))
        return rank[:nnz], score[:nnz]

    def heldout_rank_device(self, context, r0, r1, items, heldout, dev_rank, dev_score=None, exclude=None):
        """fmx_heldout_rank_device: the ranks (and scores) of the held-out entries of context rows [r0, r1) into device buffers (integers or
        pointers), entry heldout.row_ptr[r0] at index 0."""
        L.check(L.lib().fmx_heldout_rank_device(self.h, context.h, C.c_int64(r0), C.c_int64(r1), items.h, heldout.h,
                                                exclude.h if exclude is not None else None, C.c_void_p(dev_rank),
                                                C.c_void_p(dev_score) if dev_score is not None else None))

    def heldout_metrics(self, context, items, heldout, ks, exclude=None, per_context=False):
        """fmx_heldout_metrics: {"mean": float64[4 len(ks) + 2] (per K: precision, recall, ndcg, hit; then mrr, auc), "counted": (contexts with
        a held-out item, contexts with auc defined)[, "per_context": float64[n_ctx, 4 len(ks) + 2] (NaN rows: no held-out item)]}."""
        ks = np.ascontiguousarray(ks, np.int32).ravel()
        cols = 4 * len(ks) + 2
        out = np.zeros(cols)
        counted = np.zeros(2, np.int64)
        pc = np.zeros((max(context.n, 1), cols)) if per_context else None
        L.check(L.lib().fmx_heldout_metrics(self.h, context.h, items.h, heldout.h, exclude.h if exclude is not None else None, _p(ks),
                                            C.c_int32(len(ks)), _p(out), _p(pc), _p(counted)))
        res = {"mean": out, "counted": (int(counted[0]), int(counted[1]))}
        if per_context:
            res["per_context"] = pc[: context.n]
        return res

    def rank_lists(self, context, items, lists, link=L.LINK_NONE, positions=True):
        """fmx_rank_lists: (score float64[nnz], pos int64[nnz] | None) of every entry of `lists` (row c: the candidate items of context c), in
        lists' entry order -- fmx_topk's score of the pair (link applied) and the 0-based position of the item among the list's distinct
        candidates under fmx_topk's order (always on the raw score)."""
        nnz = lists.nnz
        score = np.zeros(max(nnz, 1))
        pos = np.zeros(max(nnz, 1), np.int64) if positions else None
        L.check(L.lib().fmx_rank_lists(self.h, context.h, items.h, lists.h, C.c_int(link), _p(score), _p(pos)))
        return score[:nnz], (pos[:nnz] if positions else None)

    def rank_lists_device(self, context, r0, r1, items, lists, dev_score, dev_pos=None, link=L.LINK_NONE):
        """fmx_rank_lists_device: the scores (and positions) of the list entries of context rows [r0, r1) into device buffers (integers or
        pointers), entry lists.row_ptr[r0] at index 0."""
        L.check(L.lib().fmx_rank_lists_device(self.h, context.h, C.c_int64(r0), C.c_int64(r1), items.h, lists.h, C.c_int(link),
                                              C.c_void_p(dev_score), C.c_void_p(dev_pos) if dev_pos is not None else None))

    def topk_lists(self, context, items, lists, top_k, link=L.LINK_NONE):
        """fmx_topk_lists: the top_k first distinct candidates of every context's list, as topk returns them: (index int64[n, top_k],
        score float64[n, top_k]); index -1 / score NaN where a list holds fewer distinct candidates."""
        n, k = context.n, int(top_k)
        idx = np.empty((max(n, 1), max(k, 1)), np.int64)
        score = np.empty((max(n, 1), max(k, 1)), np.float64)
        L.check(L.lib().fmx_topk_lists(self.h, context.h, items.h, lists.h, C.c_int32(k), C.c_int(link), _p(idx), _p(score)))
        return idx[:n], score[:n]

    def topk_lists_device(self, context, r0, r1, items, lists, top_k, dev_index, dev_score, link=L.LINK_NONE):
        """fmx_topk_lists_device: rows [r0, r1) of `context` into device buffers (int64 / float64 [r1 - r0][top_k], as integers or pointers)."""
        L.check(L.lib().fmx_topk_lists_device(self.h, context.h, C.c_int64(r0), C.c_int64(r1), items.h, lists.h, C.c_int32(int(top_k)),
                                              C.c_int(link), C.c_void_p(dev_index), C.c_void_p(dev_score)))

    def diversify(self, items, index, score, top_k, trade_off=0.7, relevance=L.DIV_REL_MINMAX, margin=True):
        """fmx_diversify: greedy MMR over ranked pools -- index int64[n, P] / score float64[n, P] as topk / topk_lists return them (-1: an empty
        slot) -> (index int64[n, top_k], score float64[n, top_k], margin float64[n, top_k] | None): per step the slot with the largest
        trade_off * rel - (1 - trade_off) * (largest cosine of the items' projections with a slot picked before); -1 / NaN / NaN beyond the
        slots a pool holds.  include/fmx.h has the contract to the bit."""
        index = np.ascontiguousarray(index, np.int64)
        score = np.ascontiguousarray(score, np.float64)
        if index.ndim != 2 or index.shape != score.shape:
            raise ValueError(f"index and score must be [n, pool] arrays of one shape (got {index.shape} and {score.shape})")
        n, pool = index.shape
        k = int(top_k)
        oi = np.empty((max(n, 1), max(k, 1)), np.int64)
        os_ = np.empty((max(n, 1), max(k, 1)), np.float64)
        om = np.empty((max(n, 1), max(k, 1)), np.float64) if margin else None
        L.check(L.lib().fmx_diversify(self.h, items.h, n, pool, _p(index), _p(score), k, float(trade_off), int(relevance), _p(oi), _p(os_), _p(om)))
        return oi[:n], os_[:n], (om[:n] if margin else None)

    def diversify_device(self, items, n, pool, dev_index, dev_score, top_k, trade_off, relevance, dev_out_index, dev_out_score, dev_out_margin=None):
        """fmx_diversify_device: the same on device buffers (integers or pointers): int64 / float64 [n][pool] in, [n][top_k] out; the margin
        buffer may be None."""
        L.check(L.lib().fmx_diversify_device(self.h, items.h, int(n), int(pool), C.c_void_p(dev_index), C.c_void_p(dev_score), int(top_k),
                                             float(trade_off), int(relevance), C.c_void_p(dev_out_index), C.c_void_p(dev_out_score),
                                             C.c_void_p(dev_out_margin) if dev_out_margin is not None else None))

    def neighbors(self, queries, items, top_k, metric=L.SIM_COSINE, skip_self=False):
        """fmx_neighbors: the top_k rows of `items` most similar to every row of `queries` by the cosine (L.SIM_COSINE) or the dot product
        (L.SIM_DOT) of their factor projections: (index int64[n, top_k], score float64[n, top_k]); index -1 / score NaN where there are fewer
        items.  With skip_self query row r never receives item r (the call with queries is items).  include/fmx.h has the contract to the bit."""
        n, k = queries.n, int(top_k)
        idx = np.empty((max(n, 1), max(k, 1)), np.int64)
        score = np.empty((max(n, 1), max(k, 1)), np.float64)
        L.check(L.lib().fmx_neighbors(self.h, queries.h, items.h, k, int(metric), 1 if skip_self else 0, _p(idx), _p(score)))
        return idx[:n], score[:n]

    def neighbors_device(self, queries, r0, r1, items, top_k, dev_index, dev_score, metric=L.SIM_COSINE, skip_self=False):
        """fmx_neighbors_device: rows [r0, r1) of `queries` into device buffers (int64 / float64 [r1 - r0][top_k], as integers or pointers);
        skip_self goes by the absolute row index."""
        L.check(L.lib().fmx_neighbors_device(self.h, queries.h, int(r0), int(r1), items.h, int(top_k), int(metric), 1 if skip_self else 0,
                                             C.c_void_p(dev_index), C.c_void_p(dev_score)))

    def index_build(self, items, n_lists, n_iter=10, seed=0):
        """fmx_index_build: an ItemIndex of n_lists lists over the rows of `items` -- a deterministic k-means (n_iter rounds from seeds drawn by
        `seed`) over their projections under the engine's current parameters.  include/fmx.h has the contract to the bit."""
        out = C.c_void_p()
        L.check(L.lib().fmx_index_build(self.h, items.h, int(n_lists), int(n_iter), int(seed), C.byref(out)))
        return ItemIndex(out)

    def index_from_assign(self, assign, centroids):
        """fmx_index_from_assign: an ItemIndex from a caller's clustering: assign uint32[n_items] (the list of every item) and centroids
        float64[n_lists, k + 1] (any bits)."""
        assign = np.ascontiguousarray(assign, np.uint32)
        cen = np.ascontiguousarray(centroids, np.float64)
        if cen.ndim != 2 or cen.shape[1] != self.k + 1 or cen.shape[0] < 1:
            raise ValueError(f"centroids must be n_lists x {self.k + 1} (got {cen.shape})")
        out = C.c_void_p()
        L.check(L.lib().fmx_index_from_assign(self.h, len(assign), cen.shape[0], _p(assign), _p(cen), C.byref(out)))
        return ItemIndex(out)

    def topk_index(self, index, context, items, top_k, n_probe, exclude=None, link=L.LINK_NONE):
        """fmx_topk_index: fmx_topk over the items of the n_probe lists of `index` closest to each context: (index int64[n, top_k], score
        float64[n, top_k], scanned int64[n] -- the items in the probed lists)."""
        n, k = context.n, int(top_k)
        idx = np.empty((max(n, 1), max(k, 1)), np.int64)
        score = np.empty((max(n, 1), max(k, 1)), np.float64)
        scanned = np.zeros(max(n, 1), np.int64)
        L.check(L.lib().fmx_topk_index(self.h, index.h, context.h, items.h, exclude.h if exclude is not None else None, k, int(n_probe), int(link),
                                       _p(idx), _p(score), _p(scanned)))
        return idx[:n], score[:n], scanned[:n]

    def topk_index_device(self, index, context, r0, r1, items, top_k, n_probe, dev_index, dev_score, dev_scanned=None, exclude=None, link=L.LINK_NONE):
        """fmx_topk_index_device: rows [r0, r1) of `context` into device buffers (int64 / float64 [r1 - r0][top_k], int64 [r1 - r0] or None)."""
        L.check(L.lib().fmx_topk_index_device(self.h, index.h, context.h, int(r0), int(r1), items.h, exclude.h if exclude is not None else None,
                                              int(top_k), int(n_probe), int(link), C.c_void_p(dev_index), C.c_void_p(dev_score),
                                              C.c_void_p(dev_scanned) if dev_scanned is not None else None))

    def project(self, m, with_w0=False):
        """fmx_project: (base float64[n], s float64[n, k]) of every row of m -- the row's forward (w0 added only with with_w0) and its factor
        sums as fmx_topk holds them, so that topk's raw score of (c, i) is (base_c + base_i) + the fma chain of s_c . s_i in the state type."""
        base = np.zeros(max(m.n, 1))
        s = np.zeros((max(m.n, 1), max(self.k, 1)))
        L.check(L.lib().fmx_project(self.h, m.h, C.c_int32(1 if with_w0 else 0), _p(base), _p(s) if self.k > 0 else None))
        return base[: m.n], s[: m.n, : self.k]

    def project_device(self, m, r0, r1, dev_base, dev_s, with_w0=False):
        """fmx_project_device: rows [r0, r1) into device float64 buffers [r1 - r0] and [r1 - r0][k] (integers or pointers; dev_s may be None at k = 0)."""
        L.check(L.lib().fmx_project_device(self.h, m.h, C.c_int64(r0), C.c_int64(r1), C.c_int32(1 if with_w0 else 0), C.c_void_p(dev_base),
                                           C.c_void_p(dev_s) if dev_s is not None else None))

    def train(self, m, max_iter):
        done = C.c_int64()
        L.check(L.lib().fmx_train(self.h, m.h, C.c_int64(max_iter), C.byref(done)))
        return done.value

    def train_stream(self, total_rows, nnz_per_row=0, seed=0, row_offset=0, fields=None):
        """Streamed training on generated rows (fmx_train_stream); fields = (n_dense, field_vocab, skew) for the Criteo-shaped
        stream.  Returns (examples done, host seconds spent waiting for ingest)."""
        done, wait = C.c_int64(), C.c_double()
        spec = None
        if fields is not None:
            spec, keep = fields_spec(fields[0], fields[1], fields[2], seed)
        L.check(L.lib().fmx_train_stream(self.h, C.byref(spec) if spec is not None else None, C.c_int32(nnz_per_row), C.c_uint64(seed), C.c_int64(row_offset),
                                         C.c_int64(total_rows), C.byref(done), C.byref(wait)))
        return done.value, wait.value

    def train_tracked(self, m, max_iter, step_size, metric=L.EVAL_LL, convergence=1e-4, keep_params=True):
        """Learner::learn with the tracker on; returns dict(done, convergent, iters, evals[, params])."""
        tc = L.TrackConfig(C.sizeof(L.TrackConfig), int(metric), int(step_size), float(convergence), int(bool(keep_params)), 0)
        done, conv = C.c_int64(), C.c_int32()
        L.check(L.lib().fmx_train_tracked(self.h, m.h, C.c_int64(max_iter), C.byref(tc), C.byref(done), C.byref(conv)))
        n = C.c_int64()
        L.check(L.lib().fmx_trace_size(self.h, C.byref(n)))
        iters = np.zeros(max(n.value, 1), np.int64); evals = np.zeros(max(n.value, 1))
        L.check(L.lib().fmx_trace_get(self.h, _p(iters), _p(evals)))
        out = dict(done=done.value, convergent=bool(conv.value), iters=iters[: n.value], evals=evals[: n.value])
        if keep_params:
            out["params"] = [self.trace_params(i) for i in range(n.value)]
        return out

    def trace_params(self, record):
        w0 = C.c_double(); w = np.zeros(self.p); vv = np.zeros(max(self.k * self.p, 1))
        L.check(L.lib().fmx_trace_params(self.h, C.c_int64(record), C.byref(w0), _p(w), _p(vv)))
        return w0.value, w, vv[: self.k * self.p].reshape(self.p, self.k).T.copy()

    def evaluate(self, m, metric):
        out = C.c_double()
        L.check(L.lib().fmx_evaluate(self.h, m.h, C.c_int(metric), C.byref(out)))
        return out.value

    def train_order(self, m, order):
        order = np.ascontiguousarray(order, np.int64)
        L.check(L.lib().fmx_train_order(self.h, m.h, _p(order), C.c_int64(len(order))))

    def num_batches(self, m):
        nb = C.c_int64()
        L.check(L.lib().fmx_num_batches(self.h, m.h, C.byref(nb)))
        return nb.value

    def step(self, m, batch, rows_limit=0):
        L.check(L.lib().fmx_step(self.h, m.h, C.c_int64(batch), C.c_int64(rows_limit)))

    def grad(self, m, batch, rows_limit=0):
        L.check(L.lib().fmx_grad(self.h, m.h, C.c_int64(batch), C.c_int64(rows_limit)))

    def grad_buffer(self):
        ptr, n = C.c_void_p(), C.c_int64()
        L.check(L.lib().fmx_grad_buffer(self.h, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def grad_elem_bytes(self):
        b = C.c_int32()
        L.check(L.lib().fmx_grad_elem_bytes(self.h, C.byref(b)))
        return b.value

    def grad_layout(self):
        """(n_chunks, chunk_features, chunk_elems, tail_offset) of the exchange buffer."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib().fmx_grad_layout(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def grad_begin(self, m, batch, rows_limit=0):
        L.check(L.lib().fmx_grad_begin(self.h, m.h, C.c_int64(batch), C.c_int64(rows_limit)))

    def grad_chunk(self, m, chunk):
        L.check(L.lib().fmx_grad_chunk(self.h, m.h, C.c_int64(chunk)))

    def apply_chunk(self, chunk, global_rows=0, last=False):
        L.check(L.lib().fmx_apply_chunk(self.h, C.c_int64(chunk), C.c_int64(global_rows), C.c_int32(int(last))))

    def compact_info(self, m):
        """(record_elems, capacity, usable) of the compact exchange for this matrix (builds its tile plans)."""
        a, b, u = C.c_int64(), C.c_int64(), C.c_int32()
        L.check(L.lib().fmx_compact_info(self.h, m.h, C.byref(a), C.byref(b), C.byref(u)))
        return a.value, b.value, bool(u.value)

    def compact_count(self, m, batch):
        n = C.c_int64()
        L.check(L.lib().fmx_compact_count(self.h, m.h, C.c_int64(batch), C.byref(n)))
        return n.value

    def compact_reserve(self, capacity):
        L.check(L.lib().fmx_compact_reserve(self.h, C.c_int64(capacity)))

    def grad_compact(self, m, batch, rows_limit=0):
        L.check(L.lib().fmx_grad_compact(self.h, m.h, C.c_int64(batch), C.c_int64(rows_limit)))

    def compact_records(self):
        """(device pointer of the records, record count, device pointer of the 4-element tail)."""
        r, n, t = C.c_void_p(), C.c_int64(), C.c_void_p()
        L.check(L.lib().fmx_compact_records(self.h, C.byref(r), C.byref(n), C.byref(t)))
        return r.value, n.value, t.value

    def apply_compact(self, dev_records, counts, stride, global_rows=0):
        counts = np.ascontiguousarray(counts, np.int64)
        L.check(L.lib().fmx_apply_compact(self.h, C.c_void_p(dev_records), _p(counts), C.c_int32(len(counts)), C.c_int64(stride), C.c_int64(global_rows)))

    def apply(self, global_rows):
        L.check(L.lib().fmx_apply(self.h, C.c_int64(global_rows)))

    def apply_compact_parts(self, dev_records, counts, starts, global_rows=0):
        """parts at explicit record positions (what an uneven all-to-all leaves): fmx_apply_compact_parts"""
        counts = np.ascontiguousarray(counts, np.int64); starts = np.ascontiguousarray(starts, np.int64)
        L.check(L.lib().fmx_apply_compact_parts(self.h, C.c_void_p(dev_records), _p(counts), _p(starts), C.c_int32(len(counts)), C.c_int64(global_rows)))

    # owner-sharded exchange (include/fmx.h: feature j belongs to rank j mod N)
    def owner_configure(self, n_owners, rank):
        L.check(L.lib().fmx_owner_configure(self.h, C.c_int32(n_owners), C.c_int32(rank)))
        self._owners = n_owners

    def owner_info(self, m, batch=0):
        """(counts[n_owners], device pointer of the step's ids in owner-major order)"""
        counts = np.zeros(self._owners, np.int64)
        ids = C.c_void_p()
        L.check(L.lib().fmx_owner_info(self.h, m.h, C.c_int64(batch), _p(counts), C.byref(ids)))
        return counts, ids.value

    def rows_pack(self, dev_ids, n, dev_rows):
        re = C.c_int64()
        L.check(L.lib().fmx_rows_pack(self.h, C.c_void_p(dev_ids), C.c_int64(n), C.c_void_p(dev_rows), C.byref(re)))
        return re.value

    def rows_unpack(self, dev_ids, n, dev_rows):
        L.check(L.lib().fmx_rows_unpack(self.h, C.c_void_p(dev_ids), C.c_int64(n), C.c_void_p(dev_rows)))

    def source(self, total_rows, nnz_per_row=0, seed=0, row_offset=0, fields=None):
        """A streamed source of steps over generated rows (fmx_source_open): iterate with Source.next()."""
        return Source(self, total_rows, nnz_per_row, seed, row_offset, fields)

    def sync(self):
        L.check(L.lib().fmx_sync(self.h))

    def stream(self):
        s = C.c_void_p()
        L.check(L.lib().fmx_stream(self.h, C.byref(s)))
        return s.value

    def als_vsweep(self, m, error, alpha=1.0, v_lambda=None, v_mu=None, std_normals=None):
        """ALS V sweep; std_normals ((k, p) standard normal draws) switches to the MCMC (Gibbs) form."""
        error = np.ascontiguousarray(error, np.float64).copy()
        lam = None if v_lambda is None else np.ascontiguousarray(v_lambda, np.float64)
        mu = None if v_mu is None else np.ascontiguousarray(v_mu, np.float64)
        if std_normals is None:
            L.check(L.lib().fmx_als_vsweep(self.h, m.h, _p(error), C.c_double(alpha), _p(lam), _p(mu)))
        else:
            z = np.ascontiguousarray(std_normals, np.float64)
            if z.shape != (self.k, self.p):
                raise ValueError(f"std_normals must have shape ({self.k}, {self.p})")
            L.check(L.lib().fmx_mcmc_vsweep(self.h, m.h, _p(error), C.c_double(alpha), _p(lam), _p(mu), _p(z)))
        return error

    def vsweep_device(self, m, dev_error, alpha=1.0, v_lambda=None, v_mu=None, dev_std_normals=None):
        """ALS (dev_std_normals None) or MCMC V sweep on a residual that lives on the device (fmx_vsweep_device); pointers are ints."""
        lam = None if v_lambda is None else np.ascontiguousarray(v_lambda, np.float64)
        mu = None if v_mu is None else np.ascontiguousarray(v_mu, np.float64)
        L.check(L.lib().fmx_vsweep_device(self.h, m.h, C.c_void_p(dev_error), C.c_double(alpha), _p(lam), _p(mu),
                                          C.c_void_p(dev_std_normals) if dev_std_normals else None))

    def mcmc_train(self, m, max_iter, std_gammas, std_normals):
        """MCMC learner with caller-drawn variates (fmx.h: fmx_mcmc_train); returns (alpha, w_lambda, w_mu)."""
        g = np.ascontiguousarray(std_gammas, np.float64); z = np.ascontiguousarray(std_normals, np.float64)
        if g.shape != (max_iter, 2) or z.shape != (max_iter, 2 + self.p):
            raise ValueError(f"std_gammas must be ({max_iter}, 2) and std_normals ({max_iter}, {2 + self.p})")
        state = np.zeros(3)
        L.check(L.lib().fmx_mcmc_train(self.h, m.h, C.c_int32(max_iter), _p(g), _p(z), _p(state)))
        return tuple(state)

    def mcmc_train_from(self, m, max_iter, std_gammas, std_normals, state):
        """the chain continued from state = (alpha, w_lambda, w_mu); returns the new state"""
        g = np.ascontiguousarray(std_gammas, np.float64); z = np.ascontiguousarray(std_normals, np.float64)
        st = np.ascontiguousarray(state, np.float64).copy()
        L.check(L.lib().fmx_mcmc_train_from(self.h, m.h, C.c_int32(max_iter), _p(g), _p(z), _p(st)))
        return tuple(st)

    def mcmc_v_hyper(self, v_lambda, v_mu, std_gammas=None, std_normals=None):
        """update_v_lambda + update_v_mu; variates given: the MCMC draws, else the ALS means.  Returns (v_lambda, v_mu)."""
        lam = np.ascontiguousarray(v_lambda, np.float64).copy(); mu = np.ascontiguousarray(v_mu, np.float64).copy()
        sample = std_gammas is not None
        g = None if not sample else np.ascontiguousarray(std_gammas, np.float64)
        z = None if not sample else np.ascontiguousarray(std_normals, np.float64)
        L.check(L.lib().fmx_mcmc_v_hyper(self.h, _p(g), _p(z), _p(lam), _p(mu), C.c_int32(int(sample))))
        return lam, mu

    def als_plan(self, m):
        """(levels or groups, size of the largest, approximate?, level / group of every feature) of the ALS sweeps on this matrix."""
        lv, big, ap = C.c_int64(), C.c_int64(), C.c_int32()
        lof = np.zeros(max(self.p, 1), np.int32)
        L.check(L.lib().fmx_als_plan_info(self.h, m.h, C.byref(lv), C.byref(big), C.byref(ap), _p(lof)))
        return lv.value, big.value, bool(ap.value), lof[: self.p]

    def als_plan_kind(self, m):
        """0: the exact schedule (the reference's feature order); 1: the approximate groups (cfg.als_max_levels exceeded); 2: the coloured order (cfg.als_max_levels = -1, or -2 on a plan with long or heavy lists); 3: the coloured order nested feature-major (-2)."""
        ap = C.c_int32()
        L.check(L.lib().fmx_als_plan_info(self.h, m.h, None, None, C.byref(ap), None))
        return int(ap.value)

    def group_info(self):
        """a cfg.n_gpus handle: replicas, shared device or not, ordered device pairs / those with direct peer access, default exchange of sparse-tile steps"""
        v = [C.c_int32() for _ in range(5)]
        L.check(L.lib().fmx_group_info(self.h, *[C.byref(x) for x in v]))
        return {"replicas": v[0].value, "share_one_device": bool(v[1].value), "device_pairs": v[2].value, "device_pairs_with_direct_peer_access": v[3].value,
                "sparse_exchange": {0: "none", 1: "compact", 2: "owner"}.get(v[4].value, str(v[4].value))}

    def als_tiled(self, m):
        """(levels swept in the row-tiled form, rows per tile, tiles) for this matrix (fmx_als_tiled_info); (0, 0, 0): none."""
        lv, tr, nt = C.c_int32(), C.c_int64(), C.c_int32()
        L.check(L.lib().fmx_als_tiled_info(self.h, m.h, C.byref(lv), C.byref(tr), C.byref(nt)))
        return lv.value, tr.value, nt.value

    def als_level_order(self, m):
        """True when the V sweeps of this matrix take the level-order form (fmx_als_order_info: a complete tiled plan)."""
        v = C.c_int32()
        L.check(L.lib().fmx_als_order_info(self.h, m.h, C.byref(v)))
        return bool(v.value)

    def als_level_order_form(self, m):
        """0: the V sweeps go level by level through the three-pass / column-walking kernels; 1: the tile form of the level-order sweep; 2: the block form."""
        v = C.c_int32()
        L.check(L.lib().fmx_als_order_info(self.h, m.h, C.byref(v)))
        return int(v.value)

    @staticmethod
    def train_grid(engines, m, max_iter):
        """n reference-order learners side by side on one matrix and one visiting order (fmx_train_grid): every engine its own hyper-parameters and state."""
        arr = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
        done = C.c_int64(0)
        L.check(L.lib().fmx_train_grid(arr, C.c_int32(len(engines)), m.h, C.c_int64(max_iter), C.byref(done)))
        return done.value

    def als_carry_q(self, on=True):
        """Opt-in: the block form and the feature-major form (als_max_levels = -2) of the V sweep keep q = X v_f current from sweep to sweep and skip the forward pass that rebuilds it (fmx_als_carry_q)."""
        L.check(L.lib().fmx_als_carry_q(self.h, C.c_int32(int(on))))

    def als_train(self, m, max_iter, with_v=False):
        L.check(L.lib().fmx_als_train(self.h, m.h, C.c_int32(max_iter), C.c_int32(int(with_v))))

    def profile(self, every=1):
        """every = 0: off; n > 0: HIP-event time every n-th launch of each kernel."""
        L.check(L.lib().fmx_profile_enable(self.h, C.c_int(int(every))))

    def profile_reset(self):
        L.check(L.lib().fmx_profile_reset(self.h))

    def profile_get(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        L.check(L.lib().fmx_profile_get(self.h, C.c_int(kernel), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def w_in_row(self):
        """True when the fp32 tables use the w-in-row layout (fmx_layout_info)."""
        a, b = C.c_int32(), C.c_int32()
        L.check(L.lib().fmx_layout_info(self.h, C.byref(a), C.byref(b)))
        return bool(b.value)

    def rows_tune(self):
        """(serial, ms_serial, ms_pipelined): phase 1's schedule for large steps as this engine measured it (fmx_rows_tune_info)."""
        d, a, b = C.c_int32(), C.c_double(), C.c_double()
        L.check(L.lib().fmx_rows_tune_info(self.h, C.byref(d), C.byref(a), C.byref(b)))
        return d.value, a.value, b.value

    def close(self):
        if self.h:
            for src in list(getattr(self, "_sources", [])):   # their fmx_source points at this engine: close them while it exists
                try:
                    src.close()
                except Exception:
                    pass
            L.lib().fmx_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
