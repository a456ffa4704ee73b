"""fmx_matrix_column_quantiles / fmx_matrix_bin_columns and fm_bin_features / fm_apply_bins against the numpy model of the definition
(tests/bins_model.py).  Values are only ever compared, so every comparison is exact equality of bits: in both forms of the apply kernel (the edge
table in LDS, or read from global memory), on the boundary between them (the hook lowers it to 4 and 8 edges) and with launches of 8 entries."""
import ctypes as C

import numpy as np
import pytest

from tests import bins_cases as bc
from tests import bins_model as bm

pytestmark = pytest.mark.gpu

N_BINS = [1, 2, 3, 10, 256, 4096, 65536]
# fmx_debug_bins_limits' arguments: (lds_edges, chunk_entries)
FORMS = {"default": (0, 0), "second call": (0, 0), "lds": (12288, 0), "global": (-1, 0), "lds4": (4, 0), "lds8": (8, 0), "lds, launches of 8": (0, 8),
         "global, launches of 8": (-1, 8)}
_cache = {}


def _limits(lds=0, chunk=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_bins_limits(lds, chunk))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _flags(m):
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    return out.tolist()


def _source(name):
    """(Matrix, (row_ptr, col, val, y or None), p) -- made once, shared, never changed"""
    from fmwr_amd import engine
    if name in _cache:
        return _cache[name]
    if name == "counted":
        rp, col, val, y, p = bc.counted()
    elif name == "unit":                       # the same entries with every value 1.0: the detector marks it unit_values, the values are never read
        rp, col, val, y, p = bc.counted()
        val = np.ones_like(val)
    elif name in ("mixed", "mixed_unl"):
        rp, col, val, y = bc.mixed()
        p = bc.P
        y = None if name == "mixed_unl" else y
    elif name == "wide":                       # 70 columns, for a list of 64 of them
        rng = np.random.default_rng(4)
        lens = rng.integers(0, 9, 300)
        rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        col, val, y, p = rng.integers(0, 70, int(rp[-1])).astype(np.uint32), rng.normal(0, 1, int(rp[-1])).astype(np.float32), None, 70
    else:
        raise KeyError(name)
    m = engine.Matrix.from_csr(rp, col, val, p, y)
    _cache[name] = (m, (rp, col, val, y), p)
    return _cache[name]


def _fit_model(name, cols, n_bins):
    key = ("fit", name, tuple(int(c) for c in cols), n_bins)
    if key not in _cache:
        _, host, _ = _source(name)
        _cache[key] = bm.column_quantiles(host[1], host[2], cols, n_bins)
    return _cache[key]


def _raw_fit(m, cols, n_bins):
    """the C call itself, its padded outputs as they come back"""
    from fmwr_amd import _lib as L
    cols = np.ascontiguousarray(cols, np.uint32)
    nc = len(cols)
    edges = np.full((max(nc, 1), max(n_bins - 1, 1)), 7.0, np.float32)
    n_edges, count, rng = np.full(max(nc, 1), 7, np.int32), np.full((max(nc, 1), 2), 7, np.int64), np.full((max(nc, 1), 2), 7.0, np.float32)
    keep = cols if nc else np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib().fmx_matrix_column_quantiles(m.h, p(keep), nc, n_bins, p(edges), p(n_edges), p(count), p(rng)))
    return edges[:nc, :n_bins - 1], n_edges[:nc], count[:nc], rng[:nc]


def _same_fit(got, ref, what):
    for g, r, part in zip(got, ref, ("edges", "n_edges", "count", "range")):
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(bc.bits(g), bc.bits(r)), (what, part)


# ------------------------------------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("n_bins", N_BINS)
@pytest.mark.parametrize("name", ["counted", "mixed", "unit"])
def test_fit_equals_the_model(name, n_bins):
    m, host, p = _source(name)
    cols = np.arange(p)
    ref = _fit_model(name, cols, n_bins)
    _same_fit(_raw_fit(m, cols, n_bins), ref, (name, n_bins))
    if name == "counted":
        assert ref[2][:, 0].tolist() == list(bc.COUNTS)
    if name == "unit":
        assert _flags(m)[1] == 1 and not ref[1].any() and np.all(ref[3][np.array(bc.COUNTS) > 0] == 1.0)     # read as 1.0f: one value, no edge
    edges, count, rng = m.column_quantiles(cols, n_bins)
    assert [len(e) for e in edges] == ref[1].tolist() and np.array_equal(count, ref[2]) and np.array_equal(bc.bits(rng), bc.bits(ref[3]))
    for s, e in enumerate(edges):
        assert np.array_equal(bc.bits(e), bc.bits(ref[0][s, :ref[1][s]]))


@pytest.mark.parametrize("name,cols", [("wide", []), ("wide", [69]), ("wide", [0, 33, 69]), ("wide", list(range(3, 67))), ("wide", list(range(70))),
                                       ("mixed", [4]), ("mixed", [2, 5, 6, 7])])
def test_fit_of_a_column_list_in_every_launch_cut(name, cols):
    m, host, p = _source(name)
    for n_bins in (5, 256):
        ref = _fit_model(name, cols, n_bins)
        for what, hook in (("default", (0, 0)), ("second call", (0, 0)), ("launches of 8", (0, 8)), ("launches of 4", (0, 1))):
            _limits(*hook)
            _same_fit(_raw_fit(m, cols, n_bins), ref, (name, cols, n_bins, what))


def test_a_columns_fit_depends_on_its_own_values_alone():
    """the other columns' entries permuted or dropped, the rows cut elsewhere: the same bits"""
    from fmwr_amd import engine
    _, host, p = _source("mixed")
    rp, col, val, _ = host
    cols = [1, 2, 5, 7]
    ref = _fit_model("mixed", cols, 10)
    rng = np.random.default_rng(8)
    mine = np.isin(col, cols)
    perm = rng.permutation(len(col))
    variants = {"all entries permuted": (col[perm], val[perm]), "the other columns dropped": (col[mine], val[mine]),
                "the other columns' values redrawn": (col, np.where(mine, val, rng.normal(0, 9, len(val)).astype(np.float32)))}
    for what, (c, v) in variants.items():
        cuts = np.sort(rng.integers(0, len(c) + 1, 57))
        m = engine.Matrix.from_csr(np.concatenate([[0], cuts, [len(c)]]).astype(np.int64), c, v, p)
        _same_fit(_raw_fit(m, cols, 10), ref, what)
        m.close()


# ---------------------------------------------------------------------------------------------------------------------------- the apply
def _specs(name):
    """the (cols, edges) pairs of one source: the fit's edges and hand-made ones"""
    _, host, p = _source(name)
    out = {}
    for n_bins in (8, 256):
        cols = np.arange(p)
        e, ne, _, _ = _fit_model(name, cols, n_bins)
        out[f"every column at {n_bins} bins"] = (cols, [e[s, :ne[s]] for s in range(p)])
    f32 = lambda *a: np.array(a, np.float32)
    lo, hi = np.nanmin(host[2][np.isfinite(host[2])]), np.nanmax(host[2][np.isfinite(host[2])])
    value = host[2][host[1] == 1][:1]                       # a stored value of column 1 as an edge: it lies in the bin above it
    assert len(value) == 1 and not np.isnan(value[0])
    out["hand-made"] = ([0, 1, 2, 3, 5, p - 1], [f32(), value, f32(-np.inf, 0.0, np.inf), f32(lo - 1), f32(hi + 1), f32(-1.0, -0.0, 1e-45)])
    for total in (4, 5, 8, 9):                              # the packed table on both sides of the hook's LDS bounds
        out[f"{total} edges in all"] = ([p - 1], [(np.arange(total) - total / 2 + 0.25).astype(np.float32)])
    out["4 + 4 edges"] = ([1, p - 1], [f32(-1.5, -0.25, 0.25, 1.5), f32(-2.0, -0.5, 0.5, 2.0)])
    out["4 + 5 edges"] = ([1, p - 1], [f32(-1.5, -0.25, 0.25, 1.5), f32(-2.0, -0.5, 0.0, 0.5, 2.0)])
    out["no column"] = ([], [])
    return out


@pytest.mark.parametrize("name", ["counted", "mixed", "mixed_unl", "unit"])
def test_apply_equals_the_model_in_both_forms(name):
    from fmwr_amd import engine
    m, host, p = _source(name)
    rp, col, val, y = host
    for what, (cols, edges) in _specs(name).items():
        ocol, oval, base = bm.bin_columns(col, val, p, cols, edges)
        up = engine.Matrix.from_csr(rp, ocol, oval, int(base[-1]), y)        # the model's output, uploaded: its flags are the detector's
        want = _flags(up)
        up.close()
        for form, hook in FORMS.items():
            _limits(*hook)
            out, nb = m.bin_columns(cols, edges)
            assert nb.dtype == np.uint32 and np.array_equal(nb, base), (name, what, form)
            assert (out.n, out.p, out.nnz) == (m.n, int(base[-1]), m.nnz)
            grp, gcol, gval, gy = out.export()
            assert np.array_equal(grp, rp), (name, what, form)
            assert np.array_equal(gcol, ocol), (name, what, form)
            assert np.array_equal(bc.bits(gval), bc.bits(oval)), (name, what, form)
            if y is not None:
                assert np.array_equal(bc.bits(gy), bc.bits(y))
            assert _flags(out) == want, (name, what, form)
            out.close()
    src = m.export()
    assert np.array_equal(src[1], col) and np.array_equal(bc.bits(src[2]), bc.bits(val))      # the source is left as it was


def test_every_bin_of_the_fitting_matrix_is_non_empty():
    m, host, p = _source("counted")
    for n_bins in (2, 10, 256):
        edges, count, _ = m.column_quantiles(np.arange(p), n_bins)
        out, base = m.bin_columns(np.arange(p), edges)
        stats, _ = out.column_stats(values=False)
        for c in range(p):
            bins = stats[base[c]:base[c + 1] - 1, 0]                          # the column's bins; the id behind them is NaN's
            assert len(bins) == len(edges[c]) + 1 and stats[base[c + 1] - 1, 0] == 0
            assert bins.sum() == count[c, 0] and (np.all(bins > 0) if count[c, 0] else not bins.any()), (n_bins, c)
        out.close()


def test_binned_dense_columns_make_a_field_layout_that_trains_to_the_same_bits():
    """all dense-prefix columns of a synthetic_fields matrix binned: one id per former dense column and per field, every value 1.0.
    fmx_matrix_set_fields accepts new_base's restriction to them, and five mini-batch steps on that layout leave the parameter bits of five steps
    on the same entries uploaded without one."""
    from fmwr_amd import _lib as L, engine
    vocab, dense = [50, 40, 30, 7], 3
    m = engine.Matrix.synthetic_fields(2000, dense, vocab, 1.1, 9)
    rp, col, val, y = m.export()
    cols = np.arange(dense)
    edges, count, _ = m.column_quantiles(cols, 16)
    assert np.all(count[:, 0] == 2000) and all(len(e) > 0 for e in edges)
    out, base = m.bin_columns(cols, edges)
    ocol, oval, mbase = bm.bin_columns(col, val, m.p, cols, edges)
    got = out.export()
    assert np.array_equal(base, mbase) and np.array_equal(got[0], rp) and np.array_equal(got[1], ocol) and np.array_equal(bc.bits(got[2]), bc.bits(oval))
    assert np.array_equal(bc.bits(got[3]), bc.bits(y)) and np.all(oval == 1.0)
    fields = np.concatenate([[0], np.cumsum(vocab)]) + dense
    bases = np.concatenate([base[:dense], base[fields]]).astype(np.uint32)       # the binned columns' bases, then the fields', then the feature count
    assert bases[0] == 0 and bases[-1] == out.p and len(bases) == dense + len(vocab) + 1
    out.set_fields(0, bases)
    assert _flags(out)[4] == dense + len(vocab)
    plain = engine.Matrix.from_csr(got[0], got[1], got[2], out.p, got[3])
    rng = np.random.default_rng(5)
    w, v = rng.normal(0, 0.1, out.p), rng.normal(0, 0.1, (4, out.p))
    params = []
    for mat in (out, plain):
        e = engine.Engine(out.p, mode=L.MODE_MINIBATCH, batch_rows=256, num_factor=4, task=L.TASK_CLASSIFICATION, learn_rate=0.05)
        e.set_params(0.1, w, v)
        for b in range(5):
            e.step(mat, b)
        e.sync()
        params.append(e.get_params())
        e.close()
    assert params[0][0] == params[1][0] and np.array_equal(params[0][1].view(np.uint64), params[1][1].view(np.uint64))
    assert np.array_equal(params[0][2].view(np.uint64), params[1][2].view(np.uint64)) and np.any(params[0][1] != w)
    for mat in (m, out, plain):
        mat.close()


# ------------------------------------------------------------------------------------------------------------------------- the refusals
def test_refusals_that_need_a_matrix_write_nothing():
    from fmwr_amd import _lib as L, engine
    lib = L.lib()
    m, host, p = _source("mixed")
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    edges, n_edges, count, rng = np.full((2, 3), 7.0, np.float32), np.full(2, 7, np.int32), np.full((2, 2), 7, np.int64), np.full((2, 2), 7.0, np.float32)
    for bad in ([1, p], [p, p + 1], [0, 0xFFFFFFFF]):
        cols = np.array(bad, np.uint32)
        assert lib.fmx_matrix_column_quantiles(m.h, p_(cols), 2, 4, p_(edges), p_(n_edges), p_(count), p_(rng)) == L.ERR_INVALID
        assert b"feature count" in lib.fmx_last_error()
    cols = np.array([3, 1], np.uint32)
    assert lib.fmx_matrix_column_quantiles(m.h, p_(cols), 2, 4, p_(edges), p_(n_edges), p_(count), p_(rng)) == L.ERR_INVALID
    for n_bins in (0, 65537):
        assert lib.fmx_matrix_column_quantiles(m.h, p_(np.array([1, 3], np.uint32)), 2, n_bins, p_(edges), p_(n_edges), p_(count), p_(rng)) == L.ERR_INVALID
    assert np.all(edges == 7) and np.all(n_edges == 7) and np.all(count == 7) and np.all(rng == 7)

    base = np.full(p + 1, 7, np.uint32)

    def apply(mat, cols, off, e, **kw):
        cols, off, e = np.array(cols, np.uint32), np.array(off, np.int64), np.array(e, np.float32)
        spec = L.BinSpec(kw.get("struct_size", C.sizeof(L.BinSpec)), len(cols), cols.ctypes.data, off.ctypes.data, e.ctypes.data, kw.get("reserved", 0))
        h = C.c_void_p(5)
        st = lib.fmx_matrix_bin_columns(mat.h, C.byref(spec), p_(base), C.byref(h))
        assert not h.value
        return st, lib.fmx_last_error().decode()
    for args, kw, word in ((([1, p], [0, 1, 2], [0.5, 1.5]), {}, "feature count"), (([3, 1], [0, 1, 2], [0.5, 1.5]), {}, "ascend"),
                           (([1, 3], [0, 1, 2], [0.5, np.nan]), {}, "NaN"), (([1, 3], [0, 2, 2], [1.5, 0.5]), {}, "ascend"),
                           (([1, 3], [0, 2, 1], [0.5, 1.5]), {}, "descends"), (([1, 3], [1, 1, 2], [0.5, 1.5]), {}, "start at 0"),
                           (([1, 3], [0, 1, 2], [0.5, 1.5]), dict(struct_size=44), "struct_size"), (([1, 3], [0, 1, 2], [0.5, 1.5]), dict(reserved=-1), "reserved")):
        st, msg = apply(m, *args, **kw)
        assert st == L.ERR_INVALID and word in msg, (args, kw, msg)
    # the widths: 2^32 - 10 features and one column of 20 edges make 2^32 + 11 ids
    big = engine.Matrix.from_csr(np.array([0, 1], np.int64), np.array([5], np.uint32), np.array([1.5], np.float32), 2**32 - 10)
    st, msg = apply(big, [5], [0, 20], np.arange(20))
    assert st == L.ERR_INVALID and "2^32 - 2" in msg
    big.close()
    assert np.all(base == 7)
    out, nb = m.bin_columns([1, 3], [[0.5], [1.5]])         # and the good call is taken
    assert nb[-1] == p + 4
    out.close()


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_binning_lets_the_model_learn_a_non_monotone_effect():
    """The planted problem of DESIGN.md section 28: y = 1[|x| < 0.6], x ~ N(0, 1).  fm_split -> fm_bin_features(bins = 8) on the train part ->
    fm_train -> fm_apply_bins -> fm_metrics, five seeds (of the split and the initialisation), against the same pipeline on the raw value.  The
    bar: the lowest binned AUC exceeds the highest raw one by more than ten times the five-seed spread of either."""
    import fmwr_amd as fm
    rng = np.random.default_rng(21)
    x = rng.normal(0, 1, 20000).astype(np.float32)
    x[x == 0] = 1e-3                                         # (a dense array's zeros would not be stored)
    data = fm.fm_matrix(x.reshape(-1, 1).astype(np.float64), (np.abs(x) < 0.6).astype(np.float64), feature_names=["x"])
    train, test, _ = fm.fm_split(data, test_fraction=0.5, seed=3)
    binned, binning = fm.fm_bin_features(train, [0], bins=8)
    assert binning.new_p == 9 and binned.dim == (train.dim[0], 9) and binned.feature_names[-1] == "x[nan]" and len(binning.unbinned) == 0
    e = binning.edges[0]
    tv = train.features["value"].astype(np.float32)
    ref_e, ref_n, _, _ = bm.column_quantiles(np.zeros(len(tv), np.int64), tv, [0], 8)
    assert ref_n[0] == 7 and np.array_equal(bc.bits(e), bc.bits(ref_e[0]))
    assert np.array_equal(binned.features["col_idx"], np.searchsorted(e, tv, side="right")) and np.all(binned.features["value"] == 1.0)
    test_b = fm.fm_apply_bins(test, binning)
    assert np.array_equal(test_b.features["col_idx"], np.searchsorted(e, test.features["value"].astype(np.float32), side="right"))
    width, wb = fm.fm_bin_features(train, [0], bins=8, method="width")
    lo, hi = np.float64(tv.min()), np.float64(tv.max())
    assert np.array_equal(bc.bits(wb.edges[0]), bc.bits((lo + (hi - lo) * np.arange(1, 8) / 8).astype(np.float32)))
    own, ob = fm.fm_bin_features(train, [0], edges={0: [-0.6, 0.6]})
    assert ob.new_p == 4 and own.feature_names == ["x[<-0.6]", "x[-0.6,0.6)", "x[>=0.6]", "x[nan]"]
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 2}), fm.solver_control(max_iter=20000, solver=fm.SGD_solver(learn_rate=0.1))]
    raw, cut = [], []
    for seed in (1, 2, 3, 4, 5):                             # the seed draws the split and initialises the model: with one split the five AUCs are one number
        tr, te, _ = fm.fm_split(data, test_fraction=0.5, seed=seed)
        tr_b, bn = fm.fm_bin_features(tr, [0], bins=8)
        raw.append(fm.fm_metrics(fm.fm_train(tr, normalize=False, seed=seed, control=ctl), te, normalize=False)["pooled"]["auc"])
        cut.append(fm.fm_metrics(fm.fm_train(tr_b, normalize=False, seed=seed, control=ctl), fm.fm_apply_bins(te, bn), normalize=False)["pooled"]["auc"])
    spread = max(max(raw) - min(raw), max(cut) - min(cut))
    print(f"AUC raw {raw} binned {cut} spread {spread:.4f}")
    assert min(cut) - max(raw) > 10 * spread
