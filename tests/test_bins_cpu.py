"""CPU-side checks of the value-binning surface (fmx_matrix_column_quantiles, fmx_matrix_bin_columns; fmwr_amd.fm_bin_features / fm_apply_bins):
the numpy model of the definition (tests/bins_model.py) against a brute-force restatement with Python's sorted, bisect and integers, the
consequences include/fmx.h states, the declared surface, and the argument checks, which run before any device."""
import bisect
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import bins_cases as bc
from tests import bins_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_matrix_column_quantiles", "fmx_matrix_bin_columns")


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


def _fit_brute(values, n_bins):
    """include/fmx.h's wording in Python floats and integers: (edges, cnt, nans, lo, hi)"""
    xs = [float(x) for x in values]
    L = sorted(0.0 if x == 0 else x for x in xs if x == x)          # -0 read as +0; Python orders floats as the key does
    cnt = len(L)
    if cnt == 0:
        return [], 0, len(xs), 0.0, 0.0
    cand = [L[(b * cnt) // n_bins] for b in range(1, n_bins)]
    return sorted({c for c in cand if c > L[0]}), cnt, len(xs) - cnt, L[0], L[-1]


def _bin_brute(x, edges):
    return len(edges) + 1 if x != x else bisect.bisect_right(edges, x)


# ------------------------------------------------------------------------------------------------------------------------- the order key
def test_vkey_orders_floats_with_nan_last_and_inverts():
    x = np.concatenate([bc.EDGE_VALUES, bc.NANS, np.array([-3.5, -1e-45, 1e-45, 1e38, -1e38, 0.5], np.float32)])
    k = bm.vkey(x)
    assert np.all(k[np.isnan(x)] == 0xFFFFFFFF) and bm.vkey(np.float32([np.inf]))[0] == 0xFF800000
    assert bm.vkey(np.float32([-0.0]))[0] == bm.vkey(np.float32([0.0]))[0] == 0x80000000
    real = ~np.isnan(x)
    for a, ka in zip(x[real], k[real]):
        for b, kb in zip(x[real], k[real]):
            assert (a < b) == (ka < kb) and (a == b) == (ka == kb)
    back = bm.unkey(k[real])
    assert np.array_equal(back, x[real]) and not np.any(np.signbit(back[back == 0]))     # -0 comes back as +0


# ------------------------------------------------------------------------------------------------------------------------------ the fit
@pytest.mark.parametrize("n_bins", [1, 2, 3, 8, 10, 256, 65536])
def test_fit_model_against_brute_force(n_bins):
    rp, col, val, _ = bc.mixed()
    cols = np.arange(bc.P)
    edges, n_edges, count, rng = bm.column_quantiles(col, val, cols, n_bins)
    assert edges.shape == (bc.P, n_bins - 1)
    for s, c in enumerate(cols):
        e, cnt, nans, lo, hi = _fit_brute(val[col == c], n_bins)
        assert n_edges[s] == len(e) and count[s].tolist() == [cnt, nans]
        assert np.array_equal(bc.bits(edges[s, :len(e)]), bc.bits(np.array(e, np.float32)))
        assert not edges[s, len(e):].view(np.uint32).any()                              # the padding is +0.0
        assert np.array_equal(bc.bits(rng[s]), bc.bits(np.array([lo, hi], np.float32)))
    assert count[4].tolist() == [0, 0] and count[6, 0] == 0 and count[6, 1] > 0 and count[5, 1] > 0
    assert n_edges[3] == 0 and n_edges[4] == 0 and n_edges[6] == 0                       # all equal, empty, NaN alone: one bin
    if n_bins >= 256:               # more bins than entries: every stored value is a candidate
        assert n_edges[2] == 5      # {-inf, 0, 1e-45, 3, +inf} with -0 and +0 one value: -1, 0, 1e-45, 3, +inf lie above L[0]
        assert edges[2, :5].tolist() == [-1.0, 0.0, float(np.float32(1e-45)), 3.0, math.inf]
        assert not np.signbit(edges[2, 1])


def test_apply_model_against_brute_force():
    rp, col, val, _ = bc.mixed()
    cols = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9])
    fit, n_edges, _, _ = bm.column_quantiles(col, val, cols, 8)
    edges = [fit[s, :n_edges[s]] for s in range(len(cols))]
    edges[0] = np.array([-np.inf, 0.0, np.inf], np.float32)                             # hand-made, with infinite edges
    edges[8] = np.zeros(0, np.float32)                                                  # no edges: one bin and the NaN id
    ocol, oval, base = bm.bin_columns(col, val, bc.P, cols, edges)
    width = [1] * bc.P
    for c, e in zip(cols, edges):
        width[c] = len(e) + 2
    assert base.tolist() == [sum(width[:j]) for j in range(bc.P + 1)]
    slot = {int(c): s for s, c in enumerate(cols)}
    for i in range(len(col)):
        c, x = int(col[i]), float(val[i])
        if c in slot:
            e = [float(t) for t in edges[slot[c]]]
            assert ocol[i] == base[c] + _bin_brute(x, e) and oval[i] == 1.0
        else:
            assert ocol[i] == base[c] and bc.bits(oval[i:i + 1])[0] == bc.bits(val[i:i + 1])[0]
    assert np.all(ocol < base[-1])
    # -inf is an edge: it lies in bin 1, not below all; +inf lies in the last bin; NaN in the id behind it
    z = np.array([-np.inf, -1.0, -0.0, 0.0, np.inf, np.nan], np.float32)
    zc, _, zb = bm.bin_columns(np.zeros(6, np.int64), z, 1, [0], [edges[0]])
    assert zc.tolist() == [1, 1, 2, 2, 3, 4] and zb.tolist() == [0, 5]


def _random_column(rng):
    n = int(rng.integers(0, 400))
    kind = rng.integers(0, 5)
    if kind == 0:
        x = rng.normal(0, 1, n)
    elif kind == 1:
        x = np.round(rng.normal(0, 2, n))                    # heavy ties
    elif kind == 2:
        x = np.exp(rng.normal(0, 3, n))                      # skewed
    elif kind == 3:
        x = rng.choice(np.concatenate([bc.EDGE_VALUES.astype(np.float64), [1.5, -2.0]]), n)
    else:
        x = rng.permutation(n).astype(np.float64)            # no ties
    x = x.astype(np.float32)
    if n and rng.random() < 0.3:
        x[rng.random(n) < 0.1] = np.nan
    return x


def test_the_consequences_of_the_definition_over_random_cases():
    rng = np.random.default_rng(7)
    for case in range(400):
        x = _random_column(rng)
        n_bins = int(rng.choice([1, 2, 3, 5, 8, 32, 1000]))
        z = np.zeros(len(x), np.int64)
        edges, n_edges, count, rg = bm.column_quantiles(z, x, [0], n_bins)
        e = edges[0, :n_edges[0]]
        real = x[~np.isnan(x)]
        assert count[0].tolist() == [len(real), len(x) - len(real)]
        assert len(e) <= n_bins - 1 and not np.any(np.isnan(e)) and np.all(e[1:] > e[:-1])       # at most n_bins - 1, strictly ascending, none NaN
        b = np.searchsorted(e, real, side="right")
        if len(real):
            assert np.array_equal(np.unique(b), np.arange(len(e) + 1))                         # every bin holds a fitting entry
            order = np.argsort(real, kind="stable")
            assert np.all(np.diff(b[order]) >= 0)                                              # monotone in x (and equal values share a bin)
            assert rg[0, 0] == real.min() and rg[0, 1] == real.max()
            if len(np.unique(real)) == len(real):                                              # without ties: no bin above ceil(cnt / n_bins)
                assert np.bincount(b).max() <= -(-len(real) // n_bins)
        else:
            assert len(e) == 0 and rg[0].tolist() == [0.0, 0.0]
        # any strictly increasing map of the values leaves the assignment as it is
        u, inv = np.unique(real, return_inverse=True)
        target = np.sort(rng.choice(np.arange(-5000, 5000), len(u), replace=False)).astype(np.float32) ** 3
        mapped = x.copy()
        mapped[~np.isnan(x)] = target[inv]
        e2, ne2, _, _ = bm.column_quantiles(z, mapped, [0], n_bins)
        assert ne2[0] == len(e) and np.array_equal(np.searchsorted(e2[0, :ne2[0]], target[inv], side="right"), b)
        # the column's own multiset alone: other columns, the entry order
        perm = rng.permutation(len(x))
        col2 = np.concatenate([np.full(len(x), 3), rng.integers(0, 3, 50), rng.integers(4, 6, 50)])
        val2 = np.concatenate([x[perm], rng.normal(0, 1, 100).astype(np.float32)])
        mix = rng.permutation(len(col2))
        e3, ne3, c3, r3 = bm.column_quantiles(col2[mix], val2[mix], [1, 3, 5], n_bins)
        assert ne3[1] == n_edges[0] and np.array_equal(bc.bits(e3[1]), bc.bits(edges[0]))
        assert np.array_equal(c3[1], count[0]) and np.array_equal(bc.bits(r3[1]), bc.bits(rg[0]))


def test_binning_separates_what_the_raw_value_cannot():
    """the planted problem of DESIGN.md section 28: y = 1[|x| < 0.6].  The raw value does not rank the rows; the per-bin positive rate does"""
    rng = np.random.default_rng(3)
    x, xt = rng.normal(0, 1, 10000).astype(np.float32), rng.normal(0, 1, 10000).astype(np.float32)
    y, yt = np.abs(x) < 0.6, np.abs(xt) < 0.6

    def auc(score, label):
        order = np.argsort(score, kind="stable")
        rank = np.empty(len(score)); rank[order] = np.arange(1, len(score) + 1)
        for v in np.unique(score):                            # mid-ranks for ties
            at = score == v
            rank[at] = rank[at].mean()
        pos = label.sum()
        return (rank[label].sum() - pos * (pos + 1) / 2) / (pos * (len(label) - pos))
    edges, n_edges, _, _ = bm.column_quantiles(np.zeros(len(x), np.int64), x, [0], 8)
    e = edges[0, :n_edges[0]]
    rate = np.array([y[np.searchsorted(e, x, side="right") == b].mean() for b in range(len(e) + 1)])
    assert abs(auc(xt.astype(np.float64), yt) - 0.5) < 0.03
    assert auc(rate[np.searchsorted(e, xt, side="right")], yt) > 0.9


# ------------------------------------------------------------------------------------------------------------------- the declared surface
def test_bin_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and hasattr(L.lib(), name)
        assert name + "_device" not in text                  # there is no _device form
    assert "fmx_debug_bins_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_bins_limits")
    assert "fmx_debug_bins_limits" not in text               # the hook stays out of the public header
    assert header.index("fmx_matrix_stack") < header.index("fmx_matrix_column_quantiles") < header.index("fmx_matrix_bin_columns")
    fields = re.search(r"typedef struct fmx_bin_spec \{(.*?)\} fmx_bin_spec;", header, flags=re.S).group(1)
    declared = [re.sub(r"^.*[\s\*]", "", decl.strip()) for decl in fields.split(";") if decl.strip()]
    assert declared == [f[0] for f in L.BinSpec._fields_]
    assert C.sizeof(L.BinSpec) == 40
    assert L.BINS_MAX_BINS == bm.MAX_BINS == 65536 and L.BINS_MAX_EDGES == bm.MAX_EDGES == 65535
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 28" in design and "Not built" in design.split("## 28")[1]
    import fmwr_amd as fm
    for f in (fm.fm_bin_features, fm.fm_apply_bins, fm.Binning, fm.Matrix.column_quantiles, fm.Matrix.bin_columns):
        assert callable(f)
    assert "fm_bins.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fm_bins.hip")).read()
    assert '#include "fm_prims.h"' in src and "rocprim" not in src     # the sort and the scans come from fm_prims.h


def _spec(L, keep, **kw):
    v = dict(n_cols=2, cols=np.array([1, 3], np.uint32), edge_offset=np.array([0, 2, 3], np.int64), edges=np.array([0.5, 1.5, -2.0], np.float32), reserved=0)
    v.update(kw)
    ptr = {}
    for name in ("cols", "edge_offset", "edges"):
        a = v[name]
        if a is not None:
            keep.append(a)
        ptr[name] = None if a is None else a.ctypes.data
    s = L.BinSpec(C.sizeof(L.BinSpec), v["n_cols"], ptr["cols"], ptr["edge_offset"], ptr["edges"], v["reserved"])
    if "struct_size" in kw:
        s.struct_size = kw["struct_size"]
    return s


def test_refusals_come_before_any_device_and_write_nothing():
    """every refusal that can be seen without the matrix comes before the matrix is looked at: with a NULL matrix the message names the argument"""
    L = _lib()
    lib = L.lib()
    edges = np.full((2, 3), 7.0, np.float32)
    n_edges = np.full(2, 7, np.int32)
    count = np.full((2, 2), 7, np.int64)
    rng = np.full((2, 2), 7.0, np.float32)
    pe, pn, pc, pr = (a.ctypes.data_as(C.c_void_p) for a in (edges, n_edges, count, rng))
    cols = np.array([1, 3], np.uint32)
    pcols = cols.ctypes.data_as(C.c_void_p)

    def fit(m=None, cols=pcols, n_cols=2, n_bins=4, e=pe, n=pn, c=pc, r=pr):
        st = lib.fmx_matrix_column_quantiles(m, cols, n_cols, n_bins, e, n, c, r)
        return st, lib.fmx_last_error().decode()
    for kw, word in ((dict(n_bins=0), "n_bins"), (dict(n_bins=-1), "n_bins"), (dict(n_bins=65537), "n_bins"), (dict(cols=None), "NULL"), (dict(e=None), "NULL"),
                     (dict(n=None), "NULL"), (dict(c=None), "NULL"), (dict(r=None), "NULL"), (dict(n_cols=-1), "n_cols"), (dict(), "NULL matrix"),
                     (dict(e=None, n_bins=1), "NULL matrix")):            # edges may be NULL with one bin: the next check speaks
        st, msg = fit(**kw)
        assert st == L.ERR_INVALID and word in msg, (kw, msg)
    for bad in ([3, 1], [2, 2]):
        a = np.array(bad, np.uint32)
        st, msg = fit(cols=a.ctypes.data_as(C.c_void_p))
        assert st == L.ERR_INVALID and "ascend" in msg
    assert np.all(edges == 7) and np.all(n_edges == 7) and np.all(count == 7) and np.all(rng == 7)

    base = np.full(9, 7, np.uint32)
    pb = base.ctypes.data_as(C.c_void_p)
    keep = []

    def apply(m=None, spec="good", new_base=pb, **kw):
        h = C.c_void_p(5)
        s = _spec(L, keep, **kw) if spec == "good" else spec
        st = lib.fmx_matrix_bin_columns(m, None if s is None else C.byref(s), new_base, C.byref(h))
        assert not h.value
        return st, lib.fmx_last_error().decode()
    f32, i64, u32 = (lambda *a: np.array(a, np.float32)), (lambda *a: np.array(a, np.int64)), (lambda *a: np.array(a, np.uint32))
    many = np.arange(65536, dtype=np.float32)
    for kw, word in ((dict(spec=None), "spec is NULL"), (dict(new_base=None), "new_base"), (dict(struct_size=36), "struct_size"), (dict(reserved=1), "reserved"),
                     (dict(n_cols=-1), "n_cols"), (dict(cols=None), "cols is NULL"), (dict(edge_offset=None), "edge_offset"), (dict(edges=None), "edges is NULL"),
                     (dict(cols=u32(3, 1)), "ascend"), (dict(cols=u32(3, 3)), "ascend"), (dict(edge_offset=i64(1, 2, 3)), "start at 0"),
                     (dict(edge_offset=i64(0, 2, 1)), "descends"), (dict(edges=f32(0.5, np.nan, -2.0)), "NaN"), (dict(edges=f32(0.5, 0.5, -2.0)), "ascend"),
                     (dict(edges=f32(1.5, 0.5, -2.0)), "ascend"), (dict(edges=f32(-0.0, 0.0, -2.0)), "ascend"),
                     (dict(n_cols=1, cols=u32(1), edge_offset=i64(0, 65536), edges=many), "65535"), (dict(), "NULL matrix"),
                     (dict(edges=f32(-np.inf, np.inf, 0.0)), "NULL matrix")):       # infinite edges are allowed: the next check speaks
        st, msg = apply(**kw)
        assert st == L.ERR_INVALID and word in msg, (kw, msg)
    assert lib.fmx_matrix_bin_columns(None, C.byref(_spec(L, keep)), pb, None) == L.ERR_INVALID
    assert np.all(base == 7)
    assert lib.fmx_debug_bins_limits(4, 8) == L.OK and lib.fmx_debug_bins_limits(-1, 0) == L.OK and lib.fmx_debug_bins_limits(0, 0) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    for name in ("_device_matrix", "_engine_for"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api.Matrix, "from_csr", classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    d = fm.fm_matrix(np.random.default_rng(0).random((6, 4)), np.arange(6) % 2)
    for f in (lambda x: fm.fm_bin_features(x, [0]), lambda x: fm.fm_apply_bins(x, None)):
        with pytest.raises(TypeError, match="fm.matrix"):
            f(np.ones((6, 4)))
    for columns in ([[0, 1]], [0.5], [4], [-1]):
        with pytest.raises(ValueError, match="columns must"):
            fm.fm_bin_features(d, columns)
    with pytest.raises(ValueError, match="twice"):
        fm.fm_bin_features(d, [1, 1])
    for bins in (0, 65537, 2.5, True):
        with pytest.raises(ValueError, match="bins must be an integer"):
            fm.fm_bin_features(d, [0], bins=bins)
    with pytest.raises(ValueError, match="method must be"):
        fm.fm_bin_features(d, [0], method="kmeans")
    with pytest.raises(TypeError, match="dict"):
        fm.fm_bin_features(d, [0], edges=[0.5])
    with pytest.raises(ValueError, match="not one of columns"):
        fm.fm_bin_features(d, [0], edges={1: [0.5]})
    for e in ([0.5, 0.5], [1.0, 0.5], [np.nan], [0.0, -0.0], [1.0, 1.0 + 1e-12]):     # (the last pair is one value in single precision)
        with pytest.raises(ValueError, match="ascend strictly"):
            fm.fm_bin_features(d, [0], edges={0: e})
    with pytest.raises(TypeError, match="Binning"):
        fm.fm_apply_bins(d, {"edges": []})
    b = fm.Binning(np.array([1]), [np.array([0.5, 2.0], np.float32)], np.array([0, 1, 5, 6, 7], np.uint32), d.feature_names, ["x"] * 7)
    other = fm.fm_matrix(np.ones((2, 4)), feature_names=["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_apply_bins(other, b)
    assert b.new_p == 7 and b.unbinned.tolist() == [0, 5, 6]
    from fmwr_amd.api import _bin_names
    names = _bin_names(["age", "w", "z"], [0, 2], [np.array([18.5, 31.0], np.float32), np.zeros(0, np.float32)])
    assert names == ["age[<18.5]", "age[18.5,31)", "age[>=31]", "age[nan]", "w", "z[all]", "z[nan]"]
    m = fm.Matrix(None, 3, 4, 0)
    for cols in ([1, 1], [2, 1], [4], [-1], [0.5], [[0]]):
        with pytest.raises(ValueError, match="cols must"):
            m.column_quantiles(cols, 4)
        with pytest.raises(ValueError, match="cols must"):
            m.bin_columns(cols, [np.zeros(0, np.float32)])
    for bins in (0, 65537, 1.5):
        with pytest.raises(ValueError, match="bins must"):
            m.column_quantiles([0], bins)
    with pytest.raises(ValueError, match="one array per column"):
        m.bin_columns([0, 1], [np.zeros(0, np.float32)])
    with pytest.raises(ValueError, match="ascend strictly"):
        m.bin_columns([0], [np.array([1.0, np.nan], np.float32)])
