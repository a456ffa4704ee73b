"""fmx_matrix_column_stats / fmx_column_map_select / fmx_column_map_hash / fmx_matrix_remap_columns and fm_feature_stats / fm_prune_features /
fm_hash_features / fm_apply_columns against the numpy model of the definition (tests/columns_model.py).  Counts, maps and remapped matrices are
integers and copied bits, and the sums have one stated order: every comparison is exact equality, in every form and on its boundaries (the hook
lowers the lane-group limit to 4 and 8 entries, the launches to 8 entries and 16 rows, and forces each form)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import columns_model as cm
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

LENS = [0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1025]
# fmx_debug_columns_limits' arguments: (group_entries, chunk_entries, rows_per_launch)
HOOKS = {"default": (0, 0, 0), "g4": (4, 8, 16), "g8": (8, 1024, 16), "g16": (16, 0, 0), "g32": (32, 0, 0), "long": (-1, 8, 16)}
FIELD_VOCAB = [50, 40, 30, 7]
_cache = {}


def _limits(group=0, chunk=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_columns_limits(group, chunk, rows))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _flags(m):
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    return dict(rows_sorted=int(out[0]), unit_values=int(out[1]), fixed_row_len=int(out[2]), max_row_len=int(out[3]), fields=int(out[4]))


def _ragged(p, unit, seed, lens=None, sorted_rows=False):
    """rows of LENS' lengths and a few more, columns drawn with replacement (collisions and duplicates are the rule), one column stored twice on purpose"""
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.concatenate([LENS, rng.integers(0, 10, 26)])) if lens is None else np.asarray(lens)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    if sorted_rows:
        col = np.concatenate([np.sort(rng.choice(p, int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)])
    else:
        col = rng.integers(0, p, int(rp[-1]))
        for r in np.flatnonzero(lens >= 3)[:5]:
            col[rp[r] + 2] = col[rp[r]]
    val = np.ones(len(col), np.float32) if unit else (rng.normal(0, 2, len(col)) * rng.choice([1, 0.125, -3.5], len(col))).astype(np.float32)
    y = np.where(rng.random(len(lens)) < 0.4, 1.0, -1.0).astype(np.float32)
    return rp, col.astype(np.uint32), val, y


def _source(name):
    """(Matrix, host arrays, labels?) -- made once, shared, never changed"""
    from fmwr_amd import engine
    if name in _cache:
        return _cache[name]
    labels = True
    if name.startswith("ragged"):         # ragged_<p>_<real|unit>_<lab|unl>
        _, p, kind, lab = name.split("_")
        labels = lab == "lab"
        host = _ragged(int(p), kind == "unit", 5 + int(p))
        m = engine.Matrix.from_csr(host[0], host[1], host[2], int(p), host[3] if labels else None)
    elif name == "sorted_unit":           # strictly ascending one-hot rows: the stats' unit form by default
        host = _ragged(1000, True, 3, lens=np.random.default_rng(1).permutation(np.concatenate([LENS[:-1], np.arange(1, 12)])), sorted_rows=True)
        m = engine.Matrix.from_csr(host[0], host[1], host[2], 1000, host[3])
    elif name == "fixed":                 # every row of six entries
        host = _ragged(64, False, 8, lens=np.full(45, 6))
        m = engine.Matrix.from_csr(host[0], host[1], host[2], 64, host[3])
    elif name == "fields":                # a field layout: one id of each of four fields per row, no dense columns
        m = engine.Matrix.synthetic_fields(2000, 0, FIELD_VOCAB, 1.1, 9)
        host = m.export()
    else:
        raise KeyError(name)
    if not labels:
        host = (host[0], host[1], host[2], None)
    _cache[name] = (m, host, labels)
    return _cache[name]


RAGGED = [f"ragged_{p}_{kind}_{lab}" for p, kind, lab in ((1, "real", "lab"), (7, "real", "lab"), (7, "unit", "unl"), (64, "real", "unl"), (64, "unit", "lab"),
                                                          (1000, "real", "lab"), (1000, "unit", "lab"))]
SOURCES = RAGGED + ["sorted_unit", "fixed", "fields"]


def _stats_model(name):
    if ("stats", name) not in _cache:
        m, host, _ = _source(name)
        _cache[("stats", name)] = cm.column_stats(host[0], host[1], host[2], host[3], m.p)
    return _cache[("stats", name)]


# ------------------------------------------------------------------------------------------------------------------------------ stats
@pytest.mark.parametrize("name", SOURCES)
def test_stats_equal_the_model_in_every_form(name):
    m, host, labels = _source(name)
    ref_count, ref_value = _stats_model(name)
    dc, dv = DevBuf(m.p * 3, np.int64), DevBuf(m.p * 2, np.float64)
    seen = []
    for what, hook in (("default", (0, 0, 0)), ("second call", (0, 0, 0)), ("chunks of 8", (0, 8, 16)), ("chunks of 1 024", (0, 1024, 16)), ("sorted form forced", (-1, 0, 0)),
                       ("sorted form forced, chunks of 8", (-1, 8, 16))):
        _limits(*hook)
        count, value = m.column_stats()
        assert count.dtype == np.int64 and np.array_equal(count, ref_count), (name, what, "counts")
        assert np.array_equal(value.view(np.uint64), ref_value.view(np.uint64)), (name, what, "sums")
        m.column_stats_device(dc.ptr, dv.ptr)
        assert np.array_equal(dc.numpy().reshape(-1, 3), ref_count), (name, what, "counts, device form")
        assert np.array_equal(dv.numpy().view(np.uint64).reshape(-1, 2), ref_value.view(np.uint64)), (name, what, "sums, device form")
        only, none = m.column_stats(values=False)
        assert none is None and np.array_equal(only, ref_count), (name, what, "counts alone")
        seen.append(value)
    assert all(np.array_equal(v.view(np.uint64), seen[0].view(np.uint64)) for v in seen)
    assert np.all(ref_count[:, 1] <= ref_count[:, 0]) and (labels or not ref_count[:, 2].any())
    # within entries * 2^-53 * sum |term| of the exactly rounded sums (the bar of sections 23 and 25)
    order = np.argsort(host[1], kind="stable")
    x = host[2][order].astype(np.float64)
    off = np.searchsorted(host[1][order], np.arange(m.p + 1))
    worst = 0.0
    for j in range(m.p):
        xs = x[off[j]:off[j + 1]]
        for got, terms in ((seen[0][j, 0], xs), (seen[0][j, 1], xs * xs)):
            bar = len(terms) * 2.0**-53 * math.fsum(np.abs(terms))
            err = abs(got - math.fsum(terms))
            assert err <= bar, (name, j)
            worst = max(worst, err / bar if bar else 0.0)
    print(f"column_stats {name}: largest share of the bar {worst:.3g}")
    if "unit" in name or name == "fields":
        assert np.array_equal(seen[0][:, 0], ref_count[:, 0].astype(np.float64)) and np.array_equal(seen[0][:, 1], seen[0][:, 0])


# ----------------------------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("by", [cm.BY_ROWS, cm.BY_ENTRIES])
@pytest.mark.parametrize("rare", [cm.RARE_DROP, cm.RARE_BUCKET])
def test_select_equals_the_model(by, rare):
    from fmwr_amd import engine
    m, host, _ = _source("fields")
    count, _ = _stats_model("fields")
    p = m.p
    bases = np.concatenate([[0], np.cumsum(FIELD_VOCAB)]).astype(np.uint32)
    dc, dm = DevBuf.from_numpy(count), DevBuf(p, np.uint32)
    c = count[:, 1 if by == cm.BY_ROWS else 0]
    cases = 0
    for mn, mx, prefix, base in itertools.product((0, 1, 2, 5), (0, 3), (0, 3), (None, bases)):
        survivors = int(((np.arange(p) >= prefix) & (c >= mn) & ((c <= mx) | (mx == 0))).sum())
        for cap in sorted({0, 1, max(survivors - 1, 1), max(survivors, 1), survivors + 1}):
            rule = dict(by=by, min_count=mn, max_count=mx, max_features=cap, keep_prefix=prefix, rare=rare, segment_base=base)
            ref, ref_p, ref_nsb = cm.map_select(p, count, **rule)
            got, new_p, nsb = engine.column_map_select(p, count, **rule)
            assert got.dtype == np.uint32 and np.array_equal(got, ref) and new_p == ref_p and np.array_equal(nsb, ref_nsb), rule
            dev_p, dev_nsb = engine.column_map_select_device(p, dc.ptr, dm.ptr, **rule)
            assert np.array_equal(dm.numpy(), ref) and dev_p == ref_p and np.array_equal(dev_nsb, ref_nsb), ("device form", rule)
            cases += 1
    assert cases >= 96
    ragged, _ = _stats_model("ragged_1_real_lab")      # one column
    for mn in (0, 2000):
        ref = cm.map_select(1, ragged, by, mn, 0, 0, 0, rare, None)
        got = engine.column_map_select(1, ragged, by=by, min_count=mn, rare=rare)
        assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2])


# ------------------------------------------------------------------------------------------------------------------------------- hash
def test_hash_equals_the_model():
    from fmwr_amd import engine
    p = 1000
    dm = DevBuf(p, np.uint32)
    for nb, seed, prefix in itertools.product((1, 2, 3, 2**20), (0, 977), (0, 13)):
        ref, ref_p = cm.map_hash(p, nb, seed, 3, prefix)
        got, new_p = engine.column_map_hash(p, nb, seed=seed, salt=3, keep_prefix=prefix)
        assert got.dtype == np.uint32 and np.array_equal(got, ref) and new_p == ref_p == prefix + nb, (nb, seed, prefix)
        assert engine.column_map_hash_device(p, nb, dm.ptr, seed=seed, salt=3, keep_prefix=prefix) == ref_p
        assert np.array_equal(dm.numpy(), ref), ("device form", nb, seed, prefix)
    assert len(engine.column_map_hash(0, 4)[0]) == 0


# ------------------------------------------------------------------------------------------------------------------------------ remap
def _maps(name):
    """the maps of one source: select maps under DROP and BUCKET, hash maps, all dropped, the identity, one survivor"""
    m, host, _ = _source(name)
    p = m.p
    count, _ = _stats_model(name)
    busiest = int(np.argmax(count[:, 0]))
    one = np.full(p, cm.DROP, np.uint32); one[busiest] = 0
    base = np.concatenate([[0], np.cumsum(FIELD_VOCAB)]) if name == "fields" else ([0, p // 2, p] if p > 1 else None)
    cut = int(np.median(count[count[:, 1] > 0, 1])) + 1 if count[:, 1].any() else 1
    return {"select_drop": cm.map_select(p, count, min_count=cut, rare=cm.RARE_DROP)[:2],
            "select_bucket": cm.map_select(p, count, min_count=cut, rare=cm.RARE_BUCKET, segment_base=base)[:2],
            "hash3": cm.map_hash(p, 3, 5), "hash_wide": cm.map_hash(p, 2**20, 6, keep_prefix=min(2, p)),
            "all_drop": (np.full(p, cm.DROP, np.uint32), 4), "identity": (np.arange(p, dtype=np.uint32), p), "one": (one, 1)}


def _same(out, ref, host, what):
    rp, col, val, y = out.export()
    assert out.n == len(host[0]) - 1 and out.nnz == int(ref[0][-1]), what
    assert np.array_equal(rp, ref[0]), (what, "row_ptr")
    assert np.array_equal(col, ref[1]), (what, "col")
    assert np.array_equal(val.view(np.uint32), ref[2].view(np.uint32)), (what, "value bits")
    if host[3] is not None:
        assert np.array_equal(y.view(np.uint32), host[3].view(np.uint32)), (what, "label bits")
    else:
        assert not y.any(), (what, "labels of an unlabelled matrix")
    f = _flags(out)
    lens = np.diff(ref[0])
    sorted_rows = all(np.all(np.diff(ref[1][ref[0][r]:ref[0][r + 1]].astype(np.int64)) > 0) for r in range(out.n))
    assert f["rows_sorted"] == int(sorted_rows), (what, "rows_sorted")
    assert f["unit_values"] == int(np.all(ref[2] == 1.0)), (what, "unit_values")
    assert f["max_row_len"] == (int(lens.max()) if len(lens) else 0), (what, "max_row_len")
    assert f["fixed_row_len"] == (int(lens[0]) if len(lens) and lens[0] > 0 and np.all(lens == lens[0]) else 0), (what, "fixed_row_len")


@pytest.mark.parametrize("combine", [cm.COMBINE_KEEP, cm.COMBINE_SUM, cm.COMBINE_FIRST])
@pytest.mark.parametrize("name", SOURCES)
def test_remap_equals_the_model_in_every_form(name, combine):
    m, host, _ = _source(name)
    hooks = list(HOOKS) if name in ("ragged_7_real_lab", "ragged_1000_real_lab", "ragged_64_unit_lab", "fields") else ["default", "g8", "long"]
    maps = _maps(name)
    if name == "fields":
        maps = {k: maps[k] for k in ("select_bucket", "hash3", "identity")}
    for mname, (cmap, new_p) in maps.items():
        ref = cm.remap(host[0], host[1], host[2], cmap, new_p, combine)
        dmap = DevBuf.from_numpy(cmap)
        for hook in hooks if combine != cm.COMBINE_KEEP else ["default", "g4"]:
            _limits(*HOOKS[hook])
            out = m.remap_columns(cmap, new_p, combine)
            assert out.p == new_p and out.n == m.n
            _same(out, ref, host, (name, mname, combine, hook))
            out.close()
            dev = m.remap_columns_device(dmap.ptr, new_p, combine)
            _same(dev, ref, host, (name, mname, combine, hook, "device form"))
            dev.close()
        if combine != cm.COMBINE_KEEP:
            for r in range(m.n):
                assert np.all(np.diff(ref[1][ref[0][r]:ref[0][r + 1]].astype(np.int64)) > 0)


def test_remap_per_field_buckets_keep_the_field_layout():
    m, host, _ = _source("fields")
    count, _ = _stats_model("fields")
    base = np.concatenate([[0], np.cumsum(FIELD_VOCAB)])
    cut = int(np.median(count[:, 1])) + 1           # about half of every field's ids go to the field's bucket
    cmap, new_p, nsb = cm.map_select(m.p, count, min_count=cut, rare=cm.RARE_BUCKET, segment_base=base)
    assert new_p == int((count[:, 1] >= cut).sum()) + 4 < m.p and _flags(m)["fields"] == 4
    for combine in (cm.COMBINE_FIRST, cm.COMBINE_KEEP, cm.COMBINE_SUM):
        out = m.remap_columns(cmap, new_p, combine)
        f = _flags(out)
        assert f["unit_values"] == 1 and f["fixed_row_len"] == 4 and f["rows_sorted"] == 1, combine
        out.set_fields(0, nsb)                       # accepted: one id of every field's new range per row
        assert _flags(out)["fields"] == 4
        rp, col, val, _ = out.export()
        assert np.all(np.diff(rp) == 4) and np.all(val == 1.0)
        ids = col.reshape(-1, 4).astype(np.int64)
        assert np.all((ids >= nsb[:-1]) & (ids < nsb[1:]))
        out.close()


def test_remap_refuses_a_map_value_out_of_range_in_both_forms():
    from fmwr_amd import _lib as L
    m, host, _ = _source("ragged_64_real_unl")
    count, _ = _stats_model("ragged_64_real_unl")
    absent = np.flatnonzero(count[:, 0] == 0)
    for j, bad in ((int(np.argmax(count[:, 0])), 64), (20, 0xFFFFFFFE), (int(absent[0]) if len(absent) else 3, 70)):
        cmap = np.arange(64, dtype=np.uint32)
        cmap[j] = bad
        d = DevBuf.from_numpy(cmap)
        for combine in (cm.COMBINE_KEEP, cm.COMBINE_SUM, cm.COMBINE_FIRST):
            h = C.c_void_p(1)
            assert L.lib().fmx_matrix_remap_columns(m.h, cmap.ctypes.data_as(C.c_void_p), 64, combine, C.byref(h)) == L.ERR_INVALID and not h.value
            assert f"map[{j}]".encode() in L.lib().fmx_last_error()
            h = C.c_void_p(1)
            assert L.lib().fmx_matrix_remap_columns_device(m.h, d.ptr, 64, combine, C.byref(h)) == L.ERR_INVALID and not h.value
            assert f"map[{j}]".encode() in L.lib().fmx_last_error()
    with pytest.raises(ValueError):
        m.remap_columns(np.arange(63), 64)
    with pytest.raises(ValueError):
        m.remap_columns(np.arange(64) - 1, 64)
    with pytest.raises(L.FmxError):
        m.remap_columns(np.arange(64), 64, combine=3)


# ----------------------------------------------------------------------------------------------------------------- forward invariance
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("k", [0, 3, 16])
def test_predict_is_invariant_under_an_injective_relabelling(k, fp64):
    """KEEP under an injective map that drops nothing: the same rows, entries in the same order, other ids.  The engine whose rows were moved
    along (fmx_get_rows -> fmx_set_rows) gives the same bits."""
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(11)
    for name, mapper in (("ragged_64_real_unl", lambda p: (rng.permutation(p + 3)[:p], p + 3)), ("sorted_unit", lambda p: (2 * np.arange(p) + 1, 2 * p + 1))):
        m, host, _ = _source(name)
        p = m.p
        cmap, new_p = mapper(p)
        cmap = cmap.astype(np.uint32)
        out = m.remap_columns(cmap, new_p, cm.COMBINE_KEEP)
        ref = cm.remap(host[0], host[1], host[2], cmap, new_p, cm.COMBINE_KEEP)
        assert np.array_equal(out.export()[1], ref[1]) and np.array_equal(ref[0], host[0])
        kw = dict(mode=L.MODE_MINIBATCH, batch_rows=64, state_fp64=int(fp64), num_factor=k, task=L.TASK_CLASSIFICATION, learn_rate=0.05)
        a, b = engine.Engine(p, **kw), engine.Engine(new_p, **kw)
        a.set_params(0.2, rng.normal(0, 0.3, p), rng.normal(0, 0.3, (k, p)))
        b.set_params(0.2, np.zeros(new_p), np.zeros((k, new_p)))
        ids = np.arange(p, dtype=np.uint32)
        w, v = a.get_rows(ids)
        b.set_rows(cmap, w, v)
        ya, yb = a.predict(m), b.predict(out)
        assert np.array_equal(ya.view(np.uint64), yb.view(np.uint64)), (name, k, fp64)
        assert np.any(ya != 0.2)
        out.close()


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _planted(n=1200, p=60, rare=40, seed=13):
    """labels from a planted linear model on p common features; `rare` more features occur once each and carry nothing"""
    rng = np.random.default_rng(seed)
    X = sp.random(n, p, density=0.15, random_state=3, format="csr")
    X.data = rng.normal(0, 1, X.nnz).astype(np.float32).astype(np.float64)
    y = np.where(X @ rng.normal(0, 1, p) + rng.normal(0, 0.5, n) > 0, 1.0, 0.0)
    R = sp.csr_matrix((np.ones(rare), (rng.choice(n, rare, replace=False), np.arange(rare))), shape=(n, rare))
    X = sp.hstack([X, R]).tocsr()
    X.sort_indices()
    return X, y


def test_prune_and_hash_pipelines_keep_the_auc():
    """fm_split -> fm_prune_features / fm_hash_features -> fm_train -> fm_apply_columns -> fm_metrics against the same pipeline without the
    column step.  The bar is measured here, not fixed in advance: the unpruned pipeline's AUC over five initialisation seeds gives the
    run-to-run spread, and a column pipeline may fall below the lowest of them by at most that spread."""
    import fmwr_amd as fm
    X, y = _planted()
    data = fm.fm_matrix(X, y)
    train, test, _ = fm.fm_split(data, test_fraction=0.25, seed=3)
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=4000, solver=fm.SGD_solver())]

    def auc(tr, te, seed):
        fit = fm.fm_train(tr, normalize=False, seed=seed, control=ctl)
        return fm.fm_metrics(fit, te, normalize=False)["pooled"]["auc"], fit

    plain = [auc(train, test, s)[0] for s in (1, 2, 3, 4, 5)]
    spread = max(plain) - min(plain)
    floor = min(plain) - spread
    stats = fm.fm_feature_stats(train)
    host = sp.csr_matrix((train.features["value"], train.features["col_idx"], np.concatenate([[0], np.cumsum(train.features["row_size"])])), shape=train.dim)
    assert np.array_equal(stats["rows"], np.diff(host.tocsc().indptr)) and np.array_equal(stats["entries"], stats["rows"])
    assert np.array_equal(stats["positive_rows"], np.diff(host[np.flatnonzero(train.labels > 0)].tocsc().indptr))

    pruned, cmap = fm.fm_prune_features(train, min_rows=2, rare="bucket")
    keep = stats["rows"] >= 2
    assert cmap.new_p == keep.sum() + 1 and pruned.dim == (train.dim[0], cmap.new_p) and np.array_equal(cmap.carried, keep)
    assert np.array_equal(cmap.map[keep], np.arange(keep.sum())) and np.all(cmap.map[~keep] == keep.sum())
    assert pruned.feature_names[-1] == "rare1" and pruned.feature_names[:3] == train.feature_names[:3]
    a_pruned, fit = auc(pruned, fm.fm_apply_columns(test, cmap), 1)
    # the same model, trained before the map was known and moved into its space: the survivors keep their rows
    moved = fm.fm_remap_model(auc(train, test, 1)[1], cmap)
    a_moved = fm.fm_metrics(moved, fm.fm_apply_columns(test, cmap), normalize=False)["pooled"]["auc"]

    # The bucket count.  Hashing p features into B buckets makes about p^2 / (2 B) pairs of features share a bucket and its parameters: a loss
    # the definition brings, not the code (the map is the model's, bit for bit).  At B = 4 p that is a dozen pairs of the 100 features, seen as
    # 0.0065 of AUC on this problem when it was tried; at B = 2^16 it is 0.08 pairs, and the map of this seed is injective on the features (checked
    # below), so the hashed pipeline is the unpruned one under other ids and another draw of V0: what the run-to-run figure measures.
    buckets = 2**16
    hashed, hmap = fm.fm_hash_features(train, buckets, seed=5)
    assert hashed.dim == (train.dim[0], buckets) and np.array_equal(hmap.map, cm.map_hash(train.dim[1], buckets, 5)[0])
    assert len(np.unique(hmap.map)) == train.dim[1] and hashed.features["size"] == train.features["size"]
    a_hashed, _ = auc(hashed, fm.fm_apply_columns(test, hmap), 1)
    print(f"AUC unpruned {plain} spread {spread:.4f} floor {floor:.4f}; pruned {a_pruned:.4f}, model moved {a_moved:.4f}, hashed {a_hashed:.4f}")
    assert a_pruned >= floor and a_hashed >= floor and a_moved >= floor
    dropped, dmap = fm.fm_prune_features(train, min_rows=2, rare="drop")
    assert dropped.dim[1] == keep.sum() and dropped.feature_names == [f for f, k in zip(train.feature_names, keep) if k]
    assert dropped.features["size"] == int(stats["entries"][keep].sum())
