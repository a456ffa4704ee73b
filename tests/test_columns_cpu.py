"""CPU-side checks of the column-selection surface (fmx_matrix_column_stats, fmx_column_map_select, fmx_column_map_hash, fmx_matrix_remap_columns;
fmwr_amd.fm_feature_stats / fm_prune_features / fm_hash_features / fm_apply_columns / fm_remap_model): the numpy model of the definition
(tests/columns_model.py) against a brute-force restatement in Python integers and math.fsum, the consequences include/fmx.h states, the declared
surface, and the argument checks, which run before any device."""
import ctypes as C
import itertools
import math
import os
import re
import struct

import numpy as np
import pytest

from tests import columns_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_matrix_column_stats", "fmx_matrix_column_stats_device", "fmx_column_map_select", "fmx_column_map_select_device", "fmx_column_map_hash",
         "fmx_column_map_hash_device", "fmx_matrix_remap_columns", "fmx_matrix_remap_columns_device")
M = 2**64 - 1
P = 37


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


def _data(unit=False, seed=1):
    """200 rows over 37 columns: rows of 0, 1, 2 and many entries (one of 2 100: three chunks of the sums in the hot columns), columns stored
    twice (and three times) in a row, negative and fractional values"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0, 1, 2, 0, 2100, 40, 1, 2], rng.integers(0, 12, 192)])
    col = rng.integers(0, P, int(lens.sum()))
    col[(col == 5) | (col == 30)] = 6          # columns 5 and 30 never occur
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for r in (5, 9, 20):                        # a column stored twice and three times in a row
        a = rp[r]
        if rp[r + 1] - a >= 3:
            col[a + 1] = col[a]; col[a + 2] = col[a]
    val = np.ones(len(col), np.float32) if unit else (rng.normal(0, 2, len(col)) * rng.choice([1, 0.125, -3.5], len(col))).astype(np.float32)
    y = np.where(rng.random(len(lens)) < 0.4, 1.0, -1.0).astype(np.float32)
    y[7] = 0.0                                  # not positive
    return rp, col.astype(np.uint32), val, y


def _f2d(x):
    return struct.unpack("d", struct.pack("d", float(x)))[0]


def _tree_brute(terms):
    """include/fmx.h's wording in Python floats, one addition at a time"""
    total = 0.0
    for c0 in range(0, len(terms), 1024):
        chunk = terms[c0:c0 + 1024]
        lane = [0.0] * 64
        for i, t in enumerate(chunk):
            lane[i % 64] = lane[i % 64] + t
        for s in (32, 16, 8, 4, 2, 1):
            lane = [lane[l] + lane[l ^ s] for l in range(64)]
        total = total + lane[0]
    return total


# ------------------------------------------------------------------------------------------------------------------------------ stats
@pytest.mark.parametrize("unit", [False, True])
def test_stats_model_against_brute_force(unit):
    rp, col, val, y = _data(unit)
    count, value = cm.column_stats(rp, col, val, y, P)
    worst = 0.0
    for j in range(P):
        rows = [r for r in range(len(rp) - 1) for e in range(rp[r], rp[r + 1]) if col[e] == j]
        xs = [float(val[e]) for r in range(len(rp) - 1) for e in range(rp[r], rp[r + 1]) if col[e] == j]
        assert count[j, 0] == len(rows)
        assert count[j, 1] == len(set(rows))
        assert count[j, 2] == len({r for r in rows if y[r] > 0})
        assert value[j, 0] == _tree_brute(xs) and value[j, 1] == _tree_brute([x * x for x in xs])
        for got, terms in ((value[j, 0], xs), (value[j, 1], [x * x for x in xs])):
            bar = len(terms) * 2.0**-53 * math.fsum(abs(t) for t in terms)
            err = abs(got - math.fsum(terms))
            assert err <= bar
            worst = max(worst, err / bar if bar else 0.0)
        if unit:
            assert value[j, 0] == value[j, 1] == float(count[j, 0])
    assert np.all(count[:, 1] <= count[:, 0]) and np.all(count[:, 2] <= count[:, 1])
    assert count[5].tolist() == [0, 0, 0] and value[5].tolist() == [0.0, 0.0]
    assert count[:, 0].max() > 64 and (count[:, 0] != count[:, 1]).any()     # several lane rounds, and duplicates inside rows
    assert worst < 1.0
    unl, _ = cm.column_stats(rp, col, val, None, P)
    assert not unl[:, 2].any() and np.array_equal(unl[:, :2], count[:, :2])


def test_a_columns_sums_depend_on_its_own_entries_alone():
    rp, col, val, y = _data()
    _, value = cm.column_stats(rp, col, val, y, P)
    only = col == 6
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    rp1 = np.concatenate([[0], np.cumsum(np.bincount(row[only], minlength=len(rp) - 1))])
    _, alone = cm.column_stats(rp1, col[only], val[only], None, P)      # the other columns gone: the same bits
    assert np.array_equal(alone[6].view(np.uint64), value[6].view(np.uint64))
    assert cm.tree_sum([]) == 0.0 and math.copysign(1.0, cm.tree_sum([-0.0])) == 1.0


# ----------------------------------------------------------------------------------------------------------------------------- select
def _select_brute(p, count, by, min_count, max_count, max_features, keep_prefix, rare, base):
    c = [int(count[j][1 if by == cm.BY_ROWS else 0]) for j in range(p)]
    surv = [j for j in range(keep_prefix, p) if c[j] >= min_count and (max_count == 0 or c[j] <= max_count)]
    if max_features > 0 and len(surv) > max_features:
        surv = sorted(surv, key=lambda j: (-c[j], j))[:max_features]
    surv = set(surv) | set(range(keep_prefix))
    base = [0, p] if base is None else [int(b) for b in base]
    out, nsb, nxt = [cm.DROP] * p, [], 0
    for s in range(len(base) - 1):
        nsb.append(nxt)
        for j in range(base[s], base[s + 1]):
            if j in surv:
                out[j] = nxt; nxt += 1
        if rare == cm.RARE_BUCKET:
            for j in range(base[s], base[s + 1]):
                if j not in surv:
                    out[j] = nxt
            nxt += 1
    nsb.append(nxt)
    return out, nxt, nsb


FIELDS = [0, 3, 3, 10, 22, 37]   # five segments, one of them empty


def test_select_model_against_brute_force_and_its_consequences():
    rp, col, val, y = _data()
    count, _ = cm.column_stats(rp, col, val, y, P)
    count[11] = count[12]; count[13] = count[12]     # ties for the cap
    for by, mn, mx, prefix, rare, base in itertools.product((cm.BY_ROWS, cm.BY_ENTRIES), (0, 1, 2, 5, 60), (0, 3, 70), (0, 3), (cm.RARE_DROP, cm.RARE_BUCKET),
                                                            (None, FIELDS)):
        free, _, _ = cm.map_select(P, count, by, mn, mx, 0, prefix, rare, base)
        c = count[:, 1 if by == cm.BY_ROWS else 0]
        survivors = int(((np.arange(P) >= prefix) & (c >= mn) & ((c <= mx) | (mx == 0))).sum())
        for cap in {0, 1, max(survivors - 1, 1), max(survivors, 1), survivors + 1}:
            got, new_p, nsb = cm.map_select(P, count, by, mn, mx, cap, prefix, rare, base)
            ref, ref_p, ref_nsb = _select_brute(P, count, by, mn, mx, cap, prefix, rare, base)
            what = (by, mn, mx, cap, prefix, rare, base)
            assert got.tolist() == ref and new_p == ref_p and nsb.tolist() == ref_nsb, what
            bounds = [0, P] if base is None else base
            buckets = set()
            for s in range(len(bounds) - 1):
                seg = got[bounds[s]:bounds[s + 1]].astype(np.int64)
                if rare == cm.RARE_BUCKET:
                    bucket = int(nsb[s + 1]) - 1
                    buckets.add(bucket)
                    kept = seg[seg != bucket]
                    assert np.all((seg >= nsb[s]) & (seg <= bucket)), what
                else:
                    kept = seg[seg != cm.DROP]
                assert np.all(np.diff(kept) == 1) and (len(kept) == 0 or kept[0] == nsb[s]), what       # ascending, consecutive
            assert len(buckets) == (len(bounds) - 1 if rare == cm.RARE_BUCKET else 0), what                # exactly one bucket per segment
            assert np.all(got[:prefix] != cm.DROP) and (rare == cm.RARE_BUCKET or np.array_equal(got[:prefix], np.arange(prefix))), what
            if cap >= survivors:
                assert np.array_equal(got, free), what
    # ties at the cap go to the lower id
    tie = np.zeros((6, 3), np.int64)
    tie[:, 1] = [4, 9, 9, 9, 2, 9]
    got, new_p, _ = cm.map_select(6, tie, max_features=2)
    assert got.tolist() == [cm.DROP, 0, 1, cm.DROP, cm.DROP, cm.DROP] and new_p == 2
    got, new_p, _ = cm.map_select(6, tie, max_features=2, keep_prefix=1)
    assert got.tolist() == [0, 1, 2, cm.DROP, cm.DROP, cm.DROP] and new_p == 3     # the prefix is outside the cap


# ------------------------------------------------------------------------------------------------------------------------------- hash
def _mix(x):
    x &= M
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & M
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & M
    x ^= x >> 31
    return x


def _H(seed, salt, t, stream):
    h = _mix(seed + 0x9E3779B97F4A7C15)
    h = _mix(h ^ ((salt * 0xD6E8FEB86659FD93 + stream) & M))
    return _mix(h ^ ((t + 0x632BE59BD9B4E019) & M))


def test_hash_model_against_python_integers():
    for nb, seed, salt, prefix in itertools.product((1, 2, 3, 2**20, 2**32 - 10), (0, 12345), (0, 7), (0, 3)):
        got, new_p = cm.map_hash(P, nb, seed, salt, prefix)
        ref = [j if j < prefix else prefix + ((_H(seed, salt, j, 4) * nb) >> 64) for j in range(P)]
        assert got.tolist() == ref and new_p == prefix + nb
        assert np.all(got[prefix:] >= prefix) and np.all(got.astype(np.int64) < new_p)
        # a function of (seed, salt, j) alone: another feature count reads the same values
        assert np.array_equal(cm.map_hash(20, nb, seed, salt, prefix)[0], got[:20])
    a, b = cm.map_hash(P, 2**20, 1)[0], cm.map_hash(P, 2**20, 2)[0]
    assert not np.array_equal(a, b)
    from tests import split_model as sm
    assert not np.array_equal(sm.H(1, 0, np.arange(P), 4), sm.H(1, 0, np.arange(P), 3))     # stream 4 is a stream of its own


# ------------------------------------------------------------------------------------------------------------------------------ remap
def _remap_brute(rp, col, val, cmap, combine):
    orp, ocol, obits = [0], [], []
    for r in range(len(rp) - 1):
        ent = [(int(cmap[col[e]]), i, val[rp[r] + i]) for i, e in enumerate(range(rp[r], rp[r + 1])) if cmap[col[e]] != cm.DROP]
        if combine == cm.COMBINE_KEEP:
            ocol += [c for c, _, _ in ent]; obits += [x for _, _, x in ent]
        else:
            ent.sort(key=lambda t: (t[0], t[1]))
            for c, grp in itertools.groupby(ent, key=lambda t: t[0]):
                xs = [x for _, _, x in grp]
                ocol.append(c)
                if combine == cm.COMBINE_FIRST:
                    obits.append(xs[0])
                else:
                    acc = float(xs[0])
                    for x in xs[1:]:
                        acc = acc + float(x)
                    obits.append(np.float32(acc))
        orp.append(len(ocol))
    return np.array(orp, np.int64), np.array(ocol, np.uint32), np.array(obits, np.float32)


def _maps():
    rp, col, val, y = _data()
    count, _ = cm.column_stats(rp, col, val, y, P)
    one = np.full(P, cm.DROP, np.uint32); one[6] = 0
    return {"drop": cm.map_select(P, count, min_count=40, rare=cm.RARE_DROP)[:2],
            "bucket": cm.map_select(P, count, min_count=40, rare=cm.RARE_BUCKET, segment_base=FIELDS)[:2],
            "hash3": cm.map_hash(P, 3, 5), "hash_wide": cm.map_hash(P, 2**20, 5, keep_prefix=2),
            "all_drop": (np.full(P, cm.DROP, np.uint32), 4), "identity": (np.arange(P, dtype=np.uint32), P), "one": (one, 1)}


@pytest.mark.parametrize("combine", [cm.COMBINE_KEEP, cm.COMBINE_SUM, cm.COMBINE_FIRST])
def test_remap_model_against_brute_force_and_its_consequences(combine):
    rp, col, val, y = _data()
    for name, (cmap, new_p) in _maps().items():
        orp, ocol, oval = cm.remap(rp, col, val, cmap, new_p, combine)
        brp, bcol, bval = _remap_brute(rp, col, val, cmap, combine)
        assert np.array_equal(orp, brp) and np.array_equal(ocol, bcol) and np.array_equal(oval.view(np.uint32), bval.view(np.uint32)), name
        assert len(orp) == len(rp) and (len(ocol) == 0 or int(ocol.max()) < new_p), name
        if name == "all_drop":
            assert orp[-1] == 0
        for r in range(len(rp) - 1):
            ids = ocol[orp[r]:orp[r + 1]].astype(np.int64)
            if combine != cm.COMBINE_KEEP:
                assert np.all(np.diff(ids) > 0), (name, r)           # strictly ascending: no id twice
            if combine == cm.COMBINE_SUM:
                # a row's sum survives within one fp32 rounding per merged id (of the id's own exact sum)
                src = [(int(cmap[col[e]]), float(val[e])) for e in range(rp[r], rp[r + 1]) if cmap[col[e]] != cm.DROP]
                for t, c in enumerate(ids):
                    exact = math.fsum(x for cc, x in src if cc == c)
                    terms = [x for cc, x in src if cc == c]
                    slack = len(terms) * 2.0**-53 * math.fsum(abs(x) for x in terms)
                    got = float(oval[orp[r] + t])
                    assert abs(got - exact) <= (abs(exact) + slack) * 2.0**-24 + slack + 2.0**-149, (name, r, c)
    ident = np.arange(P, dtype=np.uint32)
    krp, kcol, kval = cm.remap(rp, col, val, ident, P, cm.COMBINE_KEEP)
    assert np.array_equal(krp, rp) and np.array_equal(kcol, col) and np.array_equal(kval.view(np.uint32), val.view(np.uint32))
    with pytest.raises(ValueError):
        cm.remap(rp, col, val, np.full(P, 9, np.uint32), 9, combine)


def test_first_keeps_one_hot_data_one_hot():
    rp, col, val, y = _data(unit=True)
    for name, (cmap, new_p) in _maps().items():
        _, _, oval = cm.remap(rp, col, val, cmap, new_p, cm.COMBINE_FIRST)
        assert np.all(oval == 1.0), name
    _, _, summed = cm.remap(rp, col, val, *_maps()["hash3"], cm.COMBINE_SUM)
    assert summed.max() > 1.0


# ------------------------------------------------------------------------------------------------------------------- the declared surface
def test_column_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_columns_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_columns_limits")
    assert "fmx_debug_columns_limits" not in text   # the hook stays out of the public header
    for name, value, mine in (("COLUMNS_BY_ROWS", 0, cm.BY_ROWS), ("COLUMNS_BY_ENTRIES", 1, cm.BY_ENTRIES), ("RARE_DROP", 0, cm.RARE_DROP),
                              ("RARE_BUCKET", 1, cm.RARE_BUCKET), ("COMBINE_KEEP", 0, cm.COMBINE_KEEP), ("COMBINE_SUM", 1, cm.COMBINE_SUM),
                              ("COMBINE_FIRST", 2, cm.COMBINE_FIRST)):
        assert re.search(r"#define\s+FMX_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(L, name) == value == mine
    assert re.search(r"#define\s+FMX_COLUMN_DROP\s+0xFFFFFFFFu", header) and L.COLUMN_DROP == cm.DROP == 0xFFFFFFFF
    fields = re.search(r"typedef struct fmx_column_rule \{(.*?)\} fmx_column_rule;", header, flags=re.S).group(1)
    declared = [re.sub(r"^.*[\s\*]", "", decl.strip()) for decl in fields.split(";") if decl.strip()]
    assert declared == [f[0] for f in L.ColumnRule._fields_]
    assert C.sizeof(L.ColumnRule) == 56
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 26" in design and "Not built" in design.split("## 26")[1]
    import fmwr_amd as fm
    from fmwr_amd import engine
    for f in (fm.fm_feature_stats, fm.fm_prune_features, fm.fm_hash_features, fm.fm_apply_columns, fm.fm_remap_model, engine.column_map_select,
              engine.column_map_hash):
        assert callable(f)
    for method in ("column_stats", "remap_columns"):
        assert callable(getattr(fm.Matrix, method))
    assert "fm_columns.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES


def _rule(L, **kw):
    v = dict(by=0, min_count=1, max_count=0, max_features=0, keep_prefix=0, rare=0, n_segments=0, reserved=0, segment_base=None)
    v.update(kw)
    r = L.ColumnRule(C.sizeof(L.ColumnRule), v["by"], v["min_count"], v["max_count"], v["max_features"], v["keep_prefix"], v["rare"], v["n_segments"],
                     v["reserved"], v["segment_base"])
    if "struct_size" in kw:
        r.struct_size = kw["struct_size"]
    return r


def test_refusals_come_before_any_device_and_write_nothing():
    L = _lib()
    lib = L.lib()
    count = np.ones((8, 3), np.int64)
    cmap = np.full(8, 7, np.uint32)
    nsb = np.full(4, 7, np.uint32)
    new_p = C.c_uint32(7)
    pc, pm, pn = count.ctypes.data_as(C.c_void_p), cmap.ctypes.data_as(C.c_void_p), nsb.ctypes.data_as(C.c_void_p)
    good = np.array([0, 4, 8], np.uint32)
    bad = [dict(struct_size=12), dict(by=2), dict(by=-1), dict(rare=2), dict(rare=-1), dict(min_count=-1), dict(max_count=-1), dict(max_features=-1),
           dict(keep_prefix=9), dict(reserved=1), dict(n_segments=-1), dict(n_segments=2)]
    for arr in ([1, 4, 8], [0, 4, 7], [0, 5, 4], [0, 9, 8]):
        a = np.array(arr, np.uint32)
        bad.append(dict(n_segments=2, segment_base=a.ctypes.data, _keep=a))
    for kw in bad:
        kw = dict(kw); kw.pop("_keep", None)
        for call in (lib.fmx_column_map_select, lib.fmx_column_map_select_device):
            assert call(0, 8, pc, C.byref(_rule(L, **kw)), pm, C.byref(new_p), pn) == L.ERR_INVALID, kw
            assert lib.fmx_last_error().decode()
    ok = _rule(L, n_segments=2, segment_base=good.ctypes.data)
    for call in (lib.fmx_column_map_select, lib.fmx_column_map_select_device):
        assert call(0, 8, pc, None, pm, C.byref(new_p), pn) == L.ERR_INVALID
        assert call(0, 8, None, C.byref(ok), pm, C.byref(new_p), pn) == L.ERR_INVALID
        assert call(0, 8, pc, C.byref(ok), None, C.byref(new_p), pn) == L.ERR_INVALID
        assert call(0, 8, pc, C.byref(ok), pm, None, pn) == L.ERR_INVALID
        assert call(0, 2**32 - 2, pc, C.byref(_rule(L)), pm, C.byref(new_p), pn) == L.ERR_INVALID       # no id left for the bucket
    for call in (lib.fmx_column_map_hash, lib.fmx_column_map_hash_device):
        assert call(0, 8, 0, 1, 2, 0, pm, C.byref(new_p)) == L.ERR_INVALID                                # no bucket
        assert call(0, 8, 4, 1, 2, 9, pm, C.byref(new_p)) == L.ERR_INVALID                                # keep_prefix above p
        assert call(0, 8, 2**32 - 3, 1, 2, 2, pm, C.byref(new_p)) == L.ERR_INVALID                        # ids run out
        assert call(0, 8, 4, 1, 2, 0, None, C.byref(new_p)) == L.ERR_INVALID
        assert call(0, 8, 4, 1, 2, 0, pm, None) == L.ERR_INVALID
    assert np.all(cmap == 7) and np.all(nsb == 7) and new_p.value == 7 and np.all(count == 1)
    for call in (lib.fmx_matrix_remap_columns, lib.fmx_matrix_remap_columns_device):
        h = C.c_void_p(5)
        assert call(None, pm, 8, 0, C.byref(h)) == L.ERR_INVALID and not h.value
        assert call(None, pm, 8, 0, None) == L.ERR_INVALID
    for call in (lib.fmx_matrix_column_stats, lib.fmx_matrix_column_stats_device):
        assert call(None, pc, None) == L.ERR_INVALID
    assert np.all(count == 1)
    assert lib.fmx_debug_columns_limits(4, 8, 16) == L.OK and lib.fmx_debug_columns_limits(0, 0, 0) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    for name in ("_device_matrix", "column_map_select", "column_map_hash", "_engine_for"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api.Matrix, "from_csr", classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    d = fm.fm_matrix(np.random.default_rng(0).random((6, 4)), np.arange(6) % 2)
    for f in (fm.fm_feature_stats, fm.fm_prune_features, lambda x: fm.fm_hash_features(x, 4), lambda x: fm.fm_apply_columns(x, None)):
        with pytest.raises(TypeError, match="fm.matrix"):
            f(np.ones((6, 4)))
    with pytest.raises(ValueError, match="rare must be"):
        fm.fm_prune_features(d, rare="oov")
    for kw in (dict(min_rows=-1), dict(min_rows=1.5), dict(max_rows=0), dict(max_features=0), dict(max_features=True), dict(keep_prefix=5), dict(keep_prefix=-1)):
        with pytest.raises(ValueError, match="must be an integer"):
            fm.fm_prune_features(d, **kw)
    with pytest.raises(ValueError, match="combine must be"):
        fm.fm_prune_features(d, combine="mean")
    for fields in ([1, 4], [0, 3], [0, 3, 2, 4], [0.0, 4.0], [4], [[0, 4]]):
        with pytest.raises(ValueError, match="fields must ascend"):
            fm.fm_prune_features(d, fields=fields)
    for kw in (dict(n_buckets=0), dict(n_buckets=2.5), dict(n_buckets=2**32), dict(n_buckets=4, seed=-1), dict(n_buckets=4, keep_prefix=5)):
        with pytest.raises(ValueError, match="must be an integer"):
            fm.fm_hash_features(d, **kw)
    with pytest.raises(ValueError, match="combine must be"):
        fm.fm_hash_features(d, 4, combine="max")
    with pytest.raises(TypeError, match="column map"):
        fm.fm_apply_columns(d, {"map": [0, 1, 2, 3]})
    cmap = fm.ColumnMap(np.array([0, 1, 1, 0xFFFFFFFF], np.uint32), 2, "sum", np.array([True, True, False, False]), d.feature_names, ["a", "b"])
    other = fm.fm_matrix(np.ones((2, 4)), feature_names=["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_apply_columns(other, cmap)


def test_remap_model_carries_kept_rows_and_refuses_collisions(no_device):
    import fmwr_amd as fm
    names = ["V1", "V2", "V3", "V4"]
    w, v = np.array([1.0, 2.0, 3.0, 4.0]), np.arange(8.0).reshape(2, 4)
    fit = {"class": "FM", "Model": {"w0": 0.5, "w": w, "v": v}, "Scales": {"mean": np.array([1.0, 0, 0, 2.0]), "std": np.array([2.0, 1, 1, 3.0]), "model.vars": names,
                                                                            "target.range": (0, 1)}, "Trace": {}}
    # features 0 and 3 survive, 1 and 2 go to the bucket (id 2)
    cmap = fm.ColumnMap(np.array([0, 2, 2, 1], np.uint32), 3, "sum", np.array([True, False, False, True]), names, ["V1", "V4", "rare1"])
    out = fm.fm_remap_model(fit, cmap)
    assert out["Model"]["w"].tolist() == [1.0, 4.0, 0.0] and out["Model"]["v"].tolist() == [[0.0, 3.0, 0.0], [4.0, 7.0, 0.0]]
    assert out["Model"]["w0"] == 0.5 and out["Scales"]["mean"].tolist() == [1.0, 2.0, 0.0] and out["Scales"]["std"].tolist() == [2.0, 3.0, 1.0]
    assert out["Scales"]["model.vars"] == ["V1", "V4", "rare1"] and "Trace" not in out
    assert fit["Model"]["w"] is w and fit["Scales"]["model.vars"] == names           # the source object is left as it was
    # a dropped feature leaves its row behind; two occurring features in one hash bucket cannot be merged
    drop = fm.ColumnMap(np.array([0, 0xFFFFFFFF, 1, 0xFFFFFFFF], np.uint32), 2, "keep", np.array([True, False, True, False]), names, ["V1", "V3"])
    assert fm.fm_remap_model(fit, drop)["Model"]["w"].tolist() == [1.0, 3.0]
    clash = fm.ColumnMap(np.array([0, 1, 1, 0], np.uint32), 2, "sum", np.array([True, True, True, False]), names, ["h1", "h2"], kind="hash")
    with pytest.raises(ValueError, match="two occurring features"):
        fm.fm_remap_model(fit, clash)
    unseen = fm.ColumnMap(np.array([0, 1, 1, 0], np.uint32), 2, "sum", np.array([True, True, False, False]), names, ["h1", "h2"], kind="hash")
    assert fm.fm_remap_model(fit, unseen)["Model"]["w"].tolist() == [1.0, 2.0]      # the unseen features 2 and 3 bring nothing
    with pytest.raises(TypeError):
        fm.fm_remap_model({"class": "lm"}, cmap)
    with pytest.raises(TypeError):
        fm.fm_remap_model(fit, None)
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_remap_model(dict(fit, Scales=dict(fit["Scales"], **{"model.vars": ["a", "b", "c", "d"]})), cmap)
