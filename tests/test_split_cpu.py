"""CPU-side checks of the row-selection surface (fmx_matrix_take, fmx_split_assign, fmx_matrix_select, fmx_matrix_split_entries,
fmx_row_permutation; fmwr_amd.fm_split / fm_folds / fm_holdout): the numpy model of the definition (tests/split_model.py) against a brute-force
Python loop, the guarantees include/fmx.h states, the declared surface, and the argument checks, which run before any device."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

from tests import split_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_matrix_take", "fmx_matrix_take_device", "fmx_split_assign", "fmx_split_assign_device", "fmx_matrix_select", "fmx_matrix_select_device",
         "fmx_free_device", "fmx_matrix_split_entries", "fmx_row_permutation", "fmx_row_permutation_device")
M = 2**64 - 1


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


def _part(rho, s, n_folds, hold_count, hold_fraction, min_keep):
    if n_folds:
        return rho * n_folds // s
    c = hold_count if hold_count > 0 else math.floor(hold_fraction * float(s))
    return 1 if rho < min(c, max(s - min_keep, 0)) else 0


def _brute(n, groups, G, scope, order, seed, salt, **rule):
    """include/fmx.h's wording, one item at a time"""
    if scope == sm.ROWS:
        segments, stream = [list(range(n))], 0
    elif scope == sm.WITHIN_GROUPS:
        segments, stream = [[r for r in range(n) if groups[r] == g] for g in range(G)], 0
    else:
        segments, stream = [list(range(G))], 1
    part = {}
    for items in segments:
        ranked = sorted(items, reverse=True) if order == sm.ORDER_TAIL else sorted(items, key=lambda i: (_H(seed, salt, i, stream), i))
        for rho, i in enumerate(ranked):
            part[i] = _part(rho, len(items), **rule)
    if scope == sm.GROUPS:
        return np.array([part[int(g)] for g in groups], np.uint32)
    return np.array([part[r] for r in range(n)], np.uint32)


def _groups_200():
    """200 rows in 7 groups of 0, 1, 2, 17, 40, 60 and 80 rows, interleaved"""
    sizes = [0, 1, 2, 17, 40, 60, 80]
    g = np.repeat(np.arange(7), sizes)
    return np.random.default_rng(4).permutation(g).astype(np.uint32), 7


RULES = [dict(n_folds=0, hold_count=3, hold_fraction=0.0, min_keep=mk) for mk in (0, 1)] + \
        [dict(n_folds=0, hold_count=0, hold_fraction=0.3, min_keep=mk) for mk in (0, 1)] + \
        [dict(n_folds=k, hold_count=0, hold_fraction=0.0, min_keep=0) for k in (2, 3, 10)]


def test_hash_matches_the_integer_chain():
    t = np.array([0, 1, 5, 2**32, 2**63 + 11, M], np.uint64)
    for seed, salt, stream in ((0, 0, 0), (7, 3, 1), (M, M, 2), (12345, 2**40, 3)):
        assert sm.H(seed, salt, t, stream).tolist() == [_H(seed, salt, int(x), stream) for x in t]
    assert sm.key_entry(5, 6, [3], [9])[0] == _H(5, 6, (3 << 32) | 9, 2)


@pytest.mark.parametrize("scope", [sm.ROWS, sm.WITHIN_GROUPS, sm.GROUPS])
@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_model_matches_the_brute_force_loop(scope, order):
    g, G = _groups_200()
    assert sorted(np.bincount(g, minlength=G).tolist())[:3] == [0, 1, 2]
    for rule in RULES:
        got = sm.assign(200, g, G, scope=scope, order=order, seed=11, salt=5, **rule)
        ref = _brute(200, g, G, scope, order, 11, 5, **rule)
        assert got.dtype == np.uint32 and np.array_equal(got, ref), (scope, order, rule)


def test_parts_are_a_function_of_the_arguments_alone():
    g, G = _groups_200()
    for scope, rule in itertools.product((sm.ROWS, sm.WITHIN_GROUPS, sm.GROUPS), RULES):
        a = sm.assign(200, g, G, scope=scope, seed=3, **rule)
        assert np.array_equal(a, sm.assign(200, g.copy(), G, scope=scope, seed=3, **rule))
    assert not np.array_equal(sm.assign(200, seed=3, hold_count=50), sm.assign(200, seed=4, hold_count=50))
    assert not np.array_equal(sm.assign(200, seed=3, salt=0, hold_count=50), sm.assign(200, seed=3, salt=1, hold_count=50))


@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_within_groups_a_part_depends_on_the_group_s_own_rows_only(order):
    g, G = _groups_200()
    for rule in RULES:
        ref = sm.assign(200, g, G, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule)
        renumbered = (G - 1 - g.astype(np.int64) + 30).astype(np.uint32)   # other ids, other n_groups
        assert np.array_equal(sm.assign(200, renumbered, G + 30, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule), ref)
        for keep in (3, 6):   # every other group's rows thrown into one group: the kept group's parts stay
            merged = np.where(g == keep, 1, 0).astype(np.uint32)
            got = sm.assign(200, merged, 2, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule)
            assert np.array_equal(got[g == keep], ref[g == keep])
        gone = np.where(g == 5, 5, 1000).astype(np.uint32)   # the other groups out of range: no segment, no part
        got = sm.assign(200, gone, G, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule)
        assert np.array_equal(got[g == 5], ref[g == 5]) and np.all(got[g != 5] == sm.NO_PART)


@pytest.mark.parametrize("scope", [sm.ROWS, sm.WITHIN_GROUPS, sm.GROUPS])
@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_held_sets_are_nested_in_the_count(scope, order):
    g, G = _groups_200()
    prev = np.zeros(200, bool)
    for c in (1, 2, 3, 5, 17, 60, 500):
        held = sm.assign(200, g, G, scope=scope, order=order, hold_count=c, min_keep=1, seed=21) == 1
        assert np.all(held[prev]) and held.sum() >= prev.sum()
        prev = held


def test_groups_scope_ignores_the_rows():
    g, G = _groups_200()
    for rule in RULES:
        a = sm.assign(200, g, G, scope=sm.GROUPS, seed=2, **rule)
        other = np.random.default_rng(1).integers(0, G, 77).astype(np.uint32)
        b = sm.assign(77, other, G, scope=sm.GROUPS, seed=2, **rule)
        of_group = {int(x): int(p) for x, p in zip(g, a)}
        assert all(of_group.get(int(x), int(p)) == int(p) for x, p in zip(other, b))
        for q in range(G):   # no group on two sides
            assert len(set(a[g == q].tolist())) <= 1


def test_every_item_has_one_part_and_fold_sizes_differ_by_at_most_one():
    g, G = _groups_200()
    for K in (2, 3, 10):
        rows = sm.assign(200, scope=sm.ROWS, n_folds=K, seed=1)
        sizes = np.bincount(rows, minlength=K)
        assert rows.max() == K - 1 and sizes.sum() == 200 and sizes.max() - sizes.min() <= 1
        within = sm.assign(200, g, G, scope=sm.WITHIN_GROUPS, n_folds=K, seed=1)
        for q in range(G):
            sizes = np.bincount(within[g == q], minlength=K)
            assert sizes.sum() == (g == q).sum() and sizes.max() - sizes.min() <= 1
        gp = sm.assign(G, np.arange(G, dtype=np.uint32), G, scope=sm.GROUPS, n_folds=K, seed=1)
        sizes = np.bincount(gp, minlength=K)
        assert sizes.sum() == G and sizes.max() - sizes.min() <= 1


def test_tail_holds_exactly_the_last_rows_of_a_group():
    g, G = _groups_200()
    for c, mk in ((1, 0), (3, 1), (50, 1), (50, 0)):
        part = sm.assign(200, g, G, scope=sm.WITHIN_GROUPS, order=sm.ORDER_TAIL, hold_count=c, min_keep=mk)
        for q in range(G):
            rows = np.flatnonzero(g == q)
            k = min(c, max(len(rows) - mk, 0))
            assert np.array_equal(np.flatnonzero(part[rows] == 1), np.arange(len(rows) - k, len(rows)))
    part = sm.assign(200, scope=sm.ROWS, order=sm.ORDER_TAIL, hold_fraction=0.25)
    assert np.array_equal(np.flatnonzero(part == 1), np.arange(150, 200))


def test_hold_fraction_is_one_rounded_product():
    sizes = (10, 3, 7, 1003)
    for f in (0.1, 0.3, 0.7, 1.0, 0.0):
        held = [int((sm.part_of(np.arange(n), np.full(n, n), hold_fraction=f) == 1).sum()) for n in sizes]
        assert held == [math.floor(f * float(n)) for n in sizes]


def _entries_case():
    rng = np.random.default_rng(6)
    lens = np.array([0, 1, 2, 3, 9, 64, 65, 0, 5])
    rp = np.zeros(len(lens) + 1, np.int64); rp[1:] = np.cumsum(lens)
    col = np.concatenate([rng.choice(100, n, replace=False) for n in lens]).astype(np.uint32)
    col[rp[4] + 1] = col[rp[4] + 6]   # a column stored twice in one row
    val = rng.normal(size=len(col)).astype(np.float32)
    return rp, col, val


@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_entries_kept_and_held_interleave_back_to_the_row(order):
    rp, col, val = _entries_case()
    for rule in (dict(hold_count=1, min_keep=1), dict(hold_count=4, min_keep=0), dict(hold_count=0, hold_fraction=0.5, min_keep=2)):
        held = sm.entries_held(rp, col, order=order, seed=8, salt=1, **rule)
        (krp, kcol, kval), (hrp, hcol, hval) = sm.split_entries(rp, col, val, order=order, seed=8, salt=1, **rule)
        for r in range(len(rp) - 1):
            a, b = rp[r], rp[r + 1]
            s = b - a
            c = rule["hold_count"] if rule["hold_count"] > 0 else math.floor(rule.get("hold_fraction", 0.0) * float(s))
            assert held[a:b].sum() == min(c, max(s - rule["min_keep"], 0))
            merged_c, merged_v = np.empty(s, np.uint32), np.empty(s, np.float32)
            merged_c[held[a:b]], merged_c[~held[a:b]] = hcol[hrp[r]:hrp[r + 1]], kcol[krp[r]:krp[r + 1]]
            merged_v[held[a:b]], merged_v[~held[a:b]] = hval[hrp[r]:hrp[r + 1]], kval[krp[r]:krp[r + 1]]
            assert np.array_equal(merged_c, col[a:b]) and np.array_equal(merged_v.view(np.uint32), val[a:b].view(np.uint32))
            if order == sm.ORDER_TAIL:
                assert np.all(held[a:b][s - int(held[a:b].sum()):]) or held[a:b].sum() == 0
    # the twice-stored column: equal keys, the earlier position ranks first
    a = rp[4]
    ranked = sorted(range(9), key=lambda i: (_H(8, 1, (4 << 32) | int(col[a + i]), 2), i))
    assert ranked.index(1) < ranked.index(6)
    held = sm.entries_held(rp, col, hold_count=ranked.index(1) + 1, min_keep=0, seed=8, salt=1)
    assert held[a + 1] and not held[a + 6]


def test_take_and_select_are_fancy_indexing():
    rp, col, val = _entries_case()
    y = np.arange(len(rp) - 1, dtype=np.float32)
    rows = np.array([5, 0, 5, 8, 1, 1, 7])
    orp, ocol, oval, oy = sm.take(rp, col, val, y, rows)
    for t, r in enumerate(rows):
        assert np.array_equal(ocol[orp[t]:orp[t + 1]], col[rp[r]:rp[r + 1]]) and np.array_equal(oval[orp[t]:orp[t + 1]], val[rp[r]:rp[r + 1]])
    assert np.array_equal(oy, y[rows])
    part = np.array([0, 2, 1, sm.NO_PART, 2, 0, 1, 1, 0], np.uint32)
    assert sm.select_rows(part, 1).tolist() == [2, 6, 7] and sm.select_rows(part, 1, True).tolist() == [0, 1, 4, 5, 8]
    assert sm.take(rp, col, val, None, np.zeros(0, np.int64))[0].tolist() == [0]


def test_permutation_is_one_and_epochs_differ():
    a, b = sm.permutation(1000, 5, 0), sm.permutation(1000, 5, 1)
    assert np.array_equal(np.sort(a), np.arange(1000)) and np.array_equal(np.sort(b), np.arange(1000)) and not np.array_equal(a, b)
    assert a.tolist() == sorted(range(1000), key=lambda r: (_H(5, 0, r, 3), r))


@pytest.mark.parametrize("seed", [0, 1, 7, 12345])
def test_the_hash_spreads_the_held_rows(seed):
    """20 000 of 100 000 rows held: the held share of the first half is binomial around 0.2 with a standard deviation of 0.0018 (sampling
    without replacement: a little less); the bar is 5 of them"""
    part = sm.assign(100_000, scope=sm.ROWS, hold_count=20_000, seed=seed)
    assert int(part.sum()) == 20_000
    share = float(part[:50_000].sum()) / 50_000
    assert abs(share - 0.2) <= 0.01, share


def _lib():
    from fmwr_amd import _lib, build
    build.build()
    return _lib


def test_selection_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_take_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_take_limits")
    assert "fmx_debug_take_limits" not in text   # the hook stays out of the public header
    for name, value in (("ROWS", 0), ("WITHIN_GROUPS", 1), ("GROUPS", 2), ("ORDER_HASH", 0), ("ORDER_TAIL", 1)):
        assert re.search(r"#define\s+FMX_SPLIT_" + name + r"\s+" + str(value) + r"\b", header), name
        assert getattr(L, "SPLIT_" + name) == value
        assert getattr(sm, name) == value
    assert L.SPLIT_NO_PART == sm.NO_PART == 0xFFFFFFFF
    fields = re.search(r"typedef struct fmx_split_spec \{(.*?)\} fmx_split_spec;", header, flags=re.S).group(1)
    declared = [n for decl in fields.split(";") for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",") if n]
    assert declared == [f[0] for f in L.SplitSpec._fields_]
    assert C.sizeof(L.SplitSpec) == 56
    import fmwr_amd as fm
    from fmwr_amd import engine
    for f in (fm.fm_split, fm.fm_folds, fm.fm_holdout, engine.split_assign, engine.row_permutation):
        assert callable(f)
    for method in ("take", "select", "split_entries", "shuffled"):
        assert callable(getattr(fm.Matrix, method))


def _spec(L, **kw):
    v = dict(scope=0, order=0, n_folds=0, hold_count=0, hold_fraction=0.2, min_keep=0, seed=1, salt=2)
    v.update(kw)
    s = L.SplitSpec(C.sizeof(L.SplitSpec), v["scope"], v["order"], v["n_folds"], v["hold_count"], v["hold_fraction"], v["min_keep"], v["seed"], v["salt"])
    if "struct_size" in kw:
        s.struct_size = kw["struct_size"]
    return s


def test_split_assign_refusals_come_before_any_device_and_write_nothing():
    L = _lib()
    out = np.full(8, 7, np.uint32)
    grp = np.zeros(8, np.uint32)
    po, pg = out.ctypes.data_as(C.c_void_p), grp.ctypes.data_as(C.c_void_p)
    call = L.lib().fmx_split_assign
    bad = [dict(struct_size=12), dict(scope=3), dict(scope=-1), dict(order=2), dict(order=-1), dict(n_folds=1), dict(n_folds=65537), dict(n_folds=-2),
           dict(hold_count=-1), dict(min_keep=-1), dict(hold_fraction=-0.1), dict(hold_fraction=1.5), dict(hold_fraction=float("nan"))]
    for kw in bad:
        assert call(0, 8, pg, 1, C.byref(_spec(L, **kw)), po) == L.ERR_INVALID, kw
        assert L.lib().fmx_last_error().decode()
        assert L.lib().fmx_split_assign_device(0, 8, None, 1, C.byref(_spec(L, **kw)), po) == L.ERR_INVALID, kw
    assert call(0, 8, pg, 1, None, po) == L.ERR_INVALID                                   # no spec
    assert call(0, 8, pg, 1, C.byref(_spec(L)), None) == L.ERR_INVALID                    # no output
    assert call(0, -1, pg, 1, C.byref(_spec(L)), po) == L.ERR_INVALID                     # n out of range
    assert call(0, 2**31, None, 1, C.byref(_spec(L)), po) == L.ERR_INVALID
    assert call(0, 8, None, 1, C.byref(_spec(L, scope=1)), po) == L.ERR_INVALID           # NULL groups need scope ROWS
    assert call(0, 8, None, 1, C.byref(_spec(L, scope=2)), po) == L.ERR_INVALID
    assert call(0, 8, pg, 0, C.byref(_spec(L, scope=1)), po) == L.ERR_INVALID             # n_groups out of range
    assert call(0, 8, pg, 2**31, C.byref(_spec(L, scope=1)), po) == L.ERR_INVALID
    grp[5] = 3
    assert call(0, 8, pg, 3, C.byref(_spec(L, scope=1)), po) == L.ERR_INVALID             # an id >= n_groups (host form)
    assert b"group_of_row[5]" in L.lib().fmx_last_error()
    assert np.all(out == 7)
    h = C.c_void_p(5)
    assert L.lib().fmx_matrix_take(None, None, 0, C.byref(h)) == L.ERR_INVALID and not h.value
    assert L.lib().fmx_row_permutation(0, -1, 0, 0, po) == L.ERR_INVALID
    assert L.lib().fmx_row_permutation(0, 2**31, 0, 0, po) == L.ERR_INVALID
    hk, hh = C.c_void_p(5), C.c_void_p(5)
    assert L.lib().fmx_matrix_split_entries(None, 0, 1, 0.0, 1, 0, 0, C.byref(hk), C.byref(hh)) == L.ERR_INVALID and not hk.value and not hh.value
    assert L.lib().fmx_free_device(None) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    for name in ("_device_matrix", "split_assign", "_engine_for"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api.Matrix, "from_csr", classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    d = fm.fm_matrix(np.random.default_rng(0).random((6, 4)), np.arange(6) % 2)
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_split(np.ones((6, 4)))
    with pytest.raises(ValueError, match="how must be"):
        fm.fm_split(d, how="stratified")
    with pytest.raises(ValueError, match="order must be"):
        fm.fm_split(d, order="first")
    with pytest.raises(ValueError, match="needs `by`"):
        fm.fm_split(d, how="within")
    with pytest.raises(ValueError, match="one integer group id per row"):
        fm.fm_split(d, how="groups", by=[0, 1, 2])
    with pytest.raises(ValueError, match="one integer group id per row"):
        fm.fm_split(d, how="groups", by=np.zeros(6))
    with pytest.raises(ValueError, match="test_fraction"):
        fm.fm_split(d, test_fraction=1.2)
    with pytest.raises(ValueError, match="test_fraction"):
        fm.fm_split(d, test_fraction=float("nan"))
    with pytest.raises(ValueError, match="test_count"):
        fm.fm_split(d, test_count=0)
    with pytest.raises(ValueError, match="min_keep"):
        fm.fm_split(d, min_keep=-1)
    with pytest.raises(ValueError, match="how must be"):
        fm.fm_folds(d, 3, how="user")
    with pytest.raises(ValueError, match="k must be"):
        fm.fm_folds(d, 1)
    with pytest.raises(ValueError, match="at most 65536"):
        fm.fm_folds(d, 70000)
    with pytest.raises(ValueError, match="needs `by`"):
        fm.fm_folds(d, 3, how="groups")
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_folds([1, 2, 3], 3)
    with pytest.raises(ValueError, match="order must be"):
        fm.fm_holdout([[1, 2], [3]], order="newest")
    with pytest.raises(ValueError, match="hold must be"):
        fm.fm_holdout([[1, 2], [3]], hold=0)
    with pytest.raises(ValueError, match="fraction must be"):
        fm.fm_holdout([[1, 2], [3]], fraction=2.0)
    with pytest.raises(ValueError, match="min_keep"):
        fm.fm_holdout([[1, 2], [3]], min_keep=-1)
    with pytest.raises(ValueError, match="outside"):
        fm.fm_holdout([[1, -2], [3]])
    from fmwr_amd import engine
    with pytest.raises(ValueError, match="one group id per row"):
        engine.split_assign(5, groups=[0, 1])
