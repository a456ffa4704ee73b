"""fmx_matrix_cross and fm_cross_features / fm_apply_crosses / fm_cross_candidates against the numpy model of the definition (tests/cross_model.py).
Ids are integers and the value is the IEEE binary32 product, so every comparison is exact equality of row pointers, column ids, value bits and
label bits through fmx_matrix_export: in the three fill forms (single, group, long), on the boundary between the group and the long form (the
hook lowers it to 4 and 8 entries) and with launches of 16 rows."""
import ctypes as C

import numpy as np
import pytest

from tests import cross_cases as cc
from tests import cross_model as cm
from tests import flags_model as flm

pytestmark = pytest.mark.gpu

# fmx_debug_cross_limits' arguments: (single, group_entries, rows_per_launch)
FORMS = {"default": (0, 0, 0), "second call": (0, 0, 0), "group of 4": (0, 4, 0), "group of 8": (0, 8, 0), "long": (0, -1, 0), "launches of 16": (0, 0, 16),
         "long, launches of 16": (0, -1, 16)}
THREE = {"single": (0, 0, 0), "group": (-1, 0, 0), "long": (-1, -1, 0), "group, launches of 16": (-1, 0, 16), "single, launches of 16": (0, 0, 16)}
VOCAB = [3, 1, 17, 300, 70000]
_cache = {}


def _limits(single=0, group=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_cross_limits(single, group, rows))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _state(m):
    """(flags, layout) as the library holds them (tests/test_gpu_flags.py: state)"""
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    d, nf = C.c_int32(-1), C.c_int32(-1)
    base = np.full(flm.MAX_FIELDS + 1, 0xFFFFFFFF, np.uint32)
    L.check(L.lib().fmx_debug_matrix_layout(m.h, C.byref(d), C.byref(nf), base.ctypes.data_as(C.c_void_p)))
    flags = dict(rows_sorted=int(out[0]), unit_values=int(out[1]), fixed_row_len=int(out[2]), max_row_len=int(out[3]))
    return flags, dict(dense_prefix=d.value, field_base=[int(b) for b in base[:nf.value + 1]] if nf.value else [])


def _source(name):
    """(Matrix, (row_ptr, col, val, y or None), p, segment_base) -- made once, shared, never changed"""
    from fmwr_amd import engine
    if name in _cache:
        return _cache[name]
    if name in ("ragged", "ragged_unl"):
        rp, col, val, y = cc.ragged()
        p, base = cc.RAGGED_P, cc.RAGGED_BASE
        y = None if name == "ragged_unl" else y
        m = engine.Matrix.from_csr(rp, col, val, p, y)
    elif name == "values":
        rp, col, val, y, p = cc.values()
        base = cc.VALUE_BASE
        m = engine.Matrix.from_csr(rp, col, val, p, y)
    elif name in ("fields0", "fields2"):
        dense = int(name[-1])
        m = engine.Matrix.synthetic_fields(300, dense, VOCAB, 1.1, 11)
        rp, col, val, y = m.export()
        p = m.p
        base = np.concatenate([np.arange(dense), dense + np.concatenate([[0], np.cumsum(VOCAB)])]).astype(np.uint32)
        assert base[-1] == p
    else:
        raise KeyError(name)
    _cache[name] = (m, (rp, col, val, y), p, base)
    return _cache[name]


def _model(name, terms, seed=0, salt=0, keep=True):
    key = ("model", name, tuple(terms), seed, salt, keep)
    if key not in _cache:
        _, host, p, base = _source(name)
        _cache[key] = cm.cross(host[0], host[1], host[2], p, base, terms, seed, salt, keep)
    return _cache[key]


def _same(out, cross_base, ref, y, what):
    orp, ocol, oval, cb = ref
    assert cross_base.dtype == np.uint32 and np.array_equal(cross_base, cb), what
    assert (out.p, out.nnz) == (int(cb[-1]), int(orp[-1])), what
    grp, gcol, gval, gy = out.export()
    assert np.array_equal(grp, orp), what
    assert np.array_equal(gcol, ocol), what
    assert np.array_equal(cc.bits(gval), cc.bits(oval)), what
    if y is not None:
        assert np.array_equal(cc.bits(gy), cc.bits(y)), what
    got, want = _state(out), flm.truth(orp, ocol, oval, int(cb[-1]))
    assert got == want, (what, got, want)


# --------------------------------------------------------------------------------------------------------------------------- the ragged source
@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", ["ragged", "ragged_unl"])
def test_ragged_rows_equal_the_model_in_every_form(name, keep):
    m, host, p, base = _source(name)
    assert sorted(set(np.diff(host[0]).tolist())) == sorted(cc.RAGGED_LENS)
    ref = _model(name, cc.RAGGED_TERMS, 7, 3, keep)
    counts = np.diff(ref[0]) - (np.diff(host[0]) if keep else 0)
    assert counts.max() > 10000 and ref[3][5] == ref[3][6]                    # the 257-entry rows' bag; the term on the empty segment has width 0
    for form, hook in FORMS.items():
        _limits(*hook)
        out, cb = m.cross(base, cc.RAGGED_TERMS, seed=7, salt=3, keep_source=keep)
        assert out.n == m.n
        _same(out, cb, ref, host[3], (name, keep, form))
        out.close()
    src = m.export()
    assert np.array_equal(src[1], host[1]) and np.array_equal(cc.bits(src[2]), cc.bits(host[2]))   # the source is left as it was


# ---------------------------------------------------------------------------------------------------------------------------- the field source
FIELD_TERMS = {
    "fields0": [(0, 1), (2, 3), (3, 4), (0, 4, 1 << 20), (1, 2, 5)],                  # field x field, the 300 x 70 000 exact width among them
    "fields2": [(0, 1), (0, 2), (1, 6), (5, 6), (2, 4, 1000), (0, 1, 64), (3, 6, 1 << 20)],   # dense x dense, dense x field, field x field
}


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", ["fields0", "fields2"])
def test_field_rows_equal_the_model_in_the_single_the_group_and_the_long_form(name, keep):
    m, host, p, base = _source(name)
    terms = FIELD_TERMS[name]
    ref = _model(name, terms, 5, 0, keep)
    assert np.all(np.diff(ref[0]) == (len(base) - 1 if keep else 0) + len(terms))      # every term is one entry a row
    assert ref[3][-1] > 21_000_000
    for form, hook in THREE.items():
        _limits(*hook)
        out, cb = m.cross(base, terms, seed=5, keep_source=keep)
        _same(out, cb, ref, host[3], (name, keep, form))
        flags, layout = _state(out)
        if name == "fields0":           # a one-hot source stays one-hot and comes out as fields + n_terms fields
            assert flags["unit_values"] == 1 and flags["fixed_row_len"] == (5 if keep else 0) + len(terms)
            assert len(layout["field_base"]) - 1 == (5 if keep else 0) + len(terms)
        out.close()


def test_widths_just_above_the_limit_are_refused_and_the_source_with_a_self_cross_leaves_the_single_form():
    from fmwr_amd import _lib as L
    m, host, p, base = _source("fields0")
    # 300 x 70 000 = 21 000 000 exact ids, and hashed terms that fill the rest: p + 21 000 000 + rest = 2^32 - 2 is taken, one more is not
    rest = 2**32 - 2 - p - 21_000_000
    out, cb = m.cross(base, [(3, 4), (0, 1, rest)])
    assert int(cb[-1]) == 2**32 - 2 and out.p == 2**32 - 2
    _same(out, cb, cm.cross(host[0], host[1], host[2], p, base, [(3, 4), (0, 1, rest)]), host[3], "the widest output")
    out.close()
    arr = (L.CrossTerm * 2)(L.CrossTerm(3, 4, 0, 0), L.CrossTerm(0, 1, rest + 1, 0))
    spec = L.CrossSpec(C.sizeof(L.CrossSpec), len(base) - 1, base.ctypes.data, 2, 1, C.addressof(arr), 0, 0, 0)
    got = np.full(3, 7, np.uint32)
    h = C.c_void_p(5)
    assert L.lib().fmx_matrix_cross(m.h, C.byref(spec), got.ctypes.data_as(C.c_void_p), C.byref(h)) == L.ERR_INVALID
    assert b"2^32 - 2" in L.lib().fmx_last_error() and not h.value and np.all(got == 7)
    bad = base.copy()
    bad[-1] += 1
    spec = L.CrossSpec(C.sizeof(L.CrossSpec), len(base) - 1, bad.ctypes.data, 1, 1, C.addressof(arr), 0, 0, 0)
    assert L.lib().fmx_matrix_cross(m.h, C.byref(spec), got.ctypes.data_as(C.c_void_p), C.byref(h)) == L.ERR_INVALID
    assert b"feature count" in L.lib().fmx_last_error() and np.all(got == 7)
    # a self-cross of a one-entry field emits nothing: the rows are one entry shorter than the single form would make them
    terms = [(0, 1), (2, 2), (1, 2)]
    out, cb = m.cross(base, terms)
    _same(out, cb, cm.cross(host[0], host[1], host[2], p, base, terms), host[3], "a self-cross among field terms")
    assert np.all(np.diff(out.export()[0]) == 5 + 2)
    out.close()


# --------------------------------------------------------------------------------------------------------------------------------- the values
@pytest.mark.parametrize("keep", [True, False])
def test_products_round_once_keep_subnormals_and_canonicalise_nan_in_every_form(keep):
    m, host, p, base = _source("values")
    flags, layout = _state(m)
    assert layout["dense_prefix"] == 2 and len(layout["field_base"]) == 2 and flags["unit_values"] == 0      # the layout the single form needs
    ref = _model("values", cc.VALUE_TERMS, 3, 0, keep)
    prod = cc.bits(ref[2]).reshape(len(cc.VALUE_PAIRS), -1)[:, 3 if keep else 0]
    assert 0x7F800000 in prod and 0xFF800000 in prod and 0x80000000 in prod and cm.NAN_BITS in prod and 0x00000001 in prod and 0x00000002 in prod
    for form, hook in THREE.items():
        _limits(*hook)
        out, cb = m.cross(base, cc.VALUE_TERMS, seed=3, keep_source=keep)
        _same(out, cb, ref, None, (keep, form))
        out.close()


# ------------------------------------------------------------------------------------------------------------ composition and invariances
def test_a_cross_of_a_crossed_segment_is_the_triple():
    m, host, p, base = _source("ragged")
    first = [(0, 1), (1, 3, 7)]
    mid, cb1 = m.cross(base, first, seed=2)
    base2 = np.concatenate([base, cb1[1:]]).astype(np.uint32)               # segment_base followed by cross_base[1:]
    second = [(3, 6), (2, 7, 13), (6, 6)]                                   # 3 x (0 x 1), 2 x hashed(1 x 3), and the crossed segment with itself
    ref1 = cm.cross(host[0], host[1], host[2], p, base, first, 2)
    ref2 = cm.cross(ref1[0], ref1[1], ref1[2], int(cb1[-1]), base2, second, 9)
    for form, hook in (("default", (0, 0, 0)), ("group of 8", (0, 8, 0)), ("long", (0, -1, 0))):
        _limits(*hook)
        out, cb2 = mid.cross(base2, second, seed=9)
        _same(out, cb2, ref2, host[3], ("triple", form))
        out.close()
    # the triple's ids decode to (w, u, v): id = cb2[0] + w * (width(0) * width(1)) + u * width(1) + v
    seg = np.searchsorted(base.astype(np.int64), host[1].astype(np.int64), side="right") - 1
    r = int(np.argmax([np.sum(seg[host[0][i]:host[0][i + 1]] == 3) for i in range(m.n)]))
    row = ref2[1][ref2[0][r]:ref2[0][r + 1]].astype(np.int64)
    c, s = host[1][host[0][r]:host[0][r + 1]].astype(np.int64), seg[host[0][r]:host[0][r + 1]]
    want = [(w - 29) * 20 + u * 4 + (v - 5) for w in c[s == 3] for u in c[s == 0] for v in c[s == 1]]
    triple = row[(row >= cb2[0]) & (row < cb2[1])] - int(cb2[0])
    assert len(want) > 0 and triple.tolist() == want
    mid.close()


def test_cross_commutes_with_take():
    m, host, p, base = _source("ragged")
    rng = np.random.default_rng(3)
    whole, _ = m.cross(base, cc.RAGGED_TERMS, seed=1)
    for what, rows in (("permutation", rng.permutation(m.n)), ("bootstrap", rng.integers(0, m.n, m.n + 7))):
        a = m.take(rows)
        left, cb = a.cross(base, cc.RAGGED_TERMS, seed=1)
        right = whole.take(rows)
        x, y = left.export(), right.export()
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(cc.bits(x[2]), cc.bits(y[2])) and np.array_equal(cc.bits(x[3]), cc.bits(y[3])), what
        for t in (a, left, right):
            t.close()
    whole.close()


def test_cross_then_prune_then_remap_equals_the_models_chained():
    from fmwr_amd import _lib as L, engine
    from tests import columns_model as colm
    m, host, p, base = _source("ragged")
    terms = [(0, 1), (2, 2, 64), (1, 3)]
    out, cb = m.cross(base, terms, seed=4)
    ref = cm.cross(host[0], host[1], host[2], p, base, terms, 4)
    out_base = np.concatenate([base, cb[1:]]).astype(np.uint32)
    count, _ = out.column_stats(values=False)
    mcount, _ = colm.column_stats(ref[0], ref[1], ref[2], host[3], int(cb[-1]))
    assert np.array_equal(count, mcount)
    rule = dict(by=L.COLUMNS_BY_ROWS, min_count=3, rare=L.RARE_BUCKET, segment_base=out_base)
    cmap, new_p, nsb = engine.column_map_select(out.p, count, **rule)
    mmap, mnew_p, mnsb = colm.map_select(int(cb[-1]), mcount, by=colm.BY_ROWS, min_count=3, rare=colm.RARE_BUCKET, segment_base=out_base)
    assert np.array_equal(cmap, mmap) and new_p == mnew_p and np.array_equal(nsb, mnsb)
    pruned = out.remap_columns(cmap, new_p, L.COMBINE_SUM)
    want = colm.remap(ref[0], ref[1], ref[2], mmap, mnew_p, colm.COMBINE_SUM)
    got = pruned.export()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(cc.bits(got[2]), cc.bits(want[2]))
    assert new_p < out.p
    pruned.close()
    out.close()


# ----------------------------------------------------------------------------------------------------------------- the device-side refusals
def test_a_row_or_an_output_above_2_31_entries_is_refused_by_the_length_pass():
    """one row of 65 537 entries of one segment, crossed with itself, is 2 147 516 416 pairs; nothing is allocated.  (The passing case next to it,
    65 536 entries, would write 17 GB: left out.)"""
    from fmwr_amd import _lib as L, engine
    lens = np.array([3, 65537, 0, 65537], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = (np.arange(int(rp[-1])) % 50).astype(np.uint32)
    m = engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), 60)
    base = np.array([0, 50, 60], np.uint32)

    def refused(mat, terms):
        arr = (L.CrossTerm * len(terms))(*[L.CrossTerm(a, b, nb, 0) for a, b, nb in terms])
        spec = L.CrossSpec(C.sizeof(L.CrossSpec), 2, base.ctypes.data, len(terms), 0, C.addressof(arr), 0, 0, 0)
        got = np.full(len(terms) + 1, 7, np.uint32)
        h = C.c_void_p(5)
        st = L.lib().fmx_matrix_cross(mat.h, C.byref(spec), got.ctypes.data_as(C.c_void_p), C.byref(h))
        assert st == L.ERR_INVALID and not h.value and np.all(got == 7)
        return L.lib().fmx_last_error().decode()
    for form, hook in (("default", (0, 0, 0)), ("launches of 2 rows", (0, 0, 2)), ("long", (0, -1, 0))):
        _limits(*hook)
        assert "row 1 " in refused(m, [(0, 0, 1000)]), form
        assert "row 1 " in refused(m, [(0, 1, 0), (0, 0, 1000)]), form
    m.close()
    # no single row is too long, the rows together are: 2 x 46 342 x 46 341 / 2 pairs
    lens = np.array([46342, 1, 46342], np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    col = (np.arange(int(rp[-1])) % 50).astype(np.uint32)
    m = engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), 60)
    _limits()
    assert "the output would hold 2147534622 entries" in refused(m, [(0, 0, 1000)])
    out, cb = m.cross(base, [(0, 1), (1, 1)], keep_source=False)           # and a call that emits nothing at all is taken
    assert (out.n, out.nnz, out.p) == (3, 0, 600)
    out.close()
    m.close()


# ------------------------------------------------------------------------------------------------------------------------------ end to end
def _parity_data(n, seed):
    import fmwr_amd as fm
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    abc = rng.integers(0, 4, (n, 3))
    col = (abc + np.array([0, 4, 8])).ravel()
    X = sp.csr_matrix((np.ones(3 * n), col, np.arange(n + 1) * 3), shape=(n, 12))
    y = np.where(abc.sum(axis=1) % 2 == 0, 1.0, -1.0)
    names = [f"{f}{i}" for f in "abc" for i in range(4)]
    return fm.fm_matrix(X, y, feature_names=names)


E2E_FIELDS = [0, 4, 8, 12]
E2E_BAR = 0.75          # halfway between the measured held-out accuracies: crossed 1.000, plain 0.4995 on average over three seeds (profiles/cross.txt)


def _parity_fits(seed):
    import fmwr_amd as fm
    data = _parity_data(6000, 100 + seed)
    train, test, _ = fm.fm_split(data, test_fraction=0.25, seed=seed)
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 4, "v.init_stdev": 0.1}),
           fm.solver_control(max_iter=200 * train.dim[0], solver=fm.SGD_solver(learn_rate=0.1))]
    kw = dict(normalize=False, seed=seed, control=ctl, mode="minibatch", batch_rows=256)
    plain = fm.fm_train(train, **kw)
    crossed_train, crossing = fm.fm_cross_features(train, [(0, 1)], E2E_FIELDS)
    crossed = fm.fm_train(crossed_train, **kw)
    acc_plain = fm.fm_metrics(plain, test, normalize=False)["pooled"]["accuracy"]
    acc_cross = fm.fm_metrics(crossed, fm.fm_apply_crosses(test, crossing), normalize=False)["pooled"]["accuracy"]
    return plain, crossed_train, crossing, test, acc_plain, acc_cross


def test_a_cross_lets_the_model_learn_a_third_order_effect():
    """Three one-hot fields of four ids, y = +1 iff a + b + c is even: every function of at most two of the fields is uncorrelated with y, so the
    degree-2 FM stays at chance; with the pair (a, b) crossed the effect is <v_ab, v_c>.  fm_split -> fm_train (mini-batch, k = 4) -> fm_metrics,
    once plain and once after fm_cross_features(pairs=[(0, 1)]) with fm_apply_crosses on the held-out part.  Measured on an MI355X over the seeds
    1, 2, 3 (profiles/cross.txt): plain 0.4373, 0.5200, 0.5413 (a spread of 0.104 around chance), crossed 1.0000 three times.  The bar lies
    halfway between the two, at 0.75: twice the plain fit's spread above its best seed."""
    import fmwr_amd as fm
    plain, crossed_train, crossing, test, acc_plain, acc_cross = _parity_fits(1)
    print(f"held-out accuracy: plain {acc_plain:.4f} crossed {acc_cross:.4f}")
    assert crossed_train.dim[1] == 28 and crossing.new_segment_base.tolist() == [0, 4, 8, 12, 28]
    assert crossed_train.feature_names[12] == "a0:b0" and crossed_train.feature_names[27] == "a3:b3"
    ids = crossed_train.features["col_idx"].reshape(-1, 4)
    assert np.array_equal(ids[:, 3], 12 + ids[:, 0] * 4 + (ids[:, 1] - 4)) and np.all(crossed_train.features["value"] == 1.0)
    assert acc_cross > E2E_BAR > acc_plain
    cand = fm.fm_cross_candidates(plain, test, E2E_FIELDS, normalize=False)
    assert sorted((a, b) for a, b, _ in cand) == [(0, 1), (0, 2), (1, 2)] and all(s >= 0 for _, _, s in cand)
    assert [s for _, _, s in cand] == sorted((s for _, _, s in cand), reverse=True)
    assert len(fm.fm_cross_candidates(plain, test, E2E_FIELDS, top=2, normalize=False)) == 2
