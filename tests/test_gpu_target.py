"""fmx_target_stats*, fmx_target_table_*, fmx_matrix_encode_targets* and fm_encode_targets / fm_apply_targets against the numpy model of the
definition (tests/target_model.py).  Counts are integers, kept entries copied bits, sums and values fixed chains of IEEE operations, so every
comparison is exact equality of bits: the two forms of the fit (unit, sorted), the three of the apply (single, group, long), the boundary between
the group and the long form (the hook lowers it to 4 and 16 entries) and launches of a few entries or rows."""
import ctypes as C
import pickle

import numpy as np
import pytest

from tests import cross_model as cm
from tests import flags_model as flm
from tests import target_cases as tc
from tests import target_model as tm
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

# fmx_debug_target_limits' arguments: (single, group_entries, chunk_entries, rows_per_launch)
STATS_FORMS = {"default": (0, 0, 0, 0), "second call": (0, 0, 0, 0), "sorted": (0, -1, 0, 0), "launches of 7 entries": (0, 0, 7, 5), "sorted, launches of 7 entries": (0, -1, 7, 5)}
APPLY_FORMS = {"default": (0, 0, 0, 0), "second call": (0, 0, 0, 0), "group of 4": (-1, 4, 0, 0), "group of 16": (-1, 16, 0, 0), "long": (-1, -1, 0, 0),
               "launches of 16": (-1, 0, 0, 16), "long, launches of 16": (-1, -1, 0, 16)}
FIELD_FORMS = {"single": (0, 0, 0, 0), "single, launches of 16": (0, 0, 0, 16), "group": (-1, 0, 0, 0), "long": (-1, -1, 0, 0), "group, launches of 16": (-1, 0, 0, 16)}
_cache = {}


def _limits(single=0, group=0, chunk=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_target_limits(single, group, chunk, rows))


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
    """(Matrix, (row_ptr, col, val, y), p, segment_base, term_segment) -- made once, shared, never changed"""
    from fmwr_amd import engine
    if name in _cache:
        return _cache[name]
    if name == "ragged":
        rp, col, val, y = tc.ragged()
        p, base, terms = tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS
        m = engine.Matrix.from_csr(rp, col, val, p, y)
    elif name == "tall":
        rp, col, val, y = tc.tall()
        p, base, terms = tc.TALL_P, tc.TALL_BASE, np.array([0], np.uint32)
        m = engine.Matrix.from_csr(rp, col, val, p, y)
    elif name in ("fields0", "fields2"):
        dense = int(name[-1])
        m = engine.Matrix.synthetic_fields(300, dense, tc.FIELD_VOCAB, 1.1, 11)
        rp, col, val, y = m.export()
        p, base = m.p, tc.field_base(dense)
        terms = np.arange(len(base) - 1, dtype=np.uint32) if dense == 0 else np.array([1, 2, 4, 5, 6], np.uint32)   # a dense column among them
        assert base[-1] == p
    else:
        raise KeyError(name)
    _cache[name] = (m, (rp, col, val, y), p, base, terms)
    return _cache[name]


def _stats_model(name, n_parts, target, part):
    key = ("stats", name, n_parts, target, None if part is None else part.tobytes())
    if key not in _cache:
        _, host, p, base, terms = _source(name)
        _cache[key] = tm.target_stats(host[0], host[1], host[3], p, base, terms, n_parts, target, part)
    return _cache[key]


def _same_table(table, ref, what):
    count, total = table.export()
    assert count.dtype == np.int64 and np.array_equal(count, ref[0]), what
    if ref[1] is None:
        assert total is None, what
    else:
        assert np.array_equal(tc.bits64(total), tc.bits64(ref[1])), what


def _same_matrix(out, enc_base, ref, y, what, flags=True):
    orp, ocol, oval, eb = ref
    assert enc_base.dtype == np.uint32 and np.array_equal(enc_base, eb), what
    assert (out.p, out.nnz) == (int(eb[-1]), int(orp[-1])), what
    grp, gcol, gval, gy = out.export()
    assert np.array_equal(grp, orp), what
    assert np.array_equal(gcol, ocol), what
    assert np.array_equal(tc.bits(gval), tc.bits(oval)), what
    if y is not None:
        assert np.array_equal(tc.bits(gy), tc.bits(y)), what
    if flags:
        got, want = _state(out), flm.truth(orp, ocol, oval, int(eb[-1]))
        assert got == want, (what, got, want)


# ----------------------------------------------------------------------------------------------------------------------------------- the fit
@pytest.mark.parametrize("target", [tm.POSITIVE, tm.LABEL])
@pytest.mark.parametrize("n_parts", [1, 2, 5, 64])
def test_ragged_stats_equal_the_model_in_both_forms(n_parts, target):
    m, host, p, base, terms = _source("ragged")
    assert sorted(set(np.diff(host[0]).tolist())) == sorted(tc.RAGGED_LENS)
    parts = [tc.ragged_parts(m.n, n_parts)] + ([None] if n_parts == 1 else [])
    for part in parts:
        ref = _stats_model("ragged", n_parts, target, part)
        if part is not None:
            assert np.any(part == tc.NO_PART) and np.any(part == n_parts) and 0 < ref[0][:, :, 0].sum()
        for form, hook in STATS_FORMS.items():
            _limits(*hook)
            table = m.target_stats(part, base, terms, n_parts=n_parts, target=target)
            assert table.info() == dict(device=0, p=p, n_segments=len(base) - 1, n_terms=len(terms), n_parts=n_parts, target=target, width=33,
                                        device_bytes=table.device_bytes)
            _same_table(table, ref, (n_parts, target, part is None, form))
            table.free()
    # a column stored twice in a row counts once: the bag's rows are fewer than its entries
    seg = np.searchsorted(base.astype(np.int64), host[1].astype(np.int64), side="right") - 1
    whole = _stats_model("ragged", 1, target, None)
    assert whole[0][6:26, 0, 0].sum() < np.sum(seg == 3) and np.all(whole[0][26:, 0, 0] == 0)


@pytest.mark.parametrize("target", [tm.POSITIVE, tm.LABEL])
def test_cells_at_the_chunk_edges_of_the_sum_host_and_device_parts(target):
    m, host, p, base, terms = _source("tall")
    n = m.n
    ref = _stats_model("tall", 1, target, None)
    assert ref[0][:, 0, 0].tolist() == list(tc.TALL_ROWS)
    if target == tm.LABEL:
        s = ref[1][:, 0]
        assert np.isfinite(s[0]) and s[1] == np.inf and np.isfinite(s[2]) and tc.bits64(s[3:4])[0] == tm.NAN64 and tc.bits64(s[4:5])[0] == 0   # 0.0 + -0.0 = +0.0
        assert s[2] != np.sum(host[3][2047:3072].astype(np.float64))                       # the order of the sum shows on these labels
    two = (np.arange(n) % 2).astype(np.uint32)
    two[1023:1023 + 1024] = 1                                                              # a cell of 1 024 rows next to an empty one
    two[-1] = tc.NO_PART
    for part, n_parts in ((None, 1), (two, 2)):
        ref = _stats_model("tall", n_parts, target, part)
        for form, hook in STATS_FORMS.items():
            _limits(*hook)
            table = m.target_stats(part, base, terms, n_parts=n_parts, target=target)
            _same_table(table, ref, (target, n_parts, form))
            table.free()
        _limits()
        d = None if part is None else DevBuf.from_numpy(part)
        table = m.target_stats_device(None if d is None else d.ptr, base, terms, n_parts=n_parts, target=target)
        _same_table(table, ref, (target, n_parts, "device part"))
        table.free()


@pytest.mark.parametrize("name", ["fields0", "fields2"])
def test_field_stats_the_unit_and_the_sorted_form_agree_with_the_model(name):
    from fmwr_amd import engine
    m, host, p, base, terms = _source(name)
    flags, layout = _state(m)
    assert flags["rows_sorted"] == 1 and (flags["unit_values"] == 1) == (name == "fields0")   # fields0 takes the unit form, fields2 never
    part = engine.split_assign(m.n, n_folds=5, seed=3)
    for target in (tm.POSITIVE, tm.LABEL):
        ref = _stats_model(name, 5, target, part)
        assert ref[0][:, :, 0].sum() == m.n * len(terms)                                     # every row holds every field once
        for form, hook in STATS_FORMS.items():
            _limits(*hook[:2], 64 * hook[2], 64 * hook[3])
            table = m.target_stats(part, base, terms, n_parts=5, target=target)
            _same_table(table, ref, (name, target, form))
            table.free()


def test_export_from_arrays_export_is_the_identity():
    from fmwr_amd import engine
    rng = np.random.default_rng(2)
    base, terms = np.array([0, 3, 3, 10, 12], np.uint32), np.array([0, 1, 3], np.uint32)
    for n_parts in (1, 3, 5, 8, 64):
        count = rng.integers(-5, 2**40, (5, n_parts, 2)).astype(np.int64)
        total = rng.normal(0, 1e10, (5, n_parts))
        total[0, 0], total[1, 0], total[2, n_parts - 1] = -0.0, np.inf, np.array([0xFFF8000000012345], np.uint64).view(np.float64)[0]   # bits are copied
        for target in (tm.POSITIVE, tm.LABEL):
            t = engine.TargetTable.from_arrays(base, terms, count, total, target=target)
            assert (t.width, t.n_parts, t.target, t.p) == (5, n_parts, target, 12)
            lay = t.layout()
            assert np.array_equal(lay[0], base) and np.array_equal(lay[1], terms)
            _same_table(t, (count, total if target == tm.LABEL else None), (n_parts, target))
            again = engine.TargetTable.from_arrays(*t.layout(), *t.export(), target=target)
            _same_table(again, (count, total if target == tm.LABEL else None), (n_parts, target, "again"))
            t.free()
            again.free()
    assert engine.TargetTable.from_arrays(base, terms, np.zeros((5, 5, 2), np.int64)).device_bytes == 5 * 128   # a record of five parts is one 128-byte line


# --------------------------------------------------------------------------------------------------------------------------------- the apply
def _apply_model(name, table_key, count, total, target, part, kinds, prior, strength, keep):
    key = ("apply", name, table_key, target, None if part is None else part.tobytes(), tuple(kinds), prior, strength, keep)
    if key not in _cache:
        _, host, p, base, terms = _source(name)
        _cache[key] = tm.encode(host[0], host[1], host[2], p, base, terms, count, total, target, part, kinds, prior, strength, keep)
    return _cache[key]


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("target", [tm.POSITIVE, tm.LABEL])
def test_ragged_rows_equal_the_model_in_every_form(target, keep):
    m, host, p, base, terms = _source("ragged")
    part = tc.ragged_parts(m.n, 5)
    count, total = _stats_model("ragged", 5, target, part)
    table = m.target_stats(part, base, terms, n_parts=5, target=target)
    kinds = [3, 1, 2, 3, 1]
    for use, strength in ((part, 20.0), (None, 0.0), (part, 0.0)):
        ref = _apply_model("ragged", "fit", count, total, target, use, kinds, 0.3, strength, keep)
        lens = np.diff(ref[0]) - (np.diff(host[0]) if keep else 0)
        assert set(lens.tolist()) == {0, 1, 2, 3, 4}                                         # terms empty in some rows; the empty segment never emits
        for form, hook in APPLY_FORMS.items():
            _limits(*hook)
            out, eb = m.encode_targets(table, use, kinds=kinds, prior=0.3, strength=strength, keep_source=keep)
            assert out.n == m.n
            _same_matrix(out, eb, ref, host[3], (target, keep, use is None, strength, form))
            out.close()
    _limits()
    d = DevBuf.from_numpy(part)
    out, eb = m.encode_targets(table, kinds=kinds, prior=0.3, strength=20.0, keep_source=keep, dev_part=d.ptr)
    _same_matrix(out, eb, _apply_model("ragged", "fit", count, total, target, part, kinds, 0.3, 20.0, keep), host[3], "device part")
    out.close()
    table.free()
    src = m.export()
    assert np.array_equal(src[1], host[1]) and np.array_equal(tc.bits(src[2]), tc.bits(host[2]))   # the source is left as it was


@pytest.mark.parametrize("keep", [True, False])
@pytest.mark.parametrize("name", ["fields0", "fields2"])
def test_field_rows_equal_the_model_in_the_single_the_group_and_the_long_form(name, keep):
    from fmwr_amd import engine
    m, host, p, base, terms = _source(name)
    flags, layout = _state(m)
    assert flags["fixed_row_len"] == len(base) - 1 and len(layout["field_base"]) == 6       # the layout the single form needs
    part = engine.split_assign(m.n, n_folds=5, seed=3)
    for target in (tm.POSITIVE, tm.LABEL):
        count, total = _stats_model(name, 5, target, part)
        table = m.target_stats(part, base, terms, n_parts=5, target=target)
        for kinds in ([3] * len(terms), [1] * len(terms), [2] * len(terms), [1, 2, 3, 2, 1]):
            ref = _apply_model(name, "fit", count, total, target, part, kinds, 0.25, 20.0, keep)
            assert np.all(np.diff(ref[0]) == (len(base) - 1 if keep else 0) + sum(bin(k).count("1") for k in kinds))
            for form, hook in FIELD_FORMS.items():
                _limits(*hook)
                out, eb = m.encode_targets(table, part, kinds=kinds, prior=0.25, strength=20.0, keep_source=keep)
                _same_matrix(out, eb, ref, host[3], (name, target, keep, kinds, form))
                out.close()
        table.free()


@pytest.mark.parametrize("target", [tm.POSITIVE, tm.LABEL])
def test_injected_tables_round_once_and_an_empty_cell_gives_the_prior(target):
    """counts of 2^24 + 1 (COUNT rounds once from the integer), 2^53 + 1 (den rounds once) and 0 (strength 0: den == 0, MEAN is the prior)"""
    from fmwr_amd import engine
    m, host, p, base, terms = _source("ragged")
    rng = np.random.default_rng(4)
    W, P = 33, 5
    count = np.zeros((W, P, 2), np.int64)
    pool = np.array([2**24 + 1, 2**53 + 1, 0, 7, 2**24 + 3, 1], np.int64)
    count[:, :, 0] = pool[rng.integers(0, len(pool), (W, P))]
    count[:, :, 1] = count[:, :, 0] // 3
    count[1:6] = 0                                                                           # a field no part has seen
    count[6, :, 0], count[6, :, 1] = [2**24 + 1, 0, 0, 0, 0], 0
    total = rng.normal(0, 1e6, (W, P))
    total[7, 2], total[8, 0], total[9, 1], total[9, 3] = np.nan, -0.0, np.inf, -np.inf
    table = engine.TargetTable.from_arrays(base, terms, count, total, target=target)
    part = tc.ragged_parts(m.n, P)
    kinds = [3, 3, 3, 3, 3]
    for strength in (0.0, 20.0):
        for use in (part, None):
            ref = _apply_model("ragged", "injected", count, total, target, use, kinds, 0.3, strength, True)
            present, n, mean, cnt = tm.encode_values(host[0], host[1], p, base, terms, count, total, target, use, 0.3, strength)
            assert np.any(present & (n == 0)) and (strength > 0 or np.any(mean[present & (n == 0)] == tc.bits(np.float32(0.3))[0]))
            assert np.any(present & (n > 2**53))
            for form, hook in APPLY_FORMS.items():
                _limits(*hook)
                out, eb = m.encode_targets(table, use, kinds=kinds, prior=0.3, strength=strength)
                _same_matrix(out, eb, ref, host[3], (target, strength, use is None, form))
                out.close()
    table.free()


# ------------------------------------------------------------------------------------------------------------------------------ composition
def test_the_output_is_input_to_binning_fields_and_a_cross():
    """segment_base followed by enc_base[1:] is a segment list of the output: a cross takes it as it is; fmx_matrix_set_fields wants one value-1 id
    per field, which the new columns are once fmx_matrix_bin_columns has bucketed them -- new_base maps the segment list"""
    from fmwr_amd import engine
    m, host, p, base, terms = _source("fields0")
    part = engine.split_assign(m.n, n_folds=5, seed=3)
    count, total = _stats_model("fields0", 5, tm.POSITIVE, part)
    table = m.target_stats(part, base, terms, n_parts=5)
    kinds = [1, 1, 3, 1, 2]
    out, eb = m.encode_targets(table, part, kinds=kinds, prior=0.25, strength=20.0)
    ref = _apply_model("fields0", "fit", count, total, tm.POSITIVE, part, kinds, 0.25, 20.0, True)
    _same_matrix(out, eb, ref, host[3], "the source of the composition")
    copy = engine.Matrix.from_csr(ref[0], ref[1], ref[2], int(eb[-1]), host[3])
    assert _state(out) == _state(copy)                                                       # the flags of the uploaded copy of the model's output
    copy.close()
    seg = np.concatenate([base, eb[1:]]).astype(np.uint32)
    assert seg[-1] == out.p and np.all(np.diff(seg.astype(np.int64)) >= 0)
    crossed, cb = out.cross(seg, [(0, 5), (2, 7, 1000), (5, 9)], seed=3)
    want = cm.cross(ref[0], ref[1], ref[2], int(eb[-1]), seg, [(0, 5), (2, 7, 1000), (5, 9)], 3)
    got = crossed.export()
    assert np.array_equal(cb, want[3]) and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(tc.bits(got[2]), tc.bits(want[2]))
    crossed.close()
    cols = np.arange(int(eb[0]), int(eb[-1]), dtype=np.uint32)
    edges, _, _ = out.column_quantiles(cols, 4)
    binned, new_base = out.bin_columns(cols, edges)
    fields = new_base[np.concatenate([base, cols[1:], eb[-1:]])]                             # a field per new column: the term of two kinds is two of them
    assert fields[-1] == binned.p
    binned.set_fields(0, fields)                                                             # accepted: one id of every field in every row, value 1
    flags, layout = _state(binned)
    assert flags["unit_values"] == 1 and flags["fixed_row_len"] == len(fields) - 1 and layout["field_base"] == fields.tolist()
    binned.close()
    out.close()
    table.free()


def test_refusals_that_need_a_table():
    from fmwr_amd import _lib as L, engine
    m, host, p, base, terms = _source("ragged")
    table = m.target_stats(None, base, terms)
    other, _, _, _, _ = _source("tall")

    def refused(mat, kinds, keep=1, prior=0.3, strength=1.0):
        k = np.asarray(kinds, np.uint32)
        spec = L.EncodeSpec(C.sizeof(L.EncodeSpec), keep, k.ctypes.data, prior, strength, 0)
        got = np.full(len(terms) + 1, 7, np.uint32)
        h = C.c_void_p(5)
        st = L.lib().fmx_matrix_encode_targets(mat.h, table.h, None, C.byref(spec), got.ctypes.data_as(C.c_void_p), C.byref(h))
        assert st == L.ERR_INVALID and not h.value and np.all(got == 7)
        return L.lib().fmx_last_error().decode()
    assert "kinds[1]" in refused(m, [1, 0, 1, 1, 1]) and "kinds[4]" in refused(m, [1, 1, 1, 1, 4]) and "kinds[0]" in refused(m, [7, 1, 1, 1, 1])
    assert "features" in refused(other, [1] * 5)
    assert "strength" in refused(m, [1] * 5, strength=-1.0) and "strength" in refused(m, [1] * 5, strength=np.inf) and "prior" in refused(m, [1] * 5, prior=np.nan)
    unl = engine.Matrix.from_csr(host[0], host[1], host[2], p)
    with pytest.raises(L.FmxError, match="no labels"):
        unl.target_stats(None, base, terms)
    out, eb = unl.encode_targets(table, None, kinds=[2] * 5)                                 # the apply needs no labels
    assert out.n == unl.n and eb.tolist() == [41, 42, 43, 44, 45, 46]
    out.close()
    unl.close()
    table.free()


def test_widths_up_to_2_32_minus_2_are_taken_and_one_more_is_refused():
    from fmwr_amd import _lib as L, engine
    p = 2**32 - 3
    base, terms = np.array([0, 5, p], np.uint32), np.array([0], np.uint32)
    count = np.arange(10, dtype=np.int64).reshape(5, 1, 2)
    table = engine.TargetTable.from_arrays(base, terms, count)
    rp, col, val = np.array([0, 2, 2, 3], np.int64), np.array([4, p - 1, 0], np.uint32), np.array([1.5, 2.0, 1.0], np.float32)
    m = engine.Matrix.from_csr(rp, col, val, p)
    out, eb = m.encode_targets(table, None, kinds=[1], prior=0.5, strength=1.0)             # p + 1 = 2^32 - 2 features: taken
    _same_matrix(out, eb, tm.encode(rp, col, val, p, base, terms, count, None, tm.POSITIVE, None, [1], 0.5, 1.0, True), None, "the widest output", flags=False)
    assert out.p == 2**32 - 2 and eb.tolist() == [p, p + 1]
    out.close()
    kinds = np.array([3], np.uint32)
    spec = L.EncodeSpec(C.sizeof(L.EncodeSpec), 1, kinds.ctypes.data, 0.5, 1.0, 0)
    got = np.full(2, 7, np.uint32)
    h = C.c_void_p(5)
    assert L.lib().fmx_matrix_encode_targets(m.h, table.h, None, C.byref(spec), got.ctypes.data_as(C.c_void_p), C.byref(h)) == L.ERR_INVALID
    assert b"2^32 - 2" in L.lib().fmx_last_error() and not h.value and np.all(got == 7)
    out, eb = m.encode_targets(table, None, kinds=[3], keep_source=False)                    # without the source the two columns fit
    assert eb.tolist() == [0, 2] and out.p == 2 and out.nnz == 4
    out.close()
    m.close()
    table.free()


# ------------------------------------------------------------------------------------------------------------------------------- end to end
def _planted(n, n_ids, seed):
    import fmwr_amd as fm
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    rate = rng.random(n_ids)
    ids, ctx = rng.integers(0, n_ids, n), rng.integers(0, 4, n)
    y = np.where(rng.random(n) < rate[ids], 1.0, -1.0)
    col = np.stack([ids, n_ids + ctx], axis=1).ravel()
    X = sp.csr_matrix((np.ones(2 * n), col, np.arange(n + 1) * 2), shape=(n, n_ids + 4))
    names = [f"id{i}" for i in range(n_ids)] + [f"c{i}" for i in range(4)]
    return fm.fm_matrix(X, y, feature_names=names)


def test_encode_train_apply_metrics_end_to_end():
    """A high-cardinality field with five rows per id and a per-id rate: fm_encode_targets -> fm_train -> fm_apply_targets -> fm_metrics.  The
    device-made columns equal the model's bit for bit; training and the metrics run and are finite."""
    import fmwr_amd as fm
    n_ids = 600
    data = _planted(3000, n_ids, 21)
    train, test, _ = fm.fm_split(data, test_fraction=0.25, seed=1)
    fields = [0, n_ids, n_ids + 4]
    enc_train, encoding = fm.fm_encode_targets(train, fields, [0], folds=5, kinds=("mean", "count"), strength=20.0, seed=9)
    assert enc_train.dim[1] == n_ids + 6 and enc_train.feature_names[-2:] == ["te(0)", "cnt(0)"] and encoding.new_segment_base.tolist() == fields + [n_ids + 6]
    assert encoding.target == "positive" and encoding.prior == float(np.mean(np.asarray(train.labels) > 0)) and encoding.count.shape == (n_ids, 5, 2)
    # the model on the same rows, folds and table
    f = train.features
    rp = np.concatenate([[0], np.cumsum(f["row_size"])]).astype(np.int64)
    y = np.asarray(train.labels, np.float32)
    part = fm.fm_folds(train, 5, seed=9).astype(np.uint32)
    count, _ = tm.target_stats(rp, f["col_idx"], y, n_ids + 4, fields, [0], 5, tm.POSITIVE, part)
    assert np.array_equal(encoding.count, count) and encoding.sum is None
    ref = tm.encode(rp, f["col_idx"], f["value"], n_ids + 4, fields, [0], count, None, tm.POSITIVE, part, [3], encoding.prior, 20.0, True)
    g = enc_train.features
    assert np.array_equal(g["row_size"], np.diff(ref[0])) and np.array_equal(g["col_idx"], ref[1].astype(np.int32))
    assert np.array_equal(tc.bits(g["value"]), tc.bits(ref[2]))
    again = pickle.loads(pickle.dumps(encoding))
    enc_test = fm.fm_apply_targets(test, again)
    tf = test.features
    trp = np.concatenate([[0], np.cumsum(tf["row_size"])]).astype(np.int64)
    tref = tm.encode(trp, tf["col_idx"], tf["value"], n_ids + 4, fields, [0], count, None, tm.POSITIVE, None, [3], encoding.prior, 20.0, True)
    assert np.array_equal(enc_test.features["col_idx"], tref[1].astype(np.int32)) and np.array_equal(tc.bits(enc_test.features["value"]), tc.bits(tref[2]))
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 4, "v.init_stdev": 0.1}),
           fm.solver_control(max_iter=20 * enc_train.dim[0], solver=fm.SGD_solver(learn_rate=0.05))]
    model = fm.fm_train(enc_train, normalize=False, seed=1, control=ctl, mode="minibatch", batch_rows=256)
    met = fm.fm_metrics(model, enc_test, normalize=False)["pooled"]
    print({k: float(v) for k, v in met.items() if np.isscalar(v)})
    assert all(np.isfinite(met[k]) for k in ("auc", "logloss", "accuracy"))
