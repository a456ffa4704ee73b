"""fmx_matrix_take / fmx_split_assign / fmx_matrix_select / fmx_matrix_split_entries / fmx_row_permutation and fm_split / fm_folds / fm_holdout
against the numpy model of the definition (tests/split_model.py).  Everything is integers and copied bits: every comparison is exact equality,
in every form of the gather and on its boundaries (the hook lowers them to 4 and 8 entries and the launches to 16 rows)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import split_model as sm
from tests.util import DevBuf, read_device

pytestmark = pytest.mark.gpu

LONG = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]   # the flat form by default (a row of more than 512 entries)
HOOKS = {"default": (0, 0, 0), "at4": (4, 4, 16), "at8": (8, 8, 16), "flat": (-1, -1, 16)}   # fmx_debug_take_limits' arguments


def _limits(fixed=0, group=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_take_limits(fixed, group, rows))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _csr(lens, p, seed, unit=False):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(p, int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = np.ones(len(col), np.float32) if unit else rng.normal(0, 1, len(col)).astype(np.float32)
    y = np.where(rng.random(len(lens)) < 0.5, 1.0, -1.0).astype(np.float32)
    return rp, col, val, y


def _matrix(host, p, labels=True):
    from fmwr_amd import engine
    rp, col, val, y = host
    return engine.Matrix.from_csr(rp, col, val, p, y if labels else None)


def _lens(kind):
    rng = np.random.default_rng(2)
    if kind == "long":
        return rng.permutation(np.concatenate([LONG, rng.integers(0, 10, 40 - len(LONG))]))
    if kind == "short":   # the lane-group form by default
        return rng.permutation(np.concatenate([LONG[:-1], rng.integers(0, 10, 40 - len(LONG) + 1)]))
    if kind == "mid":     # rows of at most 64 entries
        return rng.permutation(np.concatenate([LONG[:9], rng.integers(0, 10, 31)]))
    return rng.permutation(np.concatenate([[0, 1, 2, 3, 4, 5, 7, 8], rng.integers(0, 9, 32)]))   # "tiny": rows of at most 8 entries


def _row_lists(n, seed=3):
    rng = np.random.default_rng(seed)
    return {"identity": np.arange(n), "reverse": np.arange(n)[::-1].copy(), "bootstrap": rng.integers(0, n, n), "empty": np.zeros(0, np.int64),
            "one": np.array([n // 2]), "three_n": rng.integers(0, n, 3 * n)}


def _same_matrix(m, ref, labels, what=""):
    rp, col, val, y = m.export()
    rrp, rcol, rval, ry = ref
    assert m.n == len(rrp) - 1 and m.nnz == int(rrp[-1]), what
    assert np.array_equal(rp, rrp), (what, "row_ptr")
    assert np.array_equal(col, rcol), (what, "col")
    assert np.array_equal(val.view(np.uint32), np.asarray(rval, np.float32).view(np.uint32)), (what, "value bits")
    if labels:
        assert np.array_equal(y.view(np.uint32), np.asarray(ry, np.float32).view(np.uint32)), (what, "label bits")
    else:
        assert not y.any(), (what, "labels of an unlabelled matrix")


def _check_takes(m, host, labels, what):
    for name, rows in _row_lists(m.n).items():
        out = m.take(rows)
        assert out.p == m.p
        _same_matrix(out, sm.take(*host, rows), labels, (what, name))
        out.close()


# ------------------------------------------------------------------------------------------------------------------------------ take
@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("labels,unit", [(True, False), (False, False), (True, True), (False, True)])
def test_take_ragged_rows_with_and_without_labels_and_values(labels, unit, hook):
    host = _csr(_lens("long"), 3000, 5, unit)
    m = _matrix(host, 3000, labels)
    _limits(*HOOKS[hook])
    _check_takes(m, host, labels, (labels, unit, hook))


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("kind", ["short", "tiny"])
def test_take_reaches_the_group_form_and_its_boundary(kind, hook):
    """default limits: both sources take the lane-group form.  "tiny" holds rows of at most 8 entries: group limit 8 keeps the form (the boundary
    is inclusive); under limit 4 the source's longest row no longer settles it and the longest OUTPUT row, measured in the length pass, decides:
    the identity, reverse and three_n lists hold the 8-entry row and take the flat form, a list of rows of at most 4 entries keeps the group
    form."""
    host = _csr(_lens(kind), 3000, 6)
    m = _matrix(host, 3000)
    _limits(*HOOKS[hook])
    _check_takes(m, host, True, (kind, hook))


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("L,unit", [(8, False), (6, False), (6, True), (30, False), (1, False)])
def test_take_fixed_length_rows(L, unit, hook):
    """every row of L entries: the fixed form (16-byte reads for L = 8, word reads and pieces that straddle rows for 6, 30 and 1); with a
    limit of 4 the 8-entry source goes on to the other forms, with 8 it stays (inclusive)"""
    host = _csr(np.full(45, L), 500, 7 + L, unit)
    m = _matrix(host, 500)
    _limits(*HOOKS[hook])
    _check_takes(m, host, True, (L, unit, hook))


@pytest.mark.parametrize("hook", ["default", "at4", "flat"])
@pytest.mark.parametrize("n_dense", [0, 2])
def test_take_field_layout_source(n_dense, hook):
    from fmwr_amd import engine
    m = engine.Matrix.synthetic_fields(300, n_dense, [50, 40, 30, 7], 1.1, 9)
    host = m.export()
    assert np.all(np.diff(host[0]) == n_dense + 4)
    _limits(*HOOKS[hook])
    _check_takes(m, host, True, (n_dense, hook))


def test_take_host_and_device_forms_agree_and_refuse_bad_ids():
    from fmwr_amd import _lib as L
    host = _csr(_lens("long"), 3000, 5)
    m = _matrix(host, 3000)
    rows = _row_lists(m.n)["three_n"].astype(np.int64)
    d = DevBuf.from_numpy(rows)
    for hook in ("default", "at8"):
        _limits(*HOOKS[hook])
        out = m.take_device(d.ptr, len(rows))
        _same_matrix(out, sm.take(*host, rows), True, hook)
        out.close()
    empty = m.take_device(None, 0)
    assert empty.n == 0 and empty.nnz == 0 and empty.p == m.p
    for bad in (m.n, -1, 2 ** 40):
        wrong = rows.copy()
        wrong[17] = bad
        h = C.c_void_p(1)
        assert L.lib().fmx_matrix_take(m.h, wrong.ctypes.data_as(C.c_void_p), len(wrong), C.byref(h)) == L.ERR_INVALID and not h.value
        assert b"rows[17]" in L.lib().fmx_last_error()
        d.upload(wrong)
        h = C.c_void_p(1)
        assert L.lib().fmx_matrix_take_device(m.h, d.ptr, len(wrong), C.byref(h)) == L.ERR_INVALID and not h.value
        assert b"rows[17]" in L.lib().fmx_last_error()
    with pytest.raises(L.FmxError):
        m.take([0, m.n])
    with pytest.raises(ValueError):
        m.take(np.array([0.5, 1.0]))


# ------------------------------------------------------------------------------------------------- take is the gather of one block
_ONE_BLOCK = {}


def _one_block_sources():
    """(host arrays, device Matrix) of the sources the take and the one-block join are compared on, made once"""
    if not _ONE_BLOCK:
        _ONE_BLOCK["long"] = (_csr(_lens("long"), 3000, 5), 3000)
        _ONE_BLOCK["tiny"] = (_csr(_lens("tiny"), 3000, 6), 3000)
        for L, unit in ((1, False), (6, False), (8, False), (30, False), (6, True)):
            _ONE_BLOCK[f"fixed{L}{'_unit' if unit else ''}"] = (_csr(np.full(45, L), 500, 7 + L, unit), 500)
        for name, (host, p) in list(_ONE_BLOCK.items()):
            _ONE_BLOCK[name] = (host, _matrix(host, p))
    return _ONE_BLOCK


def _join_limits(fixed=0, group=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_join_limits(fixed, group, rows))


@pytest.mark.parametrize("hooks", [(h, h) for h in HOOKS] + [("flat", "default")])
def test_take_is_the_join_of_one_block(hooks):
    """Matrix.join of the single block (m, rows, col_base 0) with the labels of block 0 and out_p = m.p is m.take(rows): row pointers, columns,
    value bits and label bits, under every setting of the two hooks -- and with the two set differently, since each keeps its own values."""
    from fmwr_amd import engine
    try:
        for name, (host, m) in _one_block_sources().items():
            for lname, rows in _row_lists(m.n).items():
                _limits(*HOOKS[hooks[0]])
                _join_limits(*HOOKS[hooks[1]])
                taken = m.take(rows)
                joined = engine.Matrix.join([(m, rows, 0)], n=len(rows), p=m.p, labels_from=0)
                ref = sm.take(*host, rows)
                _same_matrix(taken, ref, True, (name, lname, hooks, "take"))
                _same_matrix(joined, ref, True, (name, lname, hooks, "join"))
                _same_matrix(joined, taken.export(), True, (name, lname, hooks))
                assert joined.p == taken.p == m.p
                taken.close(); joined.close()
    finally:
        _join_limits()


def _flags(m):
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    return dict(rows_sorted=int(out[0]), unit_values=int(out[1]), fixed_row_len=int(out[2]), max_row_len=int(out[3]), fields=int(out[4]))


@pytest.mark.parametrize("n_dense", [0, 2])
def test_a_taken_field_layout_keeps_the_flags_of_its_source(n_dense):
    """take's own rule, not a join's: the layout of a synthetic_fields source -- rows_sorted, unit_values, max_row_len, fixed_row_len, the fields and
    with them the dense prefix (fixed_row_len - fields) -- goes on to every take of it, a dense prefix included"""
    from fmwr_amd import engine
    m = engine.Matrix.synthetic_fields(300, n_dense, [50, 40, 30, 7], 1.1, 9)
    src = _flags(m)
    assert src["fields"] == 4 and src["fixed_row_len"] - src["fields"] == n_dense and src["max_row_len"] == n_dense + 4
    lists = _row_lists(m.n)
    for lname in ("identity", "bootstrap"):
        t = m.take(lists[lname])
        assert _flags(t) == src, (lname, _flags(t), src)
        t.close()


def test_a_taken_ragged_matrix_has_the_flags_of_an_upload():
    host = _csr(_lens("long"), 3000, 5)
    m = _matrix(host, 3000)
    for lname, rows in _row_lists(m.n).items():
        t = m.take(rows)
        rp, col, val, y = sm.take(*host, rows)
        copy = _matrix((rp, col, val, y), 3000)
        assert _flags(t) == _flags(copy), (lname, _flags(t), _flags(copy))
        t.close(); copy.close()


def test_a_bad_id_is_refused_in_takes_own_words():
    """an id out of range at position 17 of a 40-row list: FMX_ERR_INVALID, *out = NULL, and the message names rows[17] as a take does, not as
    the join whose core ran it (`of block`), in the host and in the device form"""
    from fmwr_amd import _lib as L
    host = _csr(_lens("long"), 3000, 5)
    m = _matrix(host, 3000)
    rows = np.random.default_rng(3).integers(0, m.n, 40).astype(np.int64)
    d = DevBuf.from_numpy(rows)
    for bad in (m.n, -1):
        wrong = rows.copy()
        wrong[17] = bad
        d.upload(wrong)
        for call, arg in ((L.lib().fmx_matrix_take, wrong.ctypes.data_as(C.c_void_p)), (L.lib().fmx_matrix_take_device, d.ptr)):
            h = C.c_void_p(1)
            assert call(m.h, arg, len(wrong), C.byref(h)) == L.ERR_INVALID and not h.value
            msg = L.lib().fmx_last_error()
            assert b"rows[17]" in msg and b"of block" not in msg, msg


# ------------------------------------------------------------------------------------------------------------------ flags do their job
def _engine(p, k, fp64, seed=0, **kw):
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=64, state_fp64=int(fp64), num_factor=k, task=L.TASK_CLASSIFICATION, learn_rate=0.05, **kw)
    rng = np.random.default_rng(seed + 3)
    e.set_params(0.2, rng.normal(0, 0.3, p), rng.normal(0, 0.3, (k, p)))
    return e


def _sources():
    from fmwr_amd import engine
    ragged = _matrix(_csr(_lens("mid"), 3000, 6), 3000)
    fields = engine.Matrix.synthetic_fields(320, 2, [50, 40, 30, 7], 1.1, 9)
    return {"ragged": ragged, "fields": fields}


@pytest.mark.parametrize("fp64", [False, True])
def test_predict_of_taken_rows_is_predict_of_the_rows(fp64):
    """A permutation of the source's rows: the same number of rows, so the forward takes the same schedule, and the same flags.  The rows hold
    at most 64 entries: a launch this small gives a row to four lane groups, counted from the start of the 512 entries its workgroup stages at a
    time, so a row that crosses such a chunk is summed in an order that depends on its neighbours; eight rows (four with fp64 tables) of at most
    64 entries never cross one, and a row's bits are then its own."""
    for name, m in _sources().items():
        e = _engine(m.p, 5, fp64)
        rows = np.random.default_rng(4).permutation(m.n)
        t = m.take(rows)
        a, b = e.predict(t), e.predict(m)[rows]
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), name


def test_five_steps_on_the_identity_take_leave_the_same_parameters():
    for name, m in _sources().items():
        t = m.take(np.arange(m.n))
        params = []
        for mat in (m, t):
            e = _engine(m.p, 4, False, seed=1)
            nb = e.num_batches(mat)
            for b in range(5):
                e.step(mat, b % nb)
            params.append(e.get_params())
        assert params[0][0] == params[1][0], name
        assert np.array_equal(params[0][1].view(np.uint64), params[1][1].view(np.uint64)), name
        assert np.array_equal(params[0][2].view(np.uint64), params[1][2].view(np.uint64)), name


# ---------------------------------------------------------------------------------------------------------------------------- assign
SIZES = [0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025]
RULES = [dict(hold_count=3, min_keep=0), dict(hold_count=3, min_keep=1), dict(hold_fraction=0.3, min_keep=0), dict(hold_fraction=0.3, min_keep=1),
         dict(n_folds=2), dict(n_folds=3), dict(n_folds=10), dict(hold_count=2000, min_keep=5)]


def _groups():
    g = np.repeat(np.arange(len(SIZES)), SIZES)
    return np.random.default_rng(8).permutation(g).astype(np.uint32), len(SIZES)


@pytest.mark.parametrize("scope", [sm.ROWS, sm.WITHIN_GROUPS, sm.GROUPS])
@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_assign_equals_the_model(scope, order):
    from fmwr_amd import engine
    g, G = _groups()
    n = len(g)
    dg, dp = DevBuf.from_numpy(g), DevBuf(n, np.uint32)
    for rule in RULES:
        ref = sm.assign(n, g, G, scope=scope, order=order, seed=77, salt=3, **rule)
        got = engine.split_assign(n, g, G, scope=scope, order=order, seed=77, salt=3, **rule)
        assert got.dtype == np.uint32 and np.array_equal(got, ref), (scope, order, rule)
        assert np.array_equal(engine.split_assign(n, g, G, scope=scope, order=order, seed=77, salt=3, **rule), got)   # a second call
        engine.split_assign_device(n, dg.ptr, G, dp.ptr, scope=scope, order=order, seed=77, salt=3, **rule)
        assert np.array_equal(dp.numpy(), ref), ("device form", scope, order, rule)
    if scope == sm.ROWS:   # no groups at all
        ref = sm.assign(n, scope=sm.ROWS, order=order, hold_fraction=0.2, seed=5)
        assert np.array_equal(engine.split_assign(n, scope=sm.ROWS, order=order, hold_fraction=0.2, seed=5), ref)
        engine.split_assign_device(n, None, 1, dp.ptr, scope=sm.ROWS, order=order, hold_fraction=0.2, seed=5)
        assert np.array_equal(dp.numpy(), ref)
    assert len(engine.split_assign(0, scope=sm.ROWS)) == 0
    assert engine.split_assign(1, scope=sm.ROWS, hold_count=1).tolist() == [1]


@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_assign_within_groups_sees_only_the_group_and_marks_ids_out_of_range(order):
    from fmwr_amd import engine
    g, G = _groups()
    n = len(g)
    dp = DevBuf(n, np.uint32)
    for rule in (dict(hold_count=3, min_keep=1), dict(n_folds=3)):
        ref = engine.split_assign(n, g, G, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule)
        renumbered = (G - 1 - g.astype(np.int64) + 30).astype(np.uint32)
        assert np.array_equal(engine.split_assign(n, renumbered, G + 30, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule), ref)
        gone = np.where(g == 8, 8, 5000).astype(np.uint32)   # the other groups dropped: ids out of range, device form
        dgone = DevBuf.from_numpy(gone)
        engine.split_assign_device(n, dgone.ptr, G, dp.ptr, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule)
        got = dp.numpy()
        assert np.array_equal(got[g == 8], ref[g == 8]) and np.all(got[g != 8] == 0xFFFFFFFF)
        assert np.array_equal(got, sm.assign(n, gone, G, scope=sm.WITHIN_GROUPS, order=order, seed=9, **rule))
        engine.split_assign_device(n, dgone.ptr, G, dp.ptr, scope=sm.GROUPS, order=order, seed=9, **rule)
        assert np.array_equal(dp.numpy(), sm.assign(n, gone, G, scope=sm.GROUPS, order=order, seed=9, **rule))
    from fmwr_amd import _lib as L
    with pytest.raises(L.FmxError):
        engine.split_assign(n, np.where(g == 8, 8, 5000).astype(np.uint32), G, scope=sm.WITHIN_GROUPS)   # the host form refuses them


# ---------------------------------------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("hook", ["default", "at8"])
def test_select_is_boolean_indexing_and_the_folds_partition_the_rows(hook):
    from fmwr_amd import engine
    host = _csr(_lens("long"), 3000, 5)
    m = _matrix(host, 3000)
    K = 3
    part = engine.split_assign(m.n, scope=sm.ROWS, n_folds=K, seed=4)
    part[[3, 11]] = 0xFFFFFFFF   # rows without a part: in no fold, and in no complement
    _limits(*HOOKS[hook])
    seen = []
    dpart = DevBuf.from_numpy(part)
    for f in range(K):
        test, rows = m.select(part, f, return_rows=True)
        assert np.array_equal(rows, np.flatnonzero(part == f)) and np.array_equal(rows, sm.select_rows(part, f))
        _same_matrix(test, sm.take(*host, rows), True, ("test", f))
        train, trows = m.select(part, f, complement=True, return_rows=True)
        assert np.array_equal(trows, np.flatnonzero((part != f) & (part != 0xFFFFFFFF)))
        _same_matrix(train, sm.take(*host, trows), True, ("train", f))
        assert np.array_equal(np.sort(np.concatenate([rows, trows])), np.setdiff1d(np.arange(m.n), [3, 11]))
        seen.append(rows)
        dev, ptr = m.select_device(dpart.ptr, f)
        assert np.array_equal(read_device(ptr, dev.n, np.int64), rows)
        engine.free_device(ptr)
        _same_matrix(dev, sm.take(*host, rows), True, ("device", f))
    assert np.array_equal(np.sort(np.concatenate(seen)), np.setdiff1d(np.arange(m.n), [3, 11]))
    none = m.select(part, 7)
    assert none.n == 0 and none.nnz == 0
    lost, rows = m.select(part, 0xFFFFFFFF, return_rows=True)
    assert rows.tolist() == [3, 11]
    with pytest.raises(ValueError):
        m.select(part[:-1], 0)


# --------------------------------------------------------------------------------------------------------------------- split_entries
@pytest.mark.parametrize("order", [sm.ORDER_HASH, sm.ORDER_TAIL])
def test_split_entries_equals_the_model(order):
    lens = np.array([0, 1, 2, 3, 64, 65, 1025, 0, 5])
    rp, col, val, y = _csr(lens, 4000, 12)
    col[rp[4] + 1] = col[rp[4] + 40]   # a column stored twice in one row: equal keys, position decides
    m = _matrix((rp, col, val, y), 4000)
    for rule in (dict(hold_count=1, min_keep=1), dict(hold_count=0, hold_fraction=0.5, min_keep=0), dict(hold_count=70, min_keep=2)):
        kept, held = m.split_entries(hold=rule["hold_count"], fraction=rule.get("hold_fraction") if rule["hold_count"] == 0 else None, order=order,
                                     min_keep=rule["min_keep"], seed=8, salt=1)
        (krp, kcol, kval), (hrp, hcol, hval) = sm.split_entries(rp, col, val, order=order, seed=8, salt=1, **rule)
        _same_matrix(kept, (krp, kcol, kval, y), True, ("kept", order, rule))
        _same_matrix(held, (hrp, hcol, hval, y), True, ("held", order, rule))
        assert kept.nnz + held.nnz == m.nnz and kept.n == held.n == m.n
    kept, held = m.split_entries(hold=1, min_keep=1, order=order)
    hl = np.diff(held.export()[0])
    assert np.array_equal(hl, (lens >= 2).astype(np.int64))   # leave-one-out that never empties a row
    unl = _matrix((rp, col, val, y), 4000, labels=False)
    k2, h2 = unl.split_entries(hold=2, min_keep=0, order=order, seed=3)
    assert not k2.export()[3].any() and k2.nnz + h2.nnz == m.nnz
    empty = _matrix((np.zeros(4, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), np.ones(3, np.float32)), 10)
    k3, h3 = empty.split_entries()
    assert k3.n == h3.n == 3 and k3.nnz == h3.nnz == 0


# ----------------------------------------------------------------------------------------------------------------------- permutation
def test_permutation_equals_the_model_and_shuffled_round_trips():
    from fmwr_amd import engine
    n = 5000
    a = engine.row_permutation(n, 5, 0)
    assert a.dtype == np.int64 and np.array_equal(a, sm.permutation(n, 5, 0))
    assert np.array_equal(np.sort(a), np.arange(n))
    b = engine.row_permutation(n, 5, 1)
    assert np.array_equal(b, sm.permutation(n, 5, 1)) and not np.array_equal(a, b)
    d = DevBuf(n, np.int64)
    engine.row_permutation_device(n, 5, 1, d.ptr)
    assert np.array_equal(d.numpy(), b)
    assert len(engine.row_permutation(0, 1, 1)) == 0
    host = _csr(_lens("long"), 3000, 5)
    m = _matrix(host, 3000)
    s = m.shuffled(21, 3)
    perm = engine.row_permutation(m.n, 21, 3)
    _same_matrix(s, sm.take(*host, perm), True, "shuffled")
    back = s.take(np.argsort(perm))
    _same_matrix(back, host, True, "round trip")
    dinv = DevBuf.from_numpy(np.argsort(perm).astype(np.int64))
    e = s.take_device(dinv.ptr, m.n)
    _same_matrix(e, host, True, "round trip, device form")


# ------------------------------------------------------------------------------------------------------------------------ end to end
def _labelled(n=400, p=30, seed=13):
    rng = np.random.default_rng(seed)
    X = sp.random(n, p, density=0.2, random_state=3, format="csr")
    X.data = rng.normal(0, 1, X.nnz).astype(np.float32).astype(np.float64)
    X.sort_indices()
    y = np.where(X @ rng.normal(0, 1, p) + rng.normal(0, 0.5, n) > 0, 1.0, 0.0)
    return X, y, rng.integers(100, 140, n) * 7


def test_fm_split_then_train_then_metrics():
    import fmwr_amd as fm
    X, y, users = _labelled()
    data = fm.fm_matrix(X, y)
    train, test, mask = fm.fm_split(data, test_fraction=0.25, seed=3)
    ref = sm.assign(400, scope=sm.ROWS, hold_fraction=0.25, seed=3) == 1
    assert np.array_equal(mask, ref) and mask.sum() == 100 and train.dim == (300, 30) and test.dim == (100, 30)
    for part, keep in ((train, ~ref), (test, ref)):
        sub = X[np.flatnonzero(keep)]
        assert np.array_equal(part.features["value"], sub.data) and np.array_equal(part.features["col_idx"], sub.indices)
        assert np.array_equal(part.features["row_size"], np.diff(sub.indptr)) and np.array_equal(part.labels, y[keep])
        assert part.feature_names == data.feature_names
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=3000, solver=fm.SGD_solver())]
    fit = fm.fm_train(train, normalize=False, seed=1, control=ctl)
    out = fm.fm_metrics(fit, test, normalize=False)
    assert out["counts"]["rows"][0] == 100 and out["pooled"]["auc"] > 0.6
    # by user: no user on both sides; inside users: one row of every user, the last one
    tr, te, mk = fm.fm_split(data, test_fraction=0.3, by=users, how="groups", seed=2)
    assert not set(users[mk]) & set(users[~mk]) and len(set(users[mk])) == int(np.floor(0.3 * len(set(users))))
    tr, te, mk = fm.fm_split(data, test_count=1, by=users, how="within", order="last", min_keep=1)
    for u in np.unique(users):
        rows = np.flatnonzero(users == u)
        assert mk[rows].tolist() == ([False] * (len(rows) - 1) + [True] if len(rows) > 1 else [False])
    assert te.dim[0] == mk.sum() and tr.dim[0] == 400 - mk.sum()


def test_fm_folds():
    import fmwr_amd as fm
    X, y, users = _labelled()
    data = fm.fm_matrix(X, y)
    folds = fm.fm_folds(data, 3, seed=6)
    assert folds.dtype == np.int64 and np.array_equal(folds, sm.assign(400, scope=sm.ROWS, n_folds=3, seed=6))
    assert sorted(np.bincount(folds).tolist()) == [133, 133, 134]
    by_user = fm.fm_folds(data, 3, by=users, how="groups", seed=6)
    assert all(len(set(by_user[users == u])) == 1 for u in np.unique(users))
    dense = np.unique(users, return_inverse=True)[1]
    assert np.array_equal(by_user, sm.assign(400, dense, dense.max() + 1, scope=sm.GROUPS, n_folds=3, seed=6))
    strat = fm.fm_folds(data, 3, by=y.astype(np.int64), how="within", seed=6)
    for lab in (0, 1):
        sizes = np.bincount(strat[y == lab], minlength=3)
        assert sizes.max() - sizes.min() <= 1


def test_fm_holdout_then_train_rank_then_recommend_metrics():
    import fmwr_amd as fm
    rng = np.random.default_rng(5)
    n_users, n_items, k = 50, 40, 4
    S = rng.normal(0, 1, (n_users, k)) @ rng.normal(0, 1, (n_items, k)).T
    positives = [np.argsort(-S[u])[:rng.integers(1, 9)] for u in range(n_users)]
    p = n_users + n_items
    ctx = fm.fm_matrix(sp.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, p)))
    items = fm.fm_matrix(sp.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, p)))
    train, held = fm.fm_holdout(positives, hold=1, min_keep=1, seed=4)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in positives])])
    mask = sm.entries_held(rp, np.concatenate(positives), hold_count=1, min_keep=1, seed=4)
    for u in range(n_users):
        mu = mask[rp[u]:rp[u + 1]]
        assert np.array_equal(held[u], positives[u][mu]) and np.array_equal(train[u], positives[u][~mu])
        assert len(held[u]) == (1 if len(positives[u]) > 1 else 0)
    last = fm.fm_holdout(positives, hold=2, min_keep=0, order="last")
    assert all(np.array_equal(last[1][u], positives[u][max(len(positives[u]) - 2, 0):]) for u in range(n_users))
    P = sp.csr_matrix((np.ones(rp[-1]), np.concatenate(positives), rp), shape=(n_users, n_items))
    tr_s, he_s = fm.fm_holdout(P, hold=1, min_keep=1, seed=4)
    assert sp.issparse(tr_s) and tr_s.shape == (n_users, n_items) and (tr_s + he_s != P).nnz == 0 and he_s.nnz == sum(len(h) for h in held)
    ctl = [fm.model_control("RANK", **{"factor.number": 4, "v.init_stdev": 0.1}), fm.solver_control(solver=fm.SGD_solver(learn_rate=0.1))]
    fit = fm.fm_train_rank(ctx, items, train, control=ctl, n_neg=2, epochs=5, seed=3, batch_rows=256)
    out = fm.fm_recommend_metrics(fit, ctx, items, held, k=10, exclude=train, normalize=False)
    assert out["n_contexts"] == sum(1 for h in held if len(h)) and 0.0 <= out["recall@10"] <= 1.0
