"""fmx_matrix_join / fmx_matrix_stack and fm_design / fm_stack against the numpy model of the definition (tests/join_model.py).  Everything is
copied bits: every comparison of matrices is exact equality of row pointers, column ids, value bits and label bits, in every form of the copy and
on its boundaries (the hook lowers them to 4 and 8 entries and the launches to 16 rows)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import join_model as jm
from tests import split_model as sm
from tests.util import DevBuf

pytestmark = pytest.mark.gpu

LONG = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025]   # the flat form by default (a joined row of more than 512 entries)
# fmx_debug_join_limits' arguments: the boundaries at 4 and at 8 entries, each form forced (the fixed form is the default of a join whose blocks
# all have a fixed row length), 16 rows per launch
HOOKS = {"default": (0, 0, 0), "at4": (4, 4, 16), "at8": (8, 8, 16), "group": (-1, 0, 0), "flat": (-1, -1, 16), "launch16": (0, 0, 16)}
VOCAB = [50, 40, 30, 7]
N = 40


def _limits(fixed=0, group=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_join_limits(fixed, group, rows))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _flags(m):
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    return dict(rows_sorted=int(out[0]), unit_values=int(out[1]), fixed_row_len=int(out[2]), max_row_len=int(out[3]), fields=int(out[4]))


def _csr(lens, p, seed, unit=False):
    rng = np.random.default_rng(seed)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(p, int(n), replace=False)) for n in lens] + [np.zeros(0, np.int64)]).astype(np.uint32)
    val = np.ones(len(col), np.float32) if unit else rng.normal(0, 1, len(col)).astype(np.float32)
    y = rng.normal(0, 1, len(lens)).astype(np.float32)
    return rp, col, val, y


_CACHE = {}


def _src(name):
    """(host arrays, device Matrix) of a named source, made once"""
    if name not in _CACHE:
        from fmwr_amd import engine
        rng = np.random.default_rng(2)
        kind, _, rest = name.partition(":")
        if kind == "fields":      # synthetic_fields with `rest` dense columns: a field layout
            m = engine.Matrix.synthetic_fields(N, int(rest), VOCAB, 1.1, 9)
            _CACHE[name] = (m.export(), m)
            return _CACHE[name]
        unit, labels = "unit" in rest, "unl" not in rest
        if kind == "long":
            lens, p = rng.permutation(np.concatenate([LONG, rng.integers(0, 10, N - len(LONG))])), 3000
        elif kind == "short":     # rows of at most 64 entries
            lens, p = rng.permutation(np.concatenate([LONG[:9], rng.integers(0, 10, N - 9)])), 3000
        elif kind == "tiny":      # rows of at most 4 entries
            lens, p = rng.integers(0, 5, N), 3000
        else:                     # "fixedL": every row of L entries
            lens, p = np.full(N, int(kind[5:])), 500
        host = _csr(lens, p, 5 + len(name), unit)
        host = host if labels else host[:3] + (None,)
        _CACHE[name] = (host, engine.Matrix.from_csr(host[0], host[1], host[2], p, host[3]))
    return _CACHE[name]


def _width(name):
    return name if isinstance(name, int) else _src(name)[1].p


def _id_lists(seed=3):
    rng = np.random.default_rng(seed)
    return {"identity": None, "reverse": np.arange(N)[::-1].copy(), "bootstrap": rng.integers(0, N, N), "all_equal": np.full(N, 7),
            "empty": np.zeros(0, np.int64), "one": np.array([N // 2]), "three_n": rng.integers(0, N, 3 * N)}


def _same_matrix(m, ref, what=""):
    rp, col, val, y = m.export()
    rrp, rcol, rval, ry = ref
    assert m.n == len(rrp) - 1 and m.nnz == int(rrp[-1]), what
    assert np.array_equal(rp, rrp), (what, "row_ptr")
    assert np.array_equal(col, rcol), (what, "col")
    assert np.array_equal(val.view(np.uint32), np.asarray(rval, np.float32).view(np.uint32)), (what, "value bits")
    if ry is not None:
        assert np.array_equal(y.view(np.uint32), np.asarray(ry, np.float32).view(np.uint32)), (what, "label bits")
    else:
        assert not y.any(), (what, "labels of an unlabelled matrix")


def _join(names, rows, bases, out_p=None, labels_from=None, device_form=False):
    """(device join, model join) of the named blocks (a name, or an int: an indicator block of that many ids)"""
    from fmwr_amd import engine
    n_out = next((len(r) for r in rows if r is not None), N)
    if out_p is None:
        out_p = max(b + _width(s) for s, b in zip(names, bases))
    model = jm.join([(s if isinstance(s, int) else _src(s)[0], r, b) for s, r, b in zip(names, rows, bases)], n_out, out_p, labels_from)
    if device_form:
        keep = [None if r is None else DevBuf.from_numpy(np.ascontiguousarray(r, np.int64)) for r in rows]
        got = engine.Matrix.join_device([(s if isinstance(s, int) else _src(s)[1], None if k is None else k.ptr, b) for s, k, b in zip(names, keep, bases)],
                                        n_out, out_p, labels_from)
    else:
        got = engine.Matrix.join([(s if isinstance(s, int) else _src(s)[1], r, b) for s, r, b in zip(names, rows, bases)], n_out, out_p, labels_from)
    assert got.p == out_p
    return got, model


def _check(names, rows, bases, out_p=None, labels_from=None, what=""):
    for device_form in (False, True):
        got, model = _join(names, rows, bases, out_p, labels_from, device_form)
        _same_matrix(got, model, (what, names, "device" if device_form else "host"))
        got.close()


def _disjoint(names):
    return jm.bases([_width(s) for s in names])[:-1].tolist()


def _ind_rows(rows, vocab, seed=8):
    """ids of an indicator block beside a row list: as many ids as output rows"""
    n_out = N if rows is None else len(rows)
    return np.random.default_rng(seed).integers(0, vocab, n_out)


# ------------------------------------------------------------------------------------------------------------------ 1. model equality
@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("variant", ["real_lab", "real_unl", "unit_lab", "unit_unl"])
def test_join_ragged_sources(variant, hook):
    """rows of 0 .. 1 025 entries with and without labels, real and unit values; every id list; disjoint ranges and one shared range (a column
    stored twice); labels from each block and from none"""
    a, b = "long:" + variant, "short:" + variant
    _limits(*HOOKS[hook])
    labelled = "unl" not in variant
    for lname, rows in _id_lists().items():
        other = None if rows is None else np.random.default_rng(4).integers(0, N, len(rows))
        for bases in (_disjoint([a, b]), [0, 0]):
            for labels_from in ((None, 0, 1) if labelled else (None,)):
                _check([a, b], [rows, other], bases, labels_from=labels_from, what=(lname, hook))


@pytest.mark.parametrize("hook", list(HOOKS))
def test_join_fixed_length_sources(hook):
    """every block of a fixed length: 16-byte reads where every length is a multiple of four (4, 8, 4 + 8), word reads and pieces that straddle
    blocks, rows and launches otherwise (1, 3, 6, 30, sums with an indicator's 1); limits of 4 and 8 move joins of 4 and 8 entries between forms"""
    _limits(*HOOKS[hook])
    lists = _id_lists()
    for rname in ("identity", "bootstrap", "three_n", "one", "empty"):
        rows = lists[rname]
        for L in (1, 3, 4, 6, 8, 30):
            _check([f"fixed{L}:real_lab"], [rows], [0], labels_from=0, what=(L, rname, hook))
        for names in (["fixed4:real_lab", "fixed8:unit_lab"], ["fixed3:real_lab", 11], ["fixed4:real_lab", "fixed3:real_lab", "fixed1:unit_lab"],
                      [11, "fixed6:unit_lab", 13], ["fixed4:real_lab", "fixed4:real_lab"], ["fixed30:real_lab", "fixed6:unit_lab"]):
            rr = [_ind_rows(rows, s, 8 + i) if isinstance(s, int) else (rows if i == 0 or rows is None else np.roll(rows, i)) for i, s in enumerate(names)]
            _check(names, rr, _disjoint(names), what=(rname, hook))


@pytest.mark.parametrize("hook", ["default", "at4", "at8", "flat", "launch16"])
@pytest.mark.parametrize("n_dense", [0, 2])
def test_join_field_layout_sources_and_indicator_positions(n_dense, hook):
    """synthetic_fields with and without a dense prefix, an indicator block first, in the middle and last"""
    f, s = f"fields:{n_dense}", "short:real_lab"
    _limits(*HOOKS[hook])
    rows = _id_lists()["bootstrap"]
    for names in ([f], [f, 23], [23, f], [f, 23, s], [23, s, f], [s, f, 23], [23, 17], [23]):
        rr = [_ind_rows(rows, x, 20 + i) if isinstance(x, int) else np.roll(rows, i) for i, x in enumerate(names)]
        _check(names, rr, _disjoint(names), what=(n_dense, hook))
        _check(names, rr, [0] * len(names), out_p=max(_width(x) for x in names), what=(n_dense, hook, "shared"))


@pytest.mark.parametrize("hook", ["default", "at8", "group", "flat"])
def test_join_of_sixteen_blocks(hook):
    names = ["short:real_lab", 9, "fixed3:real_lab", "tiny:real_lab", 5, "fields:0", "fixed8:unit_lab", "long:unit_unl"] * 2
    rng = np.random.default_rng(6)
    _limits(*HOOKS[hook])
    for n_out in (N, 3 * N, 1, 0):
        rows = [rng.integers(0, x if isinstance(x, int) else N, n_out) for x in names]
        _check(names, rows, _disjoint(names), labels_from=2, what=(n_out, hook))
    for count in (1, 2, 3):
        rows = [rng.integers(0, x if isinstance(x, int) else N, 2 * N) for x in names[:count]]
        _check(names[:count], rows, _disjoint(names[:count]), labels_from=0, what=(count, hook))


# ---------------------------------------------------------------------------------------------------- 2. every form gives the same bits
def test_every_form_and_a_second_call_give_the_same_bits():
    """one join through every hook setting, the host and the device form, twice: one set of bits (and the model's)"""
    rng = np.random.default_rng(7)
    for names in (["tiny:real_lab", 9, "fixed3:real_lab"], ["fixed4:real_lab", "fixed4:unit_lab"], ["fixed4:real_lab", "fixed3:real_lab", 9],
                  ["short:real_lab", "long:real_lab"]):
        rows = [rng.integers(0, x if isinstance(x, int) else N, 3 * N) for x in names]
        seen = []
        for hook in HOOKS:
            _limits(*HOOKS[hook])
            for device_form in (False, True, False):
                got, model = _join(names, rows, _disjoint(names), labels_from=0, device_form=device_form)
                _same_matrix(got, model, (names, hook, device_form))
                seen.append(tuple(a.tobytes() for a in got.export()))
                got.close()
        assert len(set(seen)) == 1


# ------------------------------------------------------------------------------------------------- 3. identities with what exists
@pytest.mark.parametrize("name", ["long:real_lab", "short:unit_unl", "fixed6:real_lab", "fields:2"])
def test_one_block_is_a_take_and_the_identity_is_the_source(name):
    from fmwr_amd import engine
    host, m = _src(name)
    labels_from = None if host[3] is None else 0
    for rows in _id_lists().values():
        if rows is None:
            continue
        got = engine.Matrix.join([(m, rows, 0)], labels_from=labels_from)
        ref = m.take(rows)
        _same_matrix(got, ref.export() if host[3] is not None else ref.export()[:3] + (None,), name)
        got.close(); ref.close()
    same = engine.Matrix.join([(m, None, 0)], labels_from=labels_from)
    _same_matrix(same, host, name)
    same.close()


def test_pair_rows_are_joins_of_their_context_and_item():
    """Matrix.pairs forms context(c) + item(i) and context(c) + item(j).  Contexts and items carry a unique id column as their first entry, so
    every pair row names its (c, i): the even rows equal the join at the parsed (c, i), the odd rows the join at (c, j)."""
    from fmwr_amd import engine
    rng = np.random.default_rng(12)
    nc, ni, p = 30, 50, 400

    def with_ids(n, first, seed):
        rp, col, val, _ = _csr(rng.integers(0, 7, n), p - 100, seed)
        lens = np.diff(rp) + 1
        orp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        ocol, oval = np.zeros(int(orp[-1]), np.uint32), np.zeros(int(orp[-1]), np.float32)
        ocol[orp[:-1]] = first + np.arange(n); oval[orp[:-1]] = 1.0
        rest = np.ones(len(ocol), bool); rest[orp[:-1]] = False
        ocol[rest] = col + 100; oval[rest] = val
        return orp, ocol, oval
    ctx, items = with_ids(nc, 0, 1), with_ids(ni, nc, 2)
    pos = sp.random(nc, ni, density=0.1, random_state=5, format="csr")
    mc, mi = engine.Matrix.from_csr(*ctx, p), engine.Matrix.from_csr(*items, p)
    mp = engine.Matrix.from_csr(pos.indptr, pos.indices, np.ones(pos.nnz), ni)
    pairs = engine.Matrix.pairs(mc, mi, mp, n_neg=2, seed=3)
    host = pairs.export()
    assert pairs.n == 4 * pos.nnz and pairs.n > 0
    for parity in (0, 1):
        rp, col, val, _ = sm.take(host[0], host[1], host[2], None, np.arange(parity, pairs.n, 2))
        c = col[rp[:-1]].astype(np.int64)
        i = col[rp[:-1] + (ctx[0][c + 1] - ctx[0][c])].astype(np.int64) - nc
        assert np.all((c >= 0) & (c < nc) & (i >= 0) & (i < ni))
        if parity == 0:
            assert all(pos[cc, ii] != 0 for cc, ii in zip(c, i))
        got = engine.Matrix.join([(mc, c, 0), (mi, i, 0)], p=p)
        _same_matrix(got, (rp, col, val, None), parity)
        got.close()


def test_stack_of_takes_and_folds():
    """stack([m.take(a), m.take(b)]) is m.take(a ++ b); the k folds' selects stacked and taken by the inverse permutation give m back"""
    from fmwr_amd import engine
    for name in ("long:real_lab", "short:unit_unl", "fields:2", "fixed6:real_lab"):
        host, m = _src(name)
        full = host if host[3] is not None else host[:3] + (None,)
        lists = _id_lists()
        for a, b in (("bootstrap", "three_n"), ("empty", "one"), ("reverse", "empty"), ("empty", "empty")):
            parts = [m.take(lists[a]), m.take(lists[b])]
            got, ref = engine.Matrix.stack(parts), m.take(np.concatenate([lists[a], lists[b]]))
            _same_matrix(got, ref.export()[:3] + ((ref.export()[3],) if host[3] is not None else (None,)), (name, a, b))
            _same_matrix(got, jm.stack([sm.take(*full, lists[a]), sm.take(*full, lists[b])]), (name, a, b, "model"))
            if (a, b) == ("bootstrap", "three_n"):      # (a part of no rows carries no layout: the detector then reads the few rows there are)
                assert _flags(got) == _flags(ref), (name, a, b)
            for x in parts + [got, ref]:
                x.close()
        k = 5
        part = engine.split_assign(m.n, n_folds=k, seed=11)
        folds = [m.select(part, f, return_rows=True) for f in range(k)]
        order = np.concatenate([rows for _, rows in folds])
        inverse = np.empty(m.n, np.int64); inverse[order] = np.arange(m.n)
        whole = engine.Matrix.stack([f for f, _ in folds])
        back = whole.take(inverse)
        _same_matrix(back, full, (name, "folds"))
        for x in [f for f, _ in folds] + [whole, back]:
            x.close()
    one = engine.Matrix.stack([_src("long:real_lab")[1]])
    _same_matrix(one, _src("long:real_lab")[0], "one part")
    one.close()


# ---------------------------------------------------------------------------------------------------------------------------- 4. flags
def _fields_base(n_dense):
    return n_dense + np.concatenate([[0], np.cumsum(VOCAB)])


@pytest.mark.parametrize("case", ["indicators_and_fields", "dense_prefix_first"])
def test_a_join_that_qualifies_carries_the_concatenated_layout(case):
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(14)
    n_out = 384
    if case == "indicators_and_fields":
        names, n_dense = [60, 45, "fields:0"], 0
        cb = _disjoint(names)
        bases = [0, cb[1]] + (cb[2] + _fields_base(0)[:-1]).tolist()
    else:
        names, n_dense = ["fields:2", 45, "fields:0"], 2
        cb = _disjoint(names)
        bases = _fields_base(2)[:-1].tolist() + [cb[1]] + (cb[2] + _fields_base(0)[:-1]).tolist()
    rows = [rng.integers(0, x if isinstance(x, int) else N, n_out) for x in names]
    labels_from = 2
    got, model = _join(names, rows, cb, labels_from=labels_from)
    _same_matrix(got, model, case)
    out_p = got.p
    row_len = n_dense + len(bases)
    unit = int(all(isinstance(x, int) or _flags(_src(x)[1])["unit_values"] for x in names))
    assert unit == int(n_dense == 0)
    assert _flags(got) == dict(rows_sorted=1, unit_values=unit, fixed_row_len=row_len, max_row_len=row_len, fields=len(bases)), _flags(got)
    got.set_fields(n_dense, bases + [out_p])                 # the same layout, vouched for and checked on the device: accepted
    assert _flags(got)["fields"] == len(bases)
    # a stack of such joins carries the layout on; five mini-batch steps leave the bits of five steps on the uploaded copy
    fresh, _ = _join(names, rows, cb, labels_from=labels_from)
    twice = engine.Matrix.stack([fresh, fresh])
    assert _flags(twice) == _flags(fresh)
    twice.close()
    rp, col, val, y = model
    copy = engine.Matrix.from_csr(rp, col, val, out_p, y)
    params = []
    for m in (fresh, copy):
        e = engine.Engine(out_p, mode=L.MODE_MINIBATCH, batch_rows=64, num_factor=4, task=L.TASK_REGRESSION, learn_rate=0.05)
        prng = np.random.default_rng(15)
        e.set_params(0.1, prng.normal(0, 0.1, out_p), prng.normal(0, 0.1, (4, out_p)))
        for batch in range(5):
            e.step(m, batch)
        w0, w, v = e.get_params()
        params.append(np.concatenate([[w0], w, v.ravel()]))
        e.close()
    assert np.array_equal(params[0].view(np.uint64), params[1].view(np.uint64))
    assert np.any(params[0][1:1 + out_p] != np.random.default_rng(15).normal(0, 0.1, out_p))
    for x in (got, fresh, copy):
        x.close()


@pytest.mark.parametrize("case", ["overlap", "ragged_block", "dense_prefix_in_block_1"])
def test_a_join_that_does_not_qualify_has_the_flags_of_an_upload(case):
    from fmwr_amd import engine
    rng = np.random.default_rng(16)
    names, bases = {"overlap": (["fields:0", "fields:0"], [0, 0]), "ragged_block": ([30, "tiny:real_lab", "fields:0"], None),
                    "dense_prefix_in_block_1": ([30, "fields:2"], None)}[case]
    bases = _disjoint(names) if bases is None else bases
    rows = [rng.integers(0, x if isinstance(x, int) else N, 2 * N) for x in names]
    got, model = _join(names, rows, bases)
    _same_matrix(got, model, case)
    copy = engine.Matrix.from_csr(model[0], model[1], model[2], got.p)
    assert _flags(got) == _flags(copy), (case, _flags(got), _flags(copy))
    got.close(); copy.close()


# ------------------------------------------------------------------------------------------------------------- 5. forward consistency
@pytest.mark.parametrize("kind", ["mb32", "mb64"])
@pytest.mark.parametrize("k", [0, 3, 16])
def test_predict_of_the_joined_cross_product_is_the_full_ranking(kind, k):
    """fmx_predict on the join of every (context, item) pair against fmx_topk's full ranking scores, within the bar tests/test_gpu_topk.py holds
    the same scores to against a host-built concatenation (its RTOL times the sum of the absolute terms)"""
    from fmwr_amd import _lib as L, engine
    from tests.test_gpu_topk import RTOL
    from tests.util import random_csr
    p, nc, ni = 80, 6, 41
    ctx, items = random_csr(nc, p, 6, 1), random_csr(ni, p, 4, 2)             # one id range: c (+) i may hold a feature twice
    mc, mi = engine.Matrix.from_csr(*ctx, p), engine.Matrix.from_csr(*items, p)
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=256, state_fp64=int(kind == "mb64"))
    rng = np.random.default_rng(k + 11)
    e.set_params(0.3, rng.normal(0, 0.5, p), rng.normal(0, 0.4, (k, p)))
    c, i = np.repeat(np.arange(nc), ni), np.tile(np.arange(ni), nc)
    cross = engine.Matrix.join([(mc, c, 0), (mi, i, 0)], p=p)
    _same_matrix(cross, jm.join([(ctx + (None,), c, 0), (items + (None,), i, 0)], nc * ni, p), "cross")
    pred = e.predict(cross).reshape(nc, ni)
    idx, score = e.topk(mc, mi, ni)
    w0, w, v = e.get_params()
    rp, col, val, _ = cross.export()
    A = sp.csr_matrix((np.abs(val).astype(np.float64), col, rp), shape=(nc * ni, p))
    scale = (abs(w0) + A @ np.abs(w) + 0.5 * ((A @ np.abs(v).T) ** 2).sum(1) + 1e-300).reshape(nc, ni)
    for r in range(nc):
        assert sorted(idx[r]) == list(range(ni))
        assert np.all(np.abs(score[r] - pred[r, idx[r]]) <= RTOL[kind] * scale[r, idx[r]]), (kind, k, r)
    for x in (cross, mc, mi):
        x.close()
    e.close()


# ------------------------------------------------------------------------------------------------------------------------ 6. refusals
def _raw_join(call, specs, n_out, out_p, labels_from=-1, device=0):
    from fmwr_amd import _lib as L
    arr = (L.JoinBlock * len(specs))()
    for b, (m, rows, n_ids, base) in enumerate(specs):
        arr[b].m = None if m is None else (m.h.value if isinstance(m.h, C.c_void_p) else m.h)
        arr[b].rows, arr[b].n_ids, arr[b].col_base = rows, n_ids, base
    h = C.c_void_p(5)
    status = call(device, arr, len(specs), n_out, out_p, labels_from, C.byref(h))
    return status, h.value, L.lib().fmx_last_error().decode()


def test_refusals_leave_the_output_null_and_the_sources_usable():
    from fmwr_amd import _lib as L, engine
    lib = L.lib()
    (host, m), (host_u, unl) = _src("long:real_lab"), _src("short:real_unl")
    rng = np.random.default_rng(18)
    n_out = 3 * N
    ra, ri = rng.integers(0, N, n_out), rng.integers(0, 23, n_out)
    for t_bad, b_bad, also in ((50, 0, None), (30, 1, (50, 0)), (7, 0, (7, 1)), (0, 1, None), (n_out - 1, 0, None)):
        bad = [ra.copy(), ri.copy()]
        for t, b in [(t_bad, b_bad)] + ([also] if also else []):
            bad[b][t] = [N, 23][b] if t % 2 else -1
        keep = [DevBuf.from_numpy(x) for x in bad]
        for call, ptrs in ((lib.fmx_matrix_join, [x.ctypes.data for x in bad]), (lib.fmx_matrix_join_device, [k.ptr.value for k in keep])):
            status, out, msg = _raw_join(call, [(m, ptrs[0], 0, 0), (None, ptrs[1], 23, m.p)], n_out, m.p + 23, 0)
            assert status == L.ERR_INVALID and not out and f"rows[{t_bad}] of block {b_bad}" in msg, msg
    pa, pi = ra.ctypes.data, ri.ctypes.data
    for call in (lib.fmx_matrix_join, lib.fmx_matrix_join_device):     # (refused before any launch: the lists are never read)
        status, out, msg = _raw_join(call, [(m, pa, 0, 0), (None, pi, 23, m.p)], n_out, m.p + 22)           # col_base + n_ids over out_p
        assert status == L.ERR_INVALID and not out and "exceed out_p" in msg
        status, out, msg = _raw_join(call, [(m, pa, 0, 2**32 - 1), (None, pi, 23, 0)], n_out, 2**32 - 1)  # in 64 bits
        assert status == L.ERR_INVALID and not out and "exceed out_p" in msg
        status, out, msg = _raw_join(call, [(m, pa, 0, 0)], n_out, m.p, device=1)                           # a source on another device
        assert status == L.ERR_INVALID and not out and "on device 0" in msg
        status, out, msg = _raw_join(call, [(m, None, 0, 0)], n_out, m.p)                                   # an identity block of another row count
        assert status == L.ERR_INVALID and not out and "no row list" in msg
        status, out, msg = _raw_join(call, [(m, pa, 0, 0), (unl, pa, 0, 0)], n_out, m.p, 1)                 # labels from a source without labels
        assert status == L.ERR_INVALID and not out and "has no labels" in msg
    parts = (C.c_void_p * 2)(m.h.value if isinstance(m.h, C.c_void_p) else m.h, unl.h.value if isinstance(unl.h, C.c_void_p) else unl.h)
    h = C.c_void_p(5)
    assert lib.fmx_matrix_stack(parts, 2, C.byref(h)) == L.ERR_INVALID and not h.value                      # mixed labels
    assert "all of them or none" in lib.fmx_last_error().decode()
    other_p = engine.Matrix.from_csr(np.zeros(2, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), 7, np.zeros(1, np.float32))
    with pytest.raises(L.FmxError, match="features"):
        engine.Matrix.stack([m, other_p])
    # the sources are as they were
    _same_matrix(m, host, "source after the refusals")
    _same_matrix(unl, host_u, "source after the refusals")
    good = engine.Matrix.join([(m, ra, 0), (23, ri, m.p)], labels_from=0)
    _same_matrix(good, jm.join([(host, ra, 0), (23, ri, m.p)], n_out, m.p + 23, 0), "after the refusals")
    good.close()


# ---------------------------------------------------------------------------------------------------------------------- 7. end to end
def _planted(seed=21, n_users=400, n_items=120, n=6000):
    """the label depends on one user-side and one item-side feature only: the user's segment (8 of them) and the item's category (6)"""
    rng = np.random.default_rng(seed)
    seg, cat = rng.integers(0, 8, n_users), rng.integers(0, 6, n_items)
    a, b = rng.normal(0, 2.0, 8), rng.normal(0, 0.7, 6)
    user, item = rng.integers(0, n_users, n), rng.integers(0, n_items, n)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-(a[seg[user]] + b[cat[item]])))).astype(np.float64)
    U = sp.csr_matrix((np.ones(n_users), (np.arange(n_users), seg)), shape=(n_users, 8))
    I = sp.csr_matrix((np.ones(n_items), (np.arange(n_items), cat)), shape=(n_items, 6))
    return user, item, y, U, I


def test_side_features_beat_ids_on_cold_users_and_recommend_scores_the_design():
    """fm_design -> fm_split (whole users held out: every test user is cold) -> fm_train -> fm_metrics.  The ids-only design knows nothing of a
    cold user; the design with side features knows the user's segment.  Over five seeds the two AUC ranges must not overlap."""
    import fmwr_amd as fm
    from tests.test_gpu_topk import RTOL
    user, item, y, U, I = _planted()
    n_users, n_items = U.shape[0], I.shape[0]
    ctl = [fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=12000, solver=fm.SGD_solver())]
    side = fm.fm_design(user, item, y, fm.fm_matrix(U), fm.fm_matrix(I))
    plain = fm.fm_design(user, item, y, n_users=n_users, n_items=n_items)
    assert side["data"].dim == (len(user), n_users + n_items + 14) and plain["data"].dim == (len(user), n_users + n_items)
    assert side["bases"].tolist() == [0, n_users, n_users + n_items, n_users + n_items + 8]
    assert side["context"].dim == (n_users, side["data"].dim[1]) and side["items"].dim == (n_items, side["data"].dim[1])
    # the design is the model's join
    hostU = (U.indptr.astype(np.int64), U.indices.astype(np.uint32), U.data.astype(np.float32), None)
    hostI = (I.indptr.astype(np.int64), I.indices.astype(np.uint32), I.data.astype(np.float32), None)
    ref = jm.join([(n_users, user, 0), (n_items, item, n_users), (hostU, user, n_users + n_items), (hostI, item, n_users + n_items + 8)], len(user),
                  n_users + n_items + 14)
    f = side["data"].features
    assert np.array_equal(f["col_idx"], ref[1].astype(np.int32)) and np.array_equal(np.concatenate([[0], np.cumsum(f["row_size"])]), ref[0])
    assert np.all(f["value"] == 1.0) and np.array_equal(side["data"].labels, y)
    aucs = {"side": [], "ids": []}
    fit = None
    for name, design in (("side", side), ("ids", plain)):
        train, test, mask = fm.fm_split(design["data"], test_fraction=0.25, by=user, how="groups", seed=3)
        assert not set(user[mask]) & set(user[~mask])                         # every test user is cold
        for seed in (1, 2, 3, 4, 5):
            model = fm.fm_train(train, normalize=False, seed=seed, control=ctl)
            aucs[name].append(fm.fm_metrics(model, test, normalize=False)["pooled"]["auc"])
            if name == "side" and seed == 1:
                fit = model
    print(f"AUC on cold users: side features {min(aucs['side']):.4f} .. {max(aucs['side']):.4f}, ids only {min(aucs['ids']):.4f} .. {max(aucs['ids']):.4f}")
    assert min(aucs["side"]) > max(aucs["ids"]), aucs
    # fm_recommend(fit, context, items) scores (u, i) as predict scores data's row for (u, i)
    rec = fm.fm_recommend(fit, side["context"], side["items"], top_k=n_items, normalize=False)
    pred = fm.predict(fit, side["data"], normalize=False)
    where = np.empty((n_users, n_items), np.int64)
    where[np.arange(n_users)[:, None], rec["index"]] = np.arange(n_items)[None, :]
    got = rec["score"][user, where[user, item]]
    w0, w, v = fit["Model"]["w0"], np.asarray(fit["Model"]["w"]), np.asarray(fit["Model"]["v"])
    A = sp.csr_matrix((np.ones(len(ref[1])), ref[1], ref[0]), shape=(len(user), len(w)))
    scale = abs(w0) + A @ np.abs(w) + 0.5 * ((A @ np.abs(v.reshape(-1, len(w))).T) ** 2).sum(1) + 1e-300
    assert np.all(np.abs(got - pred) <= RTOL["seq64"] * scale)
    # fm_stack puts the split back together
    train, test, mask = fm.fm_split(side["data"], test_fraction=0.25, seed=5)
    whole = fm.fm_stack([train, test])
    order = np.concatenate([np.flatnonzero(~mask), np.flatnonzero(mask)])
    assert whole.dim == side["data"].dim and np.array_equal(whole.labels, y[order])
    assert np.array_equal(whole.features["row_size"], f["row_size"][order]) and whole.features["size"] == f["size"]
