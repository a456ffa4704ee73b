"""The flags and the field layout of an fmx_matrix (fmx_debug_matrix_flags, fmx_debug_matrix_layout) against tests/flags_model.py, which restates
them from the exported rows.  Part 1: the detector (fm_ingest.hip: entries_scan_k, rows_scan_k, positions_scan_k, detect_fields) must find exactly
`truth` on the case table of tests/flags_cases.py, whose cases sit on the seams of its decomposition.  Part 2: every producer's flags must be `sound`
(no claim the rows contradict), and equal to `truth` where the producer goes through the detector.  Every comparison is exact equality.
FMX_UNIT_VALUES and FMX_DETECT_FIELDS stay unset: both are read once per process."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import flags_cases as fc
from tests import flags_model as fm

pytestmark = pytest.mark.gpu

VOCAB = [50, 40, 30, 7]
_truth = {}


def state(m):
    """(flags, layout) as the library holds them"""
    from fmwr_amd import _lib as L
    out = np.zeros(5, np.int32)
    L.check(L.lib().fmx_debug_matrix_flags(m.h, out.ctypes.data_as(C.c_void_p)))
    d, nf = C.c_int32(-1), C.c_int32(-1)
    base = np.full(fm.MAX_FIELDS + 1, 0xFFFFFFFF, np.uint32)
    L.check(L.lib().fmx_debug_matrix_layout(m.h, C.byref(d), C.byref(nf), base.ctypes.data_as(C.c_void_p)))
    assert nf.value == int(out[4]) and 0 <= nf.value <= fm.MAX_FIELDS
    assert not base[nf.value + 1 if nf.value else 0:].any()
    flags = dict(rows_sorted=int(out[0]), unit_values=int(out[1]), fixed_row_len=int(out[2]), max_row_len=int(out[3]))
    return flags, dict(dense_prefix=d.value, field_base=[int(b) for b in base[:nf.value + 1]] if nf.value else [])


def host_of(m):
    rp, col, val, _ = m.export()
    return rp, col, val, m.p


def upload(c):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(c["rp"], c["col"], c["val"], c["p"])


def truth_of(name):
    if name not in _truth:
        c = fc.build(name)
        _truth[name] = fm.truth(c["rp"], c["col"], c["val"], c["p"])
    return _truth[name]


def assert_exact(m, what=""):
    got, want = state(m), fm.truth(*host_of(m))
    assert got == want, (what, got, want)


def assert_sound(m, what=""):
    flags, layout = state(m)
    assert fm.sound(flags, layout, *host_of(m)) == [], (what, flags, layout)
    return flags, layout


# ================================================================================================================ 1. the detector, exactly
DETECTOR = [n for s in ("in_row", "seam", "many", "wrap", "value", "lengths", "fields") for n in fc.NAMES[s]]


@pytest.mark.parametrize("name", DETECTOR)
def test_the_detector_finds_the_truth(name):
    from fmwr_amd import _lib as L
    c = fc.build(name)
    try:
        m = upload(c)
    except L.FmxError:
        assert name == "many_seams(no_rows)"       # (a matrix of no rows may be refused; if it is taken its flags are checked like any other's)
        return
    try:
        assert state(m) == truth_of(name), (name, state(m), truth_of(name))
        if "expect" in c:                          # what the case plants, said once more without the model: only this differs from its clean twin
            t = upload(c["twin"])
            assert state(m)[0] == dict(state(t)[0], **c["expect"]), name
            t.close()
    finally:
        m.close()


def test_the_other_hand_overs_reach_the_same_detector():
    """fm.matrix's list layout and a dgCMatrix's slots: the same rows, the same flags and layout as from_csr"""
    from fmwr_amd import engine
    for name in ("in_row(4095,descent)", "odd_value(4096,up)", "fields_case(clean_z39_d3)", "fields_case(meet)", "one_row_differs(256,empty)"):
        c = fc.build(name)
        m = engine.Matrix.from_rlist(c["val"].astype(np.float64), c["col"].astype(np.int32), np.diff(c["rp"]).astype(np.int32), c["p"])
        assert state(m) == truth_of(name), ("rlist", name)
        m.close()
    for name in ("fields_case(clean_z39_d3)", "fields_case(meet)", "odd_value(4096,up)", "many_seams(every_row)"):   # (a transposition cannot hand over unsorted rows)
        c = fc.build(name)
        n = len(c["rp"]) - 1
        csc = sp.csr_matrix((np.arange(1, len(c["col"]) + 1, dtype=np.float64), c["col"].astype(np.int64), c["rp"]), shape=(n, c["p"])).tocsc()
        csc.sort_indices()
        x = c["val"].astype(np.float64)[csc.data.astype(np.int64) - 1]           # (the entry's number rides through the transposition: explicit zeros survive)
        m = engine.Matrix.from_dgc(x, csc.indices, csc.indptr, n, c["p"])
        rp, col, val, _ = m.export()
        assert np.array_equal(rp, c["rp"]) and np.array_equal(col, c["col"]) and np.array_equal(val.view(np.uint32), c["val"].view(np.uint32))
        assert state(m) == truth_of(name), ("dgc", name)
        m.close()


@pytest.mark.parametrize("name", fc.NAMES["set_fields"])
def test_set_fields_takes_what_holds_every_row_and_refuses_what_one_row_violates(name):
    from fmwr_amd import _lib as L
    c = fc.build(name)
    m = upload(c)
    flags, layout = truth_of(name)
    assert state(m) == (flags, layout)
    bad = list(layout["field_base"]); bad[2] += 1              # row c["row"] alone holds the id below it
    for refused in (bad, layout["field_base"][:-1] + [c["p"] + 1], [0] + layout["field_base"][1:]):
        with pytest.raises(L.FmxError):
            m.set_fields(1, refused)
        assert state(m) == (flags, layout)                     # a refusal leaves everything as it was
    with pytest.raises(L.FmxError):
        m.set_fields(2, [2] + layout["field_base"][2:])        # one more dense column than the rows have
    assert state(m) == (flags, layout)
    m.set_fields(1, layout["field_base"])                      # the detector's own bases
    assert state(m) == (flags, layout)
    wide = c["vocab_base"]                                     # the vocabularies: wider, and they hold every row
    m.set_fields(1, wide)
    assert state(m) == (flags, dict(dense_prefix=1, field_base=wide))
    assert fm.sound(*state(m), *host_of(m)) == []
    m.close()


# ================================================================================================================ 2. every producer's flags
def _fields(n_dense, n=512, seed=9):
    from fmwr_amd import engine
    return engine.Matrix.synthetic_fields(n, n_dense, VOCAB, 1.1, seed)


def _ragged_upload(unit, n=300, p=400, seed=4, labels=True):
    from fmwr_amd import engine
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 12, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(p, int(k), replace=False)) for k in lens]).astype(np.uint32)
    val = np.ones(len(col), np.float32) if unit else rng.normal(0, 1, len(col)).astype(np.float32)
    return engine.Matrix.from_csr(rp, col, val, p, rng.normal(0, 1, n).astype(np.float32) if labels else None)


GENERATORS = ["synthetic", "iid_uniform", "iid_zipf", "ragged", "fields_d0", "fields_d2", "source", "source_fields"]


def _generated(kind):
    """(matrix, what must be closed after it)"""
    from fmwr_amd import _lib as L, engine
    if kind == "synthetic":
        return engine.Matrix.synthetic(2048, 2000, 12, 5), None
    if kind.startswith("iid"):
        return engine.Matrix.synthetic_iid(2000, 600, 8, 7, law=L.COLUMNS_ZIPF if kind == "iid_zipf" else L.COLUMNS_UNIFORM), None
    if kind == "ragged":
        return engine.Matrix.synthetic_ragged(2000, 600, 6.0, 3, min_nnz=1, max_nnz=20), None
    if kind.startswith("fields"):
        return _fields(int(kind[-1])), None
    kw = dict(task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=4, mode=L.MODE_MINIBATCH, batch_rows=512)
    if kind == "source":
        e = engine.Engine(3000, **kw)
        src = e.source(1024, nnz_per_row=6, seed=3)
    else:
        e = engine.Engine(2 + sum(VOCAB), **kw)
        src = e.source(1024, seed=3, fields=(2, VOCAB, 1.1))
    return src.next(), e


@pytest.mark.parametrize("kind", GENERATORS)
def test_generated_matrices_claim_nothing_false(kind):
    m, owner = _generated(kind)
    flags, layout = assert_sound(m, kind)
    assert flags["rows_sorted"] == 1               # (what the generators are for: the claim is made, and it is true)
    if "fields" in kind:
        d = 2 if kind.endswith("d2") or kind == "source_fields" else 0
        assert layout == dict(dense_prefix=d, field_base=(d + np.concatenate([[0], np.cumsum(VOCAB)])).tolist())
    if owner is not None:
        owner.close()
    else:
        m.close()


def _take_lists(n):
    rng = np.random.default_rng(3)
    return {"identity": np.arange(n), "bootstrap": rng.integers(0, n, n), "one": np.array([n // 2]), "empty": np.zeros(0, np.int64)}


@pytest.mark.parametrize("rows", ["identity", "bootstrap", "one", "empty"])
@pytest.mark.parametrize("source", ["fields_d2", "ragged", "upload_real", "upload_unit"])
def test_take_and_select_claim_nothing_false(source, rows):
    from fmwr_amd import engine
    m = _generated(source)[0] if not source.startswith("upload") else _ragged_upload(source.endswith("unit"))
    t = m.take(_take_lists(m.n)[rows])
    flags, layout = assert_sound(t, (source, rows))
    if rows == "identity":
        assert (flags["rows_sorted"], flags["unit_values"]) == (state(m)[0]["rows_sorted"], state(m)[0]["unit_values"])
    part = engine.split_assign(m.n, n_folds=3, seed=11)
    for which, complement in ((0, False), (1, True), (7, False)):     # (part 7 does not occur: no rows)
        s = m.select(part, which, complement=complement)
        assert_sound(s, (source, "select", which, complement))
        s.close()
    t.close(); m.close()


@pytest.mark.parametrize("source", ["fields_d0", "upload_real", "upload_unit"])
def test_split_entries_outputs_are_exact(source):
    from fmwr_amd import _lib as L
    m = _generated(source)[0] if not source.startswith("upload") else _ragged_upload(source.endswith("unit"))
    for order in (L.SPLIT_ORDER_HASH, L.SPLIT_ORDER_TAIL):
        kept, held = m.split_entries(hold=1, order=order, seed=8)
        assert_exact(kept, (source, "kept")); assert_exact(held, (source, "held"))
        kept.close(); held.close()
    m.close()


def _qualifying_join(n_out=384):
    from fmwr_amd import engine
    rng = np.random.default_rng(14)
    f2, f0 = _fields(2, n=40), _fields(0, n=40, seed=10)
    blocks = [(f2, rng.integers(0, 40, n_out), 0), (45, rng.integers(0, 45, n_out), f2.p), (f0, rng.integers(0, 40, n_out), f2.p + 45)]
    return engine.Matrix.join(blocks), (f2, f0)


def test_a_join_that_carries_the_layout_on_claims_nothing_false():
    j, keep = _qualifying_join()
    flags, layout = assert_sound(j, "join_layout")
    fb = 2 + np.concatenate([[0], np.cumsum(VOCAB)])
    want = fb[:-1].tolist() + [int(fb[-1])] + (int(fb[-1]) + 45 + np.concatenate([[0], np.cumsum(VOCAB)])).tolist()
    assert layout == dict(dense_prefix=2, field_base=want) and flags["fixed_row_len"] == 2 + 4 + 1 + 4      # the layout IS claimed, block after block
    j.close()
    for x in keep:
        x.close()


@pytest.mark.parametrize("case", ["overlap", "ragged_block", "dense_prefix_in_block_1"])
def test_a_join_that_does_not_qualify_is_exact(case):
    from fmwr_amd import engine
    rng = np.random.default_rng(16)
    f0, f2, tiny = _fields(0, n=40), _fields(2, n=40), _ragged_upload(False, n=40, p=300)
    n_out = 80
    rows = lambda n: rng.integers(0, n, n_out)
    blocks = {"overlap": [(f0, rows(40), 0), (f0, rows(40), 0)],
              "ragged_block": [(30, rows(30), 0), (tiny, rows(40), 30), (f0, rows(40), 30 + tiny.p)],
              "dense_prefix_in_block_1": [(30, rows(30), 0), (f2, rows(40), 30)]}[case]
    j = engine.Matrix.join(blocks)
    assert_exact(j, case)
    for x in (j, f0, f2, tiny):
        x.close()


@pytest.mark.parametrize("case", ["one_layout", "two_row_lengths", "an_empty_part"])
def test_stacked_parts_claim_nothing_false(case):
    from fmwr_amd import engine
    a, _ = _qualifying_join(100)
    if case == "one_layout":
        parts = [a, _qualifying_join(60)[0]]
    elif case == "two_row_lengths":
        parts = [fc_upload("all_rows(2)"), fc_upload("all_rows(30)")]
    else:
        parts = [a, a.take(np.zeros(0, np.int64)), a.take(np.arange(50))]
    s = engine.Matrix.stack(parts)
    flags, layout = assert_sound(s, case)
    if case == "one_layout":
        assert (flags, layout) == state(a)
    if case == "two_row_lengths":
        assert flags["fixed_row_len"] == 0 and flags["max_row_len"] >= 30
    for x in parts + [s, a]:
        x.close()


def fc_upload(name):
    return upload(fc.build(name))


@pytest.mark.parametrize("combine", ["KEEP", "SUM", "FIRST"])
@pytest.mark.parametrize("source", ["fields_d2", "upload_real", "upload_unit"])
def test_remapped_columns_are_exact(source, combine):
    from fmwr_amd import _lib as L
    m = _generated(source)[0] if not source.startswith("upload") else _ragged_upload(source.endswith("unit"))
    rng = np.random.default_rng(6)
    maps = {"identity": (np.arange(m.p), m.p), "reversed": (np.arange(m.p)[::-1].copy(), m.p),
            "folded": (np.where(rng.random(m.p) < 0.1, L.COLUMN_DROP, rng.integers(0, 37, m.p)), 37)}
    for what, (cmap, new_p) in maps.items():
        o = m.remap_columns(cmap, new_p, getattr(L, "COMBINE_" + combine))
        assert_exact(o, (source, combine, what))
        o.close()
    m.close()


def test_binned_columns_are_exact():
    m = _fields(2)
    rp, col, val, _ = m.export()
    for cols, edges in (([0, 1], [[-0.5, 0.5], [0.0]]), ([1], [[0.25]])):
        o, base = m.bin_columns(cols, edges)
        assert_exact(o, ("bins", cols))
        if len(cols) == 2:       # both dense columns are one-hot now: the rows are a one-hot layout, and the detector must say so
            flags, layout = state(o)
            assert flags["unit_values"] == 1 and layout["dense_prefix"] == 0 and len(layout["field_base"]) - 1 == 6
        o.close()
    m.close()


def test_pair_matrices_are_exact():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(12)
    nc, ni, p = 30, 50, 400

    def with_ids(n, first):
        lens = rng.integers(0, 7, n)
        rows = [[first + r] + (100 + np.sort(rng.choice(p - 100, int(k), replace=False))).tolist() for r, k in enumerate(lens)]
        rp = np.concatenate([[0], np.cumsum(lens + 1)]).astype(np.int64)
        col = np.concatenate(rows).astype(np.uint32)
        val = rng.normal(0, 1, len(col)).astype(np.float32); val[rp[:-1]] = 1.0
        return engine.Matrix.from_csr(rp, col, val, p)
    mc, mi = with_ids(nc, 0), with_ids(ni, nc)
    pos = sp.random(nc, ni, density=0.1, random_state=5, format="csr")
    mp = engine.Matrix.from_csr(pos.indptr, pos.indices, np.ones(pos.nnz, np.float32), ni)
    pairs = engine.Matrix.pairs(mc, mi, mp, n_neg=2, seed=3)
    assert pairs.n == 4 * pos.nnz > 0
    assert_exact(pairs, "pairs")
    assert state(pairs)[0]["rows_sorted"] == 0       # (context ids 100.. come before the item's id: the concatenated rows do not ascend, and the flag says so)
    e = engine.Engine(p, task=L.TASK_RANKING, solver=L.SOLVER_SGD, num_factor=4, mode=L.MODE_MINIBATCH, batch_rows=64)
    e.set_params(0.7, rng.normal(0, 0.5, p), rng.normal(0, 0.4, (4, p)))
    hard = engine.Matrix.pairs_hard(e, mc, mi, mp, n_neg=2, n_cand=8, seed=3)
    assert_exact(hard, "pairs_hard")
    for x in (pairs, hard, mc, mi, mp):
        x.close()
    e.close()


@pytest.mark.parametrize("source", ["fields_d0", "iid_uniform", "upload_unit"])
def test_synthetic_values_leave_exact_flags(source):
    m = _generated(source)[0] if not source.startswith("upload") else _ragged_upload(True)
    assert state(m)[0]["unit_values"] == 1
    m.synthetic_values(5)
    assert_exact(m, source)
    assert state(m)[0]["unit_values"] == 0 and state(m)[1] == fm.no_layout()
    m.close()


@pytest.mark.parametrize("source", ["fields_d2", "upload_real"])
def test_scales_then_normalize_leave_exact_flags(source):
    m = _generated(source)[0] if not source.startswith("upload") else _ragged_upload(False)
    mean, std = m.scales(np.arange(m.p))
    assert_exact(m, (source, "scales"))
    rng = np.random.default_rng(1)
    m.normalize(rng.normal(0, 1, m.p), np.where(rng.random(m.p) < 0.1, 0.0, rng.uniform(0.5, 2, m.p)))
    assert_exact(m, (source, "normalize"))
    m.close()


@pytest.mark.parametrize("kind", ["fields", "ragged"])
def test_all_twos_normalized_by_two_become_one_hot(kind):
    c = fc.all_twos(kind)
    m = upload(c)
    assert state(m) == fm.truth(c["rp"], c["col"], c["val"], c["p"]) and state(m)[0]["unit_values"] == 0 and state(m)[1] == fm.no_layout()
    m.normalize(np.zeros(m.p), np.full(m.p, 2.0))
    rp, col, val, _ = m.export()
    assert np.all(val.view(np.uint32) == fm.ONE_BITS)
    assert_exact(m, kind)
    flags, layout = state(m)
    assert flags["unit_values"] == 1 and bool(layout["field_base"]) == (kind == "fields")        # the layout appears where the rows qualify
    m.close()
