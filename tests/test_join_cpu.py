"""CPU-side checks of matrix composition (fmx_matrix_join, fmx_matrix_stack; fmwr_amd.fm_design / fm_stack): the numpy model of the definition
(tests/join_model.py) against a brute-force loop in Python, the identity with the row selection's model, the declared surface, and the argument
checks, which run before any device.  The refusals that need a source matrix -- an identity block of another row count, labels_from naming a
source without labels -- need a device to make one: tests/test_gpu_join.py has them."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import join_model as jm
from tests import split_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fmx_matrix_join", "fmx_matrix_join_device", "fmx_matrix_stack")


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


def _source(rng, n, p, lo=0, hi=10, labels=True):
    lens = rng.integers(lo, hi, n)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = rng.integers(0, p, int(rp[-1])).astype(np.uint32)
    val = rng.normal(0, 1, int(rp[-1])).astype(np.float32)
    y = rng.normal(0, 1, n).astype(np.float32) if labels else None
    return rp, col, val, y


def _join_brute(blocks, n_out, labels_from):
    orp, ocol, oval, oy = [0], [], [], []
    for t in range(n_out):
        for src, rows, base in blocks:
            r = t if rows is None else int(rows[t])
            if isinstance(src, int):
                ocol.append(base + r); oval.append(np.float32(1.0))
            else:
                for e in range(int(src[0][r]), int(src[0][r + 1])):
                    ocol.append(int(src[1][e]) + base); oval.append(src[2][e])
        orp.append(len(ocol))
        if labels_from is not None:
            src, rows, _ = blocks[labels_from]
            oy.append(src[3][t if rows is None else int(rows[t])])
    return np.array(orp, np.int64), np.array(ocol, np.uint32), np.array(oval, np.float32), (np.array(oy, np.float32) if labels_from is not None else None)


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    assert (a[3] is None) == (b[3] is None)
    if a[3] is not None:
        assert np.array_equal(a[3].view(np.uint32), b[3].view(np.uint32))


def test_join_model_against_a_brute_force_loop():
    rng = np.random.default_rng(3)
    a, b = _source(rng, 40, 11), _source(rng, 200, 7)
    n_out = 200
    ra = rng.integers(0, 40, n_out)            # repeated ids
    ri = rng.integers(0, 23, n_out)
    assert len(np.unique(ra)) < n_out and (np.diff(a[0]) == 0).any() and np.diff(a[0]).max() == 9
    for bases, out_p in (((0, 11, 34), 41), ((0, 0, 0), 23), ((5, 0, 5), 28)):       # disjoint; all zero on a shared range; overlapping
        for labels_from in (None, 0, 2):
            blocks = [(a, ra, bases[0]), (23, ri, bases[1]), (b, None, bases[2])]
            got = jm.join(blocks, n_out, out_p, labels_from)
            _same(got, _join_brute(blocks, n_out, labels_from))
            assert int(got[1].max()) < out_p and got[0][-1] == len(got[1])
    # a column that two blocks both store appears twice; no rows is a valid matrix
    twice = jm.join([(a, ra, 0), (a, ra, 0)], n_out, 11)
    assert twice[0][-1] == 2 * np.diff(a[0])[ra].sum()
    empty = jm.join([(a, np.zeros(0, np.int64), 0), (5, np.zeros(0, np.int64), 11)], 0, 16, 0)
    assert empty[0].tolist() == [0] and len(empty[1]) == 0 and len(empty[3]) == 0
    # the lowest position, and at that position the lowest block
    bad_a, bad_i = ra.copy(), ri.copy()
    bad_a[[50, 120]] = [40, -1]; bad_i[[50, 30]] = [23, 99]
    with pytest.raises(ValueError, match=r"rows\[30\] of block 1"):
        jm.join([(a, bad_a, 0), (23, bad_i, 11)], n_out, 34)
    bad_i[30] = 0
    with pytest.raises(ValueError, match=r"rows\[50\] of block 0"):
        jm.join([(a, bad_a, 0), (23, bad_i, 11)], n_out, 34)
    with pytest.raises(ValueError):
        jm.join([(a, None, 0)], n_out, 11)             # the identity on a source of another row count
    with pytest.raises(ValueError):
        jm.join([(23, ri, 20)], n_out, 42)             # col_base + n_ids above out_p
    with pytest.raises(ValueError):
        jm.join([(a, ra, 0), (23, ri, 11)], n_out, 34, labels_from=1)
    assert jm.bases([11, 23, 7]).tolist() == [0, 11, 34, 41]


def test_stack_of_two_takes_is_the_take_of_the_two_lists():
    rng = np.random.default_rng(4)
    m = _source(rng, 60, 9)
    ia, ib = rng.integers(0, 60, 35), rng.integers(0, 60, 0)
    ic = rng.permutation(60)[:17]
    for lists in ((ia, ic), (ia, ib, ic), (ib, ib), (ic,)):
        parts = [sm.take(*m, rows) for rows in lists]
        _same(jm.stack(parts), sm.take(*m, np.concatenate(lists)))
    # one join block is a take
    _same(jm.join([(m, ia, 0)], len(ia), 9, 0), sm.take(*m, ia))
    unl = sm.take(m[0], m[1], m[2], None, ia)
    assert jm.stack([unl, unl])[3] is None
    with pytest.raises(ValueError):
        jm.stack([unl, sm.take(*m, ia)])


def test_join_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS
        assert hasattr(L.lib(), name)
    assert "fmx_debug_join_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_join_limits")
    assert "fmx_debug_join_limits" not in text   # the hook stays out of the public header
    assert re.search(r"#define\s+FMX_JOIN_MAX_BLOCKS\s+16\b", header) and L.JOIN_MAX_BLOCKS == jm.MAX_BLOCKS == 16
    assert L.STACK_MAX_PARTS == jm.MAX_PARTS == 1024
    fields = re.search(r"typedef struct fmx_join_block \{(.*?)\} fmx_join_block;", header, flags=re.S).group(1)
    declared = [re.sub(r"^.*[\s\*]", "", decl.strip()) for decl in fields.split(";") if decl.strip()]
    assert declared == [f[0] for f in L.JoinBlock._fields_]
    assert C.sizeof(L.JoinBlock) == 32
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 27" in design and "Not built" in design.split("## 27")[1]
    import fmwr_amd as fm
    from fmwr_amd import engine
    for f in (fm.fm_design, fm.fm_stack, engine.join_bases, fm.Matrix.join, fm.Matrix.join_device, fm.Matrix.stack):
        assert callable(f)
    assert engine.join_bases([11, 23, 7]).tolist() == jm.bases([11, 23, 7]).tolist()
    assert "fm_join.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES


def _blocks(L, specs):
    arr = (L.JoinBlock * max(len(specs), 1))()
    for b, (m, rows, n_ids, base) in enumerate(specs):
        arr[b].m, arr[b].rows, arr[b].n_ids, arr[b].col_base = m, rows, n_ids, base
    return arr


def test_refusals_come_before_any_device_and_leave_the_output_empty():
    L = _lib()
    lib = L.lib()
    ids = np.zeros(4, np.int64)
    pi = ids.ctypes.data
    good = [(None, pi, 5, 0), (None, pi, 5, 5)]
    cases = [
        (good, 0, 4, 10, -1), (good, -1, 4, 10, -1), (good * 9, 17, 4, 90, -1),      # n_blocks outside 1 .. 16
        (good, 2, -1, 10, -1),                                                         # a negative n_out
        ([(None, pi, -1, 0)], 1, 4, 10, -1),                                           # a negative n_ids
        ([(None, None, 5, 0)], 1, 4, 10, -1),                                          # the identity on an indicator block
        (good, 2, 4, 10, 2), (good, 2, 4, 10, -2),                                     # labels_from out of range
        (good, 2, 4, 10, 0), (good, 2, 4, 10, 1),                                      # ... naming an indicator block
        (good, 2, 4, 9, -1), ([(None, pi, 5, 2**32 - 1)], 1, 4, 2**32 - 1, -1),        # col_base + n_ids above out_p, in 64 bits
    ]
    for call in (lib.fmx_matrix_join, lib.fmx_matrix_join_device):
        for specs, nb, n_out, out_p, labels_from in cases:
            h = C.c_void_p(5)
            assert call(0, _blocks(L, specs), nb, n_out, out_p, labels_from, C.byref(h)) == L.ERR_INVALID, (nb, n_out, labels_from)
            assert not h.value and lib.fmx_last_error().decode()
        h = C.c_void_p(5)
        assert call(0, None, 2, 4, 10, -1, C.byref(h)) == L.ERR_INVALID and not h.value
        assert call(0, _blocks(L, good), 2, 4, 10, -1, None) == L.ERR_INVALID
    assert np.all(ids == 0)
    h = C.c_void_p(5)
    assert lib.fmx_matrix_stack(None, 1, C.byref(h)) == L.ERR_INVALID and not h.value
    one = (C.c_void_p * 2)(None, None)
    for n_parts in (0, -1, 1025):
        h = C.c_void_p(5)
        assert lib.fmx_matrix_stack(one, n_parts, C.byref(h)) == L.ERR_INVALID and not h.value
    h = C.c_void_p(5)
    assert lib.fmx_matrix_stack(one, 2, C.byref(h)) == L.ERR_INVALID and not h.value      # a NULL part
    assert lib.fmx_matrix_stack(one, 2, None) == L.ERR_INVALID
    assert lib.fmx_debug_join_limits(4, 8, 16) == L.OK and lib.fmx_debug_join_limits(0, 0, 0) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    monkeypatch.setattr(api, "_device_matrix", lambda *a, **k: pytest.fail("a device was touched"))
    for name in ("from_csr", "join", "stack"):
        monkeypatch.setattr(api.Matrix, name, classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    from fmwr_amd import engine
    U = fm.fm_matrix(np.random.default_rng(0).random((5, 3)))
    I = fm.fm_matrix(np.random.default_rng(1).random((4, 2)))
    user, item = np.array([0, 1, 4, 2]), np.array([3, 0, 1, 1])
    with pytest.raises(ValueError, match="one interaction per position"):
        fm.fm_design(user, item[:3])
    with pytest.raises(ValueError, match="one value per interaction"):
        fm.fm_design(user, item, labels=[1.0, 0.0])
    with pytest.raises(ValueError, match="negative id"):
        fm.fm_design(np.array([0, -1, 2, 3]), item)
    with pytest.raises(ValueError, match="negative id"):
        fm.fm_design(user, np.array([0, -1, 2, 3]))
    with pytest.raises(ValueError, match=r"outside 0\.\.3"):
        fm.fm_design(user, item, n_users=4)
    with pytest.raises(ValueError, match=r"outside 0\.\.2"):
        fm.fm_design(user, item, n_items=3)
    with pytest.raises(ValueError, match=r"outside 0\.\.3"):
        fm.fm_design(user, item, user_features=I)             # the side table fixes the vocabulary
    with pytest.raises(ValueError, match="one row per id"):
        fm.fm_design(user, item, user_features=U, n_users=6)
    with pytest.raises(ValueError, match="one row per id"):
        fm.fm_design(user, item, item_features=I, n_items=9)
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_design(user, item, user_features=np.ones((5, 3)))
    with pytest.raises(ValueError, match="integer array"):
        fm.fm_design(user.astype(float), item)
    with pytest.raises(ValueError, match="nothing to join"):
        fm.fm_design(user, item, ids=False)
    with pytest.raises(ValueError, match="must be an integer"):
        fm.fm_design(user, item, n_users=-1)
    with pytest.raises(TypeError, match="fm.matrix"):
        fm.fm_stack([U, np.ones((2, 3))])
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_stack([U, I])
    with pytest.raises(ValueError, match="all of them or none"):
        fm.fm_stack([U, fm.fm_matrix(np.ones((2, 3)), [1.0, 0.0])])
    with pytest.raises(ValueError, match="1 to 1024"):
        fm.fm_stack([])
    for blocks in ([], [(5, None, 0)], [(5, np.zeros(3), 0)], [(5, np.zeros(3, np.int64), -1)], [(U, np.zeros(3, np.int64), 0)],
                   [(5, np.zeros(3, np.int64), 0), (5, np.zeros(4, np.int64), 5)]):
        with pytest.raises(ValueError):
            engine.Matrix._join_blocks(blocks, None, None, None, False)
