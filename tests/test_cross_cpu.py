"""CPU-side checks of the feature-cross surface (fmx_matrix_cross; fmwr_amd.fm_cross_features / fm_apply_crosses / fm_cross_candidates): the numpy
model of the definition (tests/cross_model.py) against a plain Python triple loop, the consequences include/fmx.h states, the declared surface,
and the argument checks, which run before any device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cross_cases as cc
from tests import cross_model as cm
from tests.split_model import H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


def _same(got, ref, what):
    for g, r, part in zip(got, ref, ("row_ptr", "col", "val", "cross_base")):
        g, r = (cc.bits(g), cc.bits(r)) if part == "val" else (np.asarray(g), np.asarray(r))
        assert g.dtype == r.dtype and np.array_equal(g, r), (what, part)


# ---------------------------------------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize("keep", [True, False])
def test_model_against_a_python_triple_loop(keep):
    rp, col, val, _ = cc.small()
    assert len(rp) > 5 and np.diff(rp).max() == 17
    for seed, salt in ((0, 0), (2**63 + 5, 77)):
        got = cm.cross(rp, col, val, cc.RAGGED_P, cc.RAGGED_BASE, cc.RAGGED_TERMS, seed, salt, keep)
        _same(got, cm.cross_loops(rp, col, val, cc.RAGGED_P, cc.RAGGED_BASE, cc.RAGGED_TERMS, seed, salt, keep), (keep, seed))
    vrp, vcol, vval, _, vp = cc.values()
    _same(cm.cross(vrp, vcol, vval, vp, cc.VALUE_BASE, cc.VALUE_TERMS, 3, 0, keep),
          cm.cross_loops(vrp, vcol, vval, vp, cc.VALUE_BASE, cc.VALUE_TERMS, 3, 0, keep), ("values", keep))


def test_the_value_cases_hold_what_they_are_meant_to():
    """the products of tests/cross_cases.py round, overflow, land in and start from the subnormals, give -0 and NaN"""
    a = np.array([x for x, _ in cc.VALUE_PAIRS], np.float32)
    b = np.array([y for _, y in cc.VALUE_PAIRS], np.float32)
    got = cm.product_bits(a, b)
    with np.errstate(all="ignore"):
        exact = a.astype(np.float64) * b.astype(np.float64)                  # exact: 24 + 24 bits
        once = exact.astype(np.float32)                                      # one rounding
    ok = ~np.isnan(once)
    assert np.array_equal(got[ok], once.view(np.uint32)[ok]) and np.all(got[~ok] == cm.NAN_BITS)
    kinds = {"inexact": np.any(ok & np.isfinite(once) & (once.astype(np.float64) != exact)), "inf": np.any(np.isinf(once) & np.isfinite(a) & np.isfinite(b)),
             "subnormal out": np.any((got & 0x7F800000 == 0) & (got & 0x7FFFFF != 0)), "subnormal in": np.any((cc.bits(a) & 0x7F800000 == 0) & (cc.bits(a) & 0x7FFFFF != 0)),
             "-0": np.any(got == 0x80000000), "nan from inf * 0": cm.NAN_BITS in got[np.isinf(a) & (b == 0)], "payload": np.any(np.isnan(a) & (cc.bits(a) != cm.NAN_BITS))}
    assert all(kinds.values()), kinds


def test_exact_ids_decode_back_and_widths_add_up():
    rp, col, val, _ = cc.ragged()
    base = cc.RAGGED_BASE.astype(np.int64)
    terms = [(0, 1), (1, 3), (2, 2), (0, 2)]
    orp, ocol, oval, cb = cm.cross(rp, col, val, cc.RAGGED_P, base, terms, keep_source=True)
    width = [(base[a + 1] - base[a]) * (base[b + 1] - base[b]) for a, b in terms]
    assert cb.tolist() == [40] + (40 + np.cumsum(width)).tolist() and cb.dtype == np.uint32
    assert cm.cross(rp, col, val, cc.RAGGED_P, base, terms, keep_source=False)[3].tolist() == [0] + np.cumsum(width).tolist()
    seg = np.searchsorted(base, col.astype(np.int64), side="right") - 1
    for r in range(len(rp) - 1):
        s, c = seg[rp[r]:rp[r + 1]], col[rp[r]:rp[r + 1]].astype(np.int64)
        row = ocol[orp[r]:orp[r + 1]].astype(np.int64)
        assert np.array_equal(row[:len(c)], c)                               # the source row first
        at = len(c)
        for t, (a, b) in enumerate(terms):
            ea, eb = c[s == a] - base[a], c[s == b] - base[b]
            n = len(ea) * (len(ea) - 1) // 2 if a == b else len(ea) * len(eb)
            ids = row[at:at + n] - int(cb[t])
            at += n
            assert np.all((ids >= 0) & (ids < width[t]))
            u, v = ids // (base[b + 1] - base[b]), ids % (base[b + 1] - base[b])
            if a == b:
                want = [(min(ea[i], ea[j]), max(ea[i], ea[j])) for i in range(len(ea)) for j in range(i + 1, len(ea))]
            else:
                want = [(x, y) for x in ea for y in eb]
            assert list(zip(u.tolist(), v.tolist())) == [(int(x), int(y)) for x, y in want], (r, t)
        assert at == len(row)
    # segment_base followed by cross_base[1:] is a segment list of the output
    out_base = np.concatenate([base, cb[1:].astype(np.int64)])
    assert out_base[-1] == cb[-1] and np.all(np.diff(out_base) >= 0)


def test_a_self_cross_does_not_depend_on_the_storage_order():
    rp, col, val, _ = cc.ragged()
    rng = np.random.default_rng(1)
    terms = [(2, 2), (2, 2, 11), (0, 0)]
    ref = cm.cross(rp, col, val, cc.RAGGED_P, cc.RAGGED_BASE, terms, 4, 1, False)
    perm = np.concatenate([rp[r] + rng.permutation(int(rp[r + 1] - rp[r])) for r in range(len(rp) - 1)]).astype(np.int64)
    got = cm.cross(rp, col[perm], val[perm], cc.RAGGED_P, cc.RAGGED_BASE, terms, 4, 1, False)
    assert np.array_equal(got[0], ref[0])
    changed = False
    for r in range(len(rp) - 1):
        a, b = int(ref[0][r]), int(ref[0][r + 1])
        key = lambda o: sorted(zip(o[1][a:b].tolist(), cc.bits(o[2][a:b]).tolist()))
        assert key(got) == key(ref)                                          # the multiset of (id, value bits) of the row
        changed |= not np.array_equal(got[1][a:b], ref[1][a:b])
    assert changed


def test_hashed_ids_are_h_of_the_pair_on_the_terms_stream():
    rp, col, val, _ = cc.ragged()
    base = cc.RAGGED_BASE.astype(np.int64)
    terms = [(0, 1, 1000003), (1, 3, 7), (0, 1, 1000003)]
    seed, salt = 12345, 6
    orp, ocol, _, cb = cm.cross(rp, col, val, cc.RAGGED_P, base, terms, seed, salt, False)
    assert cb.tolist() == [0, 1000003, 1000010, 2000013]
    seg = np.searchsorted(base, col.astype(np.int64), side="right") - 1
    first, third = [], []
    for r in range(len(rp) - 1):
        s, c = seg[rp[r]:rp[r + 1]], col[rp[r]:rp[r + 1]].astype(np.int64)
        row = ocol[orp[r]:orp[r + 1]].astype(np.int64)
        at = 0
        for t, (a, b, nb) in enumerate(terms):
            want = []
            for x in c[s == a] - base[a]:
                for y in c[s == b] - base[b]:
                    h = int(H(seed, salt, np.array([(int(x) << 32) | int(y)], np.uint64), 128 + t)[0])
                    want.append(int(cb[t]) + ((h * nb) >> 64))
            assert row[at:at + len(want)].tolist() == want
            (first if t == 0 else third if t == 2 else []).extend(i - int(cb[t]) for i in want)
            at += len(want)
    assert len(first) > 100 and first != third                              # the same pair on another stream hashes elsewhere
    assert len(set(ocol[(ocol >= cb[1]) & (ocol < cb[2])].tolist())) <= 7    # seven buckets: collisions are certain
    assert cm.mulhi64(np.array([2**64 - 1, 2**63, 12345], np.uint64), 2**32 - 1).tolist() == [((2**64 - 1) * (2**32 - 1)) >> 64, (2**63 * (2**32 - 1)) >> 64, 0]


def test_model_refusals():
    rp, col, val, _ = cc.small()
    good = dict(rp=rp, col=col, val=val, p=cc.RAGGED_P, segment_base=cc.RAGGED_BASE, terms=[(0, 1)])
    for kw in (dict(segment_base=[1, 40]), dict(segment_base=[0, 39]), dict(segment_base=[0, 9, 5, 40]), dict(terms=[(1, 0)]), dict(terms=[(0, 6)]), dict(terms=[]),
               dict(terms=[(0, 1)] * 65), dict(terms=[(0, 1, 2**32 - 41)]), dict(terms=[(0, 1, 2**32 - 2)], keep_source=True)):
        with pytest.raises(ValueError):
            cm.cross(**dict(good, **kw))
    assert cm.cross(**dict(good, terms=[(0, 1, 2**32 - 2 - 40)]))[3].tolist() == [40, 2**32 - 2]


# ------------------------------------------------------------------------------------------------------------------- the declared surface
def test_cross_entry_point_is_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+fmx_matrix_cross\s*\(", header)
    assert "fmx_matrix_cross" in L.SYMBOLS and hasattr(L.lib(), "fmx_matrix_cross")
    assert "fmx_matrix_cross_device" not in text                             # there is no _device form
    assert "fmx_debug_cross_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_cross_limits")
    assert "fmx_debug_cross_limits" not in text                              # the hook stays out of the public header
    assert header.index("fmx_matrix_bin_columns") < header.index("fmx_matrix_cross")
    for name, struct in (("fmx_cross_term", L.CrossTerm), ("fmx_cross_spec", L.CrossSpec)):
        fields = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", header, flags=re.S).group(1)
        declared = []
        for decl in fields.split(";"):
            if decl.strip():
                declared += [re.sub(r"^.*[\s\*]", "", part.strip()) for part in decl.split(",")]
        assert declared == [f[0] for f in struct._fields_], name
    assert C.sizeof(L.CrossTerm) == 16 and C.sizeof(L.CrossSpec) == 56
    assert L.CROSS_MAX_SEGMENTS == cm.MAX_SEGMENTS == 4096 and L.CROSS_MAX_TERMS == cm.MAX_TERMS == 64 and L.CROSS_STREAM0 == cm.STREAM0 == 128
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 30" in design and "Not built" in design.split("## 30")[1]
    import fmwr_amd as fm
    for f in (fm.fm_cross_features, fm.fm_apply_crosses, fm.fm_cross_candidates, fm.Crossing, fm.Matrix.cross):
        assert callable(f)
    assert "fm_cross.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fm_cross.hip")).read()
    assert '#include "fm_prims.h"' in src and "rocprim" not in src and "pair_hash(" in src      # the scan and the hash are the shared ones


def _spec(L, keep, **kw):
    v = dict(n_segments=3, segment_base=np.array([0, 4, 4, 10], np.uint32), terms=[(0, 2, 0, 0), (2, 2, 5, 0)], keep_source=1, seed=1, salt=2, reserved=0)
    v.update(kw)
    terms = v["terms"]
    arr = None if terms is None else (L.CrossTerm * max(len(terms), 1))(*[L.CrossTerm(*t) for t in terms])
    base = v["segment_base"]
    keep.extend([arr, base])
    s = L.CrossSpec(C.sizeof(L.CrossSpec), v["n_segments"], None if base is None else base.ctypes.data, v.get("n_terms", 0 if terms is None else len(terms)),
                    v["keep_source"], None if arr is None else C.addressof(arr), v["seed"], v["salt"], v["reserved"])
    if "struct_size" in kw:
        s.struct_size = kw["struct_size"]
    return s


def test_refusals_come_before_any_device_and_write_nothing():
    """every refusal that can be seen without the matrix comes before the matrix is looked at: with a NULL matrix the message names the argument.
    None of them may touch a device: on a machine without one that would be FMX_ERR_NOGPU, not FMX_ERR_INVALID"""
    L = _lib()
    lib = L.lib()
    base = np.full(4, 7, np.uint32)
    pb = base.ctypes.data_as(C.c_void_p)
    keep = []
    u32 = lambda *a: np.array(a, np.uint32)

    def cross(m=None, spec="good", cross_base=pb, **kw):
        h = C.c_void_p(5)
        s = _spec(L, keep, **kw) if spec == "good" else spec
        st = lib.fmx_matrix_cross(m, None if s is None else C.byref(s), cross_base, C.byref(h))
        assert not h.value
        return st, lib.fmx_last_error().decode()
    many = np.arange(4098, dtype=np.uint32)
    for kw, word in ((dict(spec=None), "spec is NULL"), (dict(cross_base=None), "cross_base"), (dict(struct_size=52), "struct_size"), (dict(reserved=1), "spec.reserved"),
                     (dict(n_segments=0), "n_segments"), (dict(n_segments=4097, segment_base=many), "n_segments"), (dict(n_segments=-1), "n_segments"),
                     (dict(terms=[]), "n_terms"), (dict(terms=[(0, 1, 0, 0)] * 65), "n_terms"), (dict(n_terms=-1), "n_terms"), (dict(keep_source=2), "keep_source"),
                     (dict(segment_base=None), "segment_base is NULL"), (dict(terms=None, n_terms=1), "terms is NULL"),
                     (dict(segment_base=u32(1, 4, 4, 10)), "start at 0"), (dict(segment_base=u32(0, 5, 4, 10)), "descends"),
                     (dict(terms=[(0, 2, 0, 1)]), "reserved"), (dict(terms=[(2, 0, 0, 0)]), "seg_a"), (dict(terms=[(0, 3, 0, 0)]), "segment 3"),
                     (dict(terms=[(0, 0xFFFFFFFF, 0, 0)]), "segment"),
                     (dict(terms=[(0, 2, 2**32 - 1, 0)]), "2^32 - 2"), (dict(terms=[(0, 2, 2**31, 0), (2, 2, 2**31, 0)]), "2^32 - 2"),
                     (dict(segment_base=u32(0, 70000, 70000, 140000), terms=[(0, 2, 0, 0)]), "2^32 - 2"),       # 70 000 x 70 000 exact ids
                     (dict(), "NULL matrix"), (dict(terms=[(0, 2, 2**32 - 2, 0)]), "NULL matrix")):                  # the widest list that fits: the next check speaks
        st, msg = cross(**kw)
        assert st == L.ERR_INVALID and word in msg, (kw, msg)
    assert lib.fmx_matrix_cross(None, C.byref(_spec(L, keep)), pb, None) == L.ERR_INVALID
    assert np.all(base == 7)
    assert lib.fmx_debug_cross_limits(-1, 4, 16) == L.OK and lib.fmx_debug_cross_limits(0, -1, 0) == L.OK and lib.fmx_debug_cross_limits(0, 0, 0) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    for name in ("_device_matrix", "_engine_for"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api.Matrix, "from_csr", classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    d = fm.fm_matrix(np.random.default_rng(0).random((6, 4)), np.arange(6) % 2)
    fields = [0, 1, 2, 4]
    for f in (lambda x: fm.fm_cross_features(x, [(0, 1)], fields), lambda x: fm.fm_apply_crosses(x, None)):
        with pytest.raises(TypeError, match="fm.matrix"):
            f(np.ones((6, 4)))
    for bad in ([0, 1, 2, 3], [1, 2, 4], [0, 3, 2, 4], [[0, 4]], [0.0, 4.0], [0]):
        with pytest.raises(ValueError, match="segment_base must"):
            fm.fm_cross_features(d, [(0, 1)], bad)
    for pairs, word in (([], "1..64 terms"), ([(0, 1)] * 65, "1..64 terms"), ([(1, 0)], "a <= b"), ([(0, 3)], "a <= b"), ([(-1, 0)], "a <= b"), ([(0,)], "must be"),
                        ([(0, 1, 2, 3)], "must be"), ([(0, 1.5)], "must be"), ([(0, True)], "must be"), ([(0, 1, -1)], "n_buckets"), ([(0, 1, 2**32)], "n_buckets"),
                        (5, "pairs must be"), ([3], "pairs must be")):
        with pytest.raises(ValueError, match=word):
            fm.fm_cross_features(d, pairs, fields)
    for buckets in (-1, 2**32, 1.5, True):
        with pytest.raises(ValueError, match="buckets must be an integer"):
            fm.fm_cross_features(d, [(0, 1)], fields, buckets=buckets)
    with pytest.raises(ValueError, match="keep must be"):
        fm.fm_cross_features(d, [(0, 1)], fields, keep=1)
    with pytest.raises(ValueError, match="seed must be"):
        fm.fm_cross_features(d, [(0, 1)], fields, seed=0.5)
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        fm.fm_cross_features(d, [(0, 1, 2**31)], fields)
    with pytest.raises(TypeError, match="Crossing"):
        fm.fm_apply_crosses(d, {"terms": []})
    names = ["a", "b", "c0", "c1"]
    from fmwr_amd.api import _cross_names
    new = _cross_names(names, fields, [(0, 2, 0), (1, 2, 3), (2, 2, 0)], True)
    assert new == names + ["a:c0", "a:c1", "1x2#0", "1x2#1", "1x2#2", "c0:c0", "c0:c1", "c1:c0", "c1:c1"]
    assert _cross_names(names, fields, [(0, 1, 0)], False) == ["a:b"]
    c = fm.Crossing(np.array(fields, np.uint32), [(0, 2, 0), (1, 2, 3)], 7, 0, True, np.array([4, 6, 9], np.uint32), d.feature_names, ["x"] * 9)
    assert c.new_p == 9 and c.new_segment_base.tolist() == [0, 1, 2, 4, 6, 9] and c.terms == [(0, 2, 0), (1, 2, 3)]
    assert fm.Crossing(np.array(fields, np.uint32), [(0, 2, 0)], 0, 0, False, np.array([0, 2], np.uint32), d.feature_names, ["x"] * 2).new_segment_base.tolist() == [0, 2]
    other = fm.fm_matrix(np.ones((2, 4)), feature_names=["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_apply_crosses(other, c)
    m = fm.Matrix(None, 3, 4, 0)
    with pytest.raises(ValueError, match="segment_base must"):
        m.cross([0, 5], [(0, 0)])
    with pytest.raises(ValueError, match="a <= b"):
        m.cross([0, 2, 4], [(1, 0)])
    with pytest.raises(ValueError, match="2\\^32 - 2"):
        m.cross([0, 2, 4], [(0, 1, 2**32 - 5)])
    with pytest.raises(ValueError, match="fields must ascend"):
        fm.fm_cross_candidates({"Model": {"w": np.zeros(4)}}, d, [0, 5])
