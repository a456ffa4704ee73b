"""CPU-side checks of the target-encoding surface (fmx_target_stats, fmx_matrix_encode_targets; fmwr_amd.fm_encode_targets / fm_apply_targets): the
properties of the numpy model of the definition (tests/target_model.py), the leak the folds are there to close, the declared surface, and the
argument checks, which run before any device."""
import ctypes as C
import os
import pickle
import re

import numpy as np
import pytest

from tests import columns_model as colm
from tests import target_cases as tc
from tests import target_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from fmwr_amd import build, _lib
    build.build()
    return _lib


# ---------------------------------------------------------------------------------------------------------------------------- the model
def test_a_parts_cells_sum_to_column_stats_and_one_part_is_the_totals():
    rp, col, val, y = tc.ragged()
    n = len(rp) - 1
    whole, _ = colm.column_stats(rp, col, val, y, tc.RAGGED_P)
    lo, hi, term_base = tm.layout(tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS)
    cols = np.concatenate([np.arange(a, b) for a, b in zip(lo, hi)])
    assert len(cols) == term_base[-1] == 33
    part = np.random.default_rng(1).integers(0, 5, n).astype(np.uint32)
    for target in (tm.POSITIVE, tm.LABEL):
        count, total = tm.target_stats(rp, col, y, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 5, target, part)
        assert np.array_equal(count.sum(axis=1), whole[cols][:, 1:])                  # rows and positive rows of fmx_matrix_column_stats
        one, tone = tm.target_stats(rp, col, y, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 1, target, None)
        N, A, T = tm.totals(count, total)
        assert np.array_equal(one[:, 0, 0], N) and np.array_equal(one[:, 0, 1], A)     # n_parts = 1 with part = NULL: the totals
        zeros = tm.target_stats(rp, col, y, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 1, target, np.zeros(n, np.uint32))
        assert np.array_equal(zeros[0], one) and (target == tm.POSITIVE or np.array_equal(tc.bits64(zeros[1]), tc.bits64(tone)))
        if target == tm.LABEL:
            assert np.allclose(tone[:, 0], T, rtol=1e-12, atol=1e-9)                  # another association of the same labels
    # rows without a valid part are counted nowhere
    cut = part.copy()
    cut[::3] = tc.NO_PART
    cut[1::3] = 5
    kept = np.flatnonzero(cut < 5)
    rows = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in kept])
    sub_rp = np.concatenate([[0], np.cumsum(np.diff(rp)[kept])])
    a = tm.target_stats(rp, col, y, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 5, tm.LABEL, cut)
    b = tm.target_stats(sub_rp, col[rows], y[kept], tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 5, tm.LABEL, cut[kept])
    assert np.array_equal(a[0], b[0]) and np.array_equal(tc.bits64(a[1]), tc.bits64(b[1]))   # a cell's bits depend on its own row list alone


def test_out_of_fold_values_never_read_the_rows_own_fold():
    rp, col, val, y = tc.ragged()
    n = len(rp) - 1
    part = (np.arange(n) % 5).astype(np.uint32)
    rng = np.random.default_rng(2)
    for target in (tm.POSITIVE, tm.LABEL):
        count, total = tm.target_stats(rp, col, y, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, 5, target, part)
        ref = tm.encode_values(rp, col, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, count, total, target, part, 0.3, 20.0)
        for f in range(5):
            c2 = count.copy()
            c2[:, f] = rng.integers(0, 1000, c2[:, f].shape)                          # fold f's cells rewritten ...
            t2 = None
            if total is not None:
                t2 = total.copy()
                t2[:, f] = 0.0                                                         # (a sum whose removal is exact: T - 0)
                base0 = total.copy()
                base0[:, f] = 0.0
                ref_f = tm.encode_values(rp, col, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, count, base0, target, part, 0.3, 20.0)
            else:
                ref_f = ref
            got = tm.encode_values(rp, col, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, c2, t2, target, part, 0.3, 20.0)
            mine = part == f
            assert mine.any()
            for g, r in zip(got[1:], ref_f[1:]):
                assert np.array_equal(g[mine], r[mine])                                # ... and the rows of fold f do not move
        # part = None and rows without a valid part take the totals
        none = tm.encode_values(rp, col, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, count, total, target, None, 0.3, 20.0)
        out = tm.encode_values(rp, col, tc.RAGGED_P, tc.RAGGED_BASE, tc.RAGGED_TERMS, count, total, target, np.full(n, tc.NO_PART, np.uint32), 0.3, 20.0)
        for a, b in zip(none, out):
            assert np.array_equal(a, b)
        N, _, _ = tm.totals(count, total)
        assert np.array_equal(none[1][:, 0][none[0][:, 0]], np.full(none[0][:, 0].sum(), N[0]))   # the dense column's COUNT is its row count


def test_the_prior_at_an_empty_denominator_and_counts_that_round_once():
    rp = np.array([0, 1, 2, 4], np.int64)
    col = np.array([0, 1, 2, 2], np.uint32)
    val = np.ones(4, np.float32)
    base, terms = [0, 3], [0]
    count = np.zeros((3, 1, 2), np.int64)
    count[1, 0] = (2**24 + 1, 2**24 + 1)
    count[2, 0] = (2**53 + 1, 3)
    for target, total in ((tm.POSITIVE, None), (tm.LABEL, np.array([[0.0], [5.0], [1e30]]))):
        present, n, mean, cnt = tm.encode_values(rp, col, 3, base, terms, count, total, target, None, 0.25, 0.0)
        assert present.all() and n[:, 0].tolist() == [0, 2**24 + 1, 2 * (2**53 + 1)]      # a column stored twice is two entries
        assert mean[0, 0] == tc.bits(np.float32(0.25))[0]                              # strength = 0 and n = 0: den == 0, the prior
        assert cnt[0, 0] == 0 and cnt[1, 0] == tc.bits(np.float32(2**24))[0]           # 2^24 + 1 is a tie: to even, rounded once from the integer
        assert cnt[2, 0] == tc.bits(np.float32(2.0**54))[0]
        if target == tm.POSITIVE:
            assert mean[1, 0] == tc.bits(np.float32(1.0))[0] and mean[2, 0] == tc.bits(np.float32(6.0 / float(2 * (2**53 + 1))))[0]
        else:
            assert mean[2, 0] == tc.bits(np.float32((1e30 + 1e30) / float(2 * (2**53 + 1))))[0]
    # a NaN result is the canonical one; den = 0 with strength > 0 cannot happen, den < 0 (an injected table) divides like any other
    count[0, 0] = (-20, 0)
    _, n, mean, _ = tm.encode_values(rp, col, 3, base, terms, count, np.array([[np.inf], [-np.inf], [np.nan]]), tm.LABEL, None, 0.5, 20.0)
    assert mean[0, 0] == tc.bits(np.float32(0.5))[0] and mean[1, 0] == tc.bits(np.float32(-np.inf))[0] and mean[2, 0] == tm.NAN32
    out = tm.encode(rp, col, val, 3, base, terms, count, None, tm.POSITIVE, None, [3], 0.25, 1.0, True)
    assert out[3].tolist() == [3, 5] and out[0].tolist() == [0, 3, 6, 10] and out[1].tolist() == [0, 3, 4, 1, 3, 4, 2, 2, 3, 4]
    assert tm.encode(rp, col, val, 3, base, terms, count, None, tm.POSITIVE, None, [2], 0.25, 1.0, False)[1].tolist() == [0, 0, 0]


def test_model_refusals():
    rp, col, val, y = tc.ragged()
    good = dict(rp=rp, col=col, y=y, p=tc.RAGGED_P, segment_base=tc.RAGGED_BASE, term_segment=[0, 2])
    for kw in (dict(segment_base=[1, 41]), dict(segment_base=[0, 40]), dict(segment_base=[0, 9, 5, 41]), dict(term_segment=[]), dict(term_segment=[2, 0]),
               dict(term_segment=[1, 1]), dict(term_segment=[7]), dict(term_segment=list(range(65))), dict(n_parts=0), dict(n_parts=65), dict(target=2), dict(y=None)):
        with pytest.raises(ValueError):
            tm.target_stats(**dict(good, **kw))
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        tm.layout(2**26, [0, 2**26], [0], 32)
    assert tm.layout(2**26 - 1, [0, 2**26 - 1], [0], 32)[2].tolist() == [0, 2**26 - 1]
    count, _ = tm.target_stats(**good)
    for kw in (dict(kinds=[0, 1]), dict(kinds=[1, 4]), dict(kinds=[1]), dict(strength=-1.0), dict(strength=np.inf), dict(prior=np.nan)):
        with pytest.raises(ValueError):
            tm.encode(rp, col, val, tc.RAGGED_P, tc.RAGGED_BASE, [0, 2], count, None, **dict(dict(kinds=[1, 1], prior=0.1, strength=1.0), **kw))
    with pytest.raises(ValueError, match="2\\^32 - 2"):
        tm.enc_bases(2**32 - 3, [3], True)
    assert tm.enc_bases(2**32 - 4, [3], True) == [2**32 - 4, 2**32 - 2] and tm.enc_bases(2**32 - 3, [3], False) == [0, 2]


# ----------------------------------------------------------------------------------------------------------------------------- the leak
def _auc(s, y):
    """the Mann-Whitney AUC with midranks"""
    o = np.argsort(s, kind="stable")
    s, y = s[o], y[o]
    _, first, cnt = np.unique(s, return_index=True, return_counts=True)
    rank = np.repeat(first + (cnt - 1) / 2.0 + 1.0, cnt)
    P = y.sum()
    N = len(y) - P
    return (rank[y == 1].sum() - P * (P + 1) / 2.0) / (P * N)


@pytest.mark.parametrize("strength", [0.0, 1.0, 20.0])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_naive_encoding_leaks_the_label_and_the_out_of_fold_one_does_not(seed, strength):
    """4 000 rows, 1 000 ids, 5 parts, labels independent of the ids: the encoding fitted on the rows it is applied to ranks a row by its own label
    (AUC 0.77 - 0.80), the out-of-fold one does not (0.45 - 0.49); with a per-id rate planted the out-of-fold column carries it (0.71 - 0.76)"""
    rng = np.random.default_rng(seed)
    n, W, F = 4000, 1000, 5
    c = rng.integers(0, W, n)
    y = (rng.random(n) < 0.3).astype(np.int64)
    part = (rng.permutation(n) % F).astype(np.uint32)
    rp = np.arange(n + 1, dtype=np.int64)

    def columns(labels):
        lab = np.where(labels == 1, 1.0, -1.0).astype(np.float32)
        count, _ = tm.target_stats(rp, c, lab, W, [0, W], [0], F, tm.POSITIVE, part)
        naive = tm.encode_values(rp, c, W, [0, W], [0], count, None, tm.POSITIVE, None, 0.3, strength)[2][:, 0].view(np.float32)
        oof = tm.encode_values(rp, c, W, [0, W], [0], count, None, tm.POSITIVE, part, 0.3, strength)[2][:, 0].view(np.float32)
        return naive, oof
    naive, oof = columns(y)
    rate = rng.random(W)
    y2 = (rng.random(n) < rate[c]).astype(np.int64)
    _, oof2 = columns(y2)
    a_naive, a_oof, a_planted = _auc(naive, y), _auc(oof, y), _auc(oof2, y2)
    print(f"seed {seed} strength {strength}: noise naive {a_naive:.3f} oof {a_oof:.3f} | planted oof {a_planted:.3f}")
    assert a_naive >= 0.70
    assert 0.40 <= a_oof <= 0.52
    assert a_planted >= 0.65


# ------------------------------------------------------------------------------------------------------------------- the declared surface
NAMES = ["fmx_target_stats", "fmx_target_stats_device", "fmx_target_table_from_arrays", "fmx_target_table_info", "fmx_target_table_export", "fmx_target_table_free",
         "fmx_matrix_encode_targets", "fmx_matrix_encode_targets_device"]


def test_target_entry_points_are_declared_and_exported():
    L = _lib()
    text = open(os.path.join(ROOT, "include", "fmx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.SYMBOLS and hasattr(L.lib(), name), name
    assert "fmx_debug_target_limits" in L.TEST_HOOKS and hasattr(L.lib(), "fmx_debug_target_limits")
    assert "fmx_debug_target_limits" not in text                              # the hook stays out of the public header
    assert header.index("fmx_matrix_cross") < header.index("fmx_target_stats")
    for name, struct in (("fmx_target_spec", L.TargetSpec), ("fmx_encode_spec", L.EncodeSpec)):
        fields = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", header, flags=re.S).group(1)
        declared = []
        for decl in fields.split(";"):
            if decl.strip():
                declared += [re.sub(r"^.*[\s\*]", "", part.strip()) for part in decl.split(",")]
        assert declared == [f[0] for f in struct._fields_], name
    assert C.sizeof(L.TargetSpec) == 48 and C.sizeof(L.EncodeSpec) == 40
    for macro, value in (("FMX_TARGET_POSITIVE", L.TARGET_POSITIVE), ("FMX_TARGET_LABEL", L.TARGET_LABEL), ("FMX_ENCODE_MEAN", L.ENCODE_MEAN),
                         ("FMX_ENCODE_COUNT", L.ENCODE_COUNT)):
        assert int(re.search(r"#define " + macro + r" (\d+)", header).group(1)) == value
    assert (L.TARGET_POSITIVE, L.TARGET_LABEL, L.ENCODE_MEAN, L.ENCODE_COUNT) == (tm.POSITIVE, tm.LABEL, tm.MEAN, tm.COUNT)
    assert L.TARGET_MAX_TERMS == tm.MAX_TERMS == 64 and L.TARGET_MAX_PARTS == tm.MAX_PARTS == 64
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "## 31" in design and "Not built" in design.split("## 31")[1]
    import fmwr_amd as fm
    for f in (fm.fm_encode_targets, fm.fm_apply_targets, fm.TargetEncoding, fm.TargetTable, fm.Matrix.target_stats, fm.Matrix.encode_targets,
              fm.TargetTable.from_arrays, fm.TargetTable.export, fm.TargetTable.info, fm.TargetTable.free):
        assert callable(f)
    assert "fm_target.hip" in __import__("fmwr_amd.build", fromlist=["SOURCES"]).SOURCES
    src = open(os.path.join(ROOT, "fmwr_amd", "csrc", "fm_target.hip")).read()
    assert '#include "fm_prims.h"' in src and "rocprim" not in src                            # the sort and the scans are the shared ones
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"atomicAdd\s*\(\s*[^,]*\b(float|double)", code) and "unsafeAtomicAdd" not in code and "__ddiv_rn" in code


def _tspec(L, keep, **kw):
    v = dict(n_segments=3, segment_base=np.array([0, 4, 4, 10], np.uint32), term_segment=np.array([0, 2], np.uint32), n_parts=5, target=0, reserved=0)
    v.update(kw)
    base, seg = v["segment_base"], v["term_segment"]
    keep.extend([base, seg])
    s = L.TargetSpec(C.sizeof(L.TargetSpec), v["n_segments"], None if base is None else base.ctypes.data, v.get("n_terms", 0 if seg is None else len(seg)),
                     None if seg is None else seg.ctypes.data, v["n_parts"], v["target"], v["reserved"])
    if "struct_size" in kw:
        s.struct_size = kw["struct_size"]
    return s


def test_refusals_come_before_any_device_and_write_nothing():
    """every refusal that can be seen without the matrix comes before the matrix is looked at: with a NULL matrix the message names the argument.
    None of them may touch a device: on a machine without one that would be FMX_ERR_NOGPU, not FMX_ERR_INVALID"""
    L = _lib()
    lib = L.lib()
    keep = []
    u32 = lambda *a: np.array(a, np.uint32)
    many = np.arange(4098, dtype=np.uint32)
    cases = ((dict(spec=None), "spec is NULL"), (dict(struct_size=44), "struct_size"), (dict(reserved=1), "spec.reserved"),
             (dict(n_segments=0), "n_segments"), (dict(n_segments=4097, segment_base=many), "n_segments"), (dict(n_segments=-1), "n_segments"),
             (dict(term_segment=u32()), "n_terms"), (dict(n_terms=65), "n_terms"), (dict(n_terms=-1), "n_terms"),
             (dict(n_parts=0), "n_parts"), (dict(n_parts=65), "n_parts"), (dict(target=2), "target"), (dict(target=-1), "target"),
             (dict(segment_base=None), "segment_base is NULL"), (dict(term_segment=None, n_terms=1), "term_segment is NULL"),
             (dict(segment_base=u32(1, 4, 4, 10)), "start at 0"), (dict(segment_base=u32(0, 5, 4, 10)), "descends"),
             (dict(term_segment=u32(2, 0)), "ascend strictly"), (dict(term_segment=u32(1, 1)), "ascend strictly"), (dict(term_segment=u32(0, 3)), "segment 3"),
             (dict(segment_base=u32(0, 4, 4, 2**29 + 4), n_parts=4), "2^31 - 1"))
    for call in ("stats", "stats_device", "from_arrays"):
        for kw, word in cases + (((dict(), "NULL matrix"),) if call != "from_arrays" else ((dict(count=None), "count is NULL"), (dict(target=1), "sum is NULL"))):
            kw = dict(kw)
            h = C.c_void_p(5)
            count = np.zeros((10, 5, 2), np.int64) if kw.pop("count", 1) is not None else None
            s = None if "spec" in kw else _tspec(L, keep, **kw)
            ref = None if s is None else C.byref(s)
            if call == "from_arrays":
                st = lib.fmx_target_table_from_arrays(0, ref, None if count is None else count.ctypes.data_as(C.c_void_p), None, C.byref(h))
            else:
                st = getattr(lib, "fmx_target_" + call)(None, None, ref, C.byref(h))
            assert st == L.ERR_INVALID and not h.value and word in lib.fmx_last_error().decode(), (call, kw, lib.fmx_last_error())
        good = _tspec(L, keep)
        assert (lib.fmx_target_table_from_arrays(0, C.byref(good), None, None, None) if call == "from_arrays" else
                getattr(lib, "fmx_target_" + call)(None, None, C.byref(good), None)) == L.ERR_INVALID
    # the apply: what can be seen without the table comes before it
    kinds = u32(1, 3)
    got = np.full(3, 7, np.uint32)
    pg = got.ctypes.data_as(C.c_void_p)
    for call in (lib.fmx_matrix_encode_targets, lib.fmx_matrix_encode_targets_device):
        for kw, word in ((dict(spec=None), "spec is NULL"), (dict(enc_base=None), "enc_base"), (dict(struct_size=36), "struct_size"), (dict(reserved=1), "reserved"),
                         (dict(keep_source=2), "keep_source"), (dict(kinds=None), "kinds is NULL"), (dict(strength=-0.5), "strength"), (dict(strength=np.nan), "strength"),
                         (dict(strength=np.inf), "strength"), (dict(prior=np.nan), "prior"), (dict(prior=-np.inf), "prior"), (dict(), "table is NULL")):
            v = dict(struct_size=C.sizeof(L.EncodeSpec), keep_source=1, kinds=kinds, prior=0.3, strength=20.0, reserved=0, enc_base=pg)
            v.update(kw)
            s = None if "spec" in kw else L.EncodeSpec(v["struct_size"], v["keep_source"], None if v["kinds"] is None else v["kinds"].ctypes.data, v["prior"], v["strength"],
                                                       v["reserved"])
            h = C.c_void_p(5)
            st = call(None, None, None, None if s is None else C.byref(s), v["enc_base"], C.byref(h))
            assert st == L.ERR_INVALID and not h.value and word in lib.fmx_last_error().decode(), (kw, lib.fmx_last_error())
    assert np.all(got == 7)
    info = np.zeros(8, np.int64)
    assert lib.fmx_target_table_info(None, info.ctypes.data_as(C.c_void_p)) == L.ERR_INVALID and lib.fmx_target_table_export(None, None, None, None, None) == L.ERR_INVALID
    assert lib.fmx_target_table_free(None) == L.OK
    assert lib.fmx_debug_target_limits(-1, 4, 7, 16) == L.OK and lib.fmx_debug_target_limits(0, -1, 0, 0) == L.OK and lib.fmx_debug_target_limits(0, 0, 0, 0) == L.OK


@pytest.fixture
def no_device(monkeypatch):
    from fmwr_amd import api
    for name in ("_device_matrix", "_engine_for", "split_assign"):
        monkeypatch.setattr(api, name, lambda *a, **k: pytest.fail("a device was touched"))
    monkeypatch.setattr(api.Matrix, "from_csr", classmethod(lambda *a, **k: pytest.fail("a device was touched")))


def test_python_refusals_come_before_any_device(no_device):
    import fmwr_amd as fm
    from fmwr_amd.api import _target_names
    d = fm.fm_matrix(np.random.default_rng(0).random((6, 4)), np.arange(6) % 2)
    fields = [0, 1, 2, 4]
    for f in (lambda x: fm.fm_encode_targets(x, fields, [2]), lambda x: fm.fm_apply_targets(x, None)):
        with pytest.raises(TypeError, match="fm.matrix"):
            f(np.ones((6, 4)))
    for bad in ([0, 1, 2, 3], [1, 2, 4], [0, 3, 2, 4], [[0, 4]], [0.0, 4.0], [0]):
        with pytest.raises(ValueError, match="fields must ascend"):
            fm.fm_encode_targets(d, bad, [0])
    for bad in ([], [3], [-1], [1, 0], [1, 1], [0.5], 2):
        with pytest.raises(ValueError, match="encode must hold"):
            fm.fm_encode_targets(d, fields, bad)
    for kw, word in ((dict(folds=1), "folds"), (dict(folds=65), "folds"), (dict(folds=2.5), "folds"), (dict(kinds=()), "kinds"), (dict(kinds=("mean", "mean")), "kinds"),
                     (dict(kinds="median"), "kinds"), (dict(keep=1), "keep must be"), (dict(seed=0.5), "seed"), (dict(strength=-1), "strength"),
                     (dict(strength=np.nan), "strength"), (dict(prior=np.inf), "prior"), (dict(target="rate"), "target must be"), (dict(how="within"), "needs `by`"),
                     (dict(by=[0, 1]), "by must hold")):
        with pytest.raises(ValueError, match=word):
            fm.fm_encode_targets(d, fields, [2], **kw)
    with pytest.raises(ValueError, match="needs labels"):
        fm.fm_encode_targets(fm.fm_matrix(np.ones((2, 4))), fields, [2])
    with pytest.raises(TypeError, match="TargetEncoding"):
        fm.fm_apply_targets(d, {"count": []})
    names = ["a", "b", "c0", "c1"]
    assert _target_names(names, fields, [0, 2], [3, 1], True) == names + ["te(a)", "cnt(a)", "te(2)"]
    assert _target_names(names, fields, [1], [2], False) == ["cnt(b)"]
    enc = fm.TargetEncoding(fields, [0, 2], 5, "positive", np.zeros((3, 5, 2), np.int64), None, [3, 1], 0.25, 20.0, True, [4, 6, 7], d.feature_names, ["x"] * 7)
    assert enc.new_p == 7 and enc.new_segment_base.tolist() == [0, 1, 2, 4, 6, 7]
    back = pickle.loads(pickle.dumps(enc))
    assert back.new_segment_base.tolist() == [0, 1, 2, 4, 6, 7] and np.array_equal(back.count, enc.count) and back.kinds.tolist() == [3, 1] and back.target == "positive"
    assert fm.TargetEncoding(fields, [0], 2, "label", None, None, [1], 0.0, 1.0, False, [0, 1], d.feature_names, ["x"]).new_segment_base.tolist() == [0, 1]
    other = fm.fm_matrix(np.ones((2, 4)), feature_names=["a", "b", "c", "d"])
    with pytest.raises(ValueError, match="not the same"):
        fm.fm_apply_targets(other, enc)
    m = fm.Matrix(None, 3, 4, 0)
    with pytest.raises(ValueError, match="segment_base must"):
        m.target_stats(None, [0, 5], [0])
    with pytest.raises(ValueError, match="term_segment must"):
        m.target_stats(None, [0, 2, 4], [1, 0])
    with pytest.raises(ValueError, match="n_parts must"):
        m.target_stats(None, [0, 2, 4], [1], n_parts=65)
    with pytest.raises(ValueError, match="part must hold"):
        m.target_stats([0, 1], [0, 2, 4], [1])
    with pytest.raises(TypeError, match="TargetTable"):
        m.encode_targets(None)
