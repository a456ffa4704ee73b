"""fmx_metrics / fmx_metrics_device / fm_metrics against the numpy model of the definition (tests/metrics_model.py), fed with fmx_predict's own z and
p for the same engine and matrix: the integers in every bit, the quotients of integers in every bit, the sums within the summation bound, in
every engine form, on the edge scores, in each of the three pair-counting forms and on their boundaries; the invariances of a group's bits; the
refusals; fm_metrics end to end."""
import ctypes
import math

import numpy as np
import pytest
import scipy.sparse as sp

from tests import metrics_model as mm

pytestmark = pytest.mark.gpu

KINDS = ["seq64", "mb32", "mb32_wir", "mb64"]
U = 2.0 ** -53
# (classification, link): all four accepted links
CASES = {"cls_logistic": (True, mm.LINK_LOGISTIC), "cls_probit": (True, mm.LINK_PROBIT), "reg_none": (False, mm.LINK_NONE), "reg_clamp": (False, mm.LINK_CLAMP)}
FORMS = {"mixed": (4, 8), "wave": (64, 0), "workgroup": (-1, 2 ** 30), "global": (-1, -1)}   # the hook's (wave_rows, lds_rows)


def _engine(kind, p, k, monkeypatch, cls, seed=0, w0=0.3, w=None, v=None, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    common = dict(num_factor=k, task=L.TASK_CLASSIFICATION if cls else L.TASK_REGRESSION, min_target=-0.6, max_target=0.9, **kw)
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, **common)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), **common)
    rng = np.random.default_rng(seed + 7 * k + 1)
    e.set_params(w0, rng.normal(0, 0.5, p) if w is None else w, rng.normal(0, 0.4, (k, p)) if v is None else v)
    return e


def _limits(wave=0, lds=0, chunk=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_metrics_limits(wave, lds, chunk))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _limits()


def _random_matrix(n, p, rng, cls, lens=(0, 9)):
    from fmwr_amd import engine
    ln = rng.integers(lens[0], lens[1], n)
    rp = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    col = rng.integers(0, p, int(rp[-1])).astype(np.uint32)
    val = rng.normal(0, 1, int(rp[-1])).astype(np.float32)
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0) if cls else rng.normal(0, 1, n).astype(np.float32).astype(np.float64)
    return engine.Matrix.from_csr(rp, col, val, p, y), y


def _one_hot(cols, vals, p, y):
    """row r = the single entry (cols[r], vals[r]): its raw score is w0 + w[cols[r]] vals[r] when the factors are zero"""
    from fmwr_amd import engine
    n = len(cols)
    return engine.Matrix.from_csr(np.arange(n + 1, dtype=np.int64), np.asarray(cols, np.uint32), np.asarray(vals, np.float32), p, y)


def _scores(e, mat, link):
    from fmwr_amd import _lib as L
    return e.predict(mat, L.LINK_NONE), e.predict(mat, link)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((mm.bits(a) == mm.bits(b)) | (np.isnan(a) & np.isnan(b))))


def _same(got, ref, what=""):
    assert _same_bits(got[0], ref[0]), (what, "value bits")
    assert np.array_equal(got[1], ref[1]), (what, "counts")


WORST = {"sum": 0.0, "logloss": 0.0}


def _check(got, z, p, y, groups, G, cls, link, what=""):
    """the returned (value, count) against the model fed with z and p"""
    value, count = got
    rc, rv, ra = mm.metrics(z, p, y, groups, G, cls, link)
    assert value.shape == (G, 6) and count.shape == (G, 4)
    assert count.tolist() == rc, (what, "counts")
    for g in range(G):
        rows = rc[g][0]
        exact = (0, 2, 5) if cls else ()
        for j in range(6):
            a, b, w = float(value[g, j]), float(rv[g][j]), (what, g, j, float(value[g, j]), float(rv[g][j]))
            if not cls and j == 1:   # RMSE: the IEEE square root of the returned MSE
                assert _same_bits(a, np.sqrt(value[g, 0])), w
            elif j in exact or rows == 0 or math.isnan(b) or math.isinf(b):
                assert _same_bits(a, b), w
            elif cls and j == 1:     # LOGLOSS: the device exp / log1p / log
                tol = 1e-12 * max(1.0, abs(b))
                WORST["logloss"] = max(WORST["logloss"], abs(a - b) / tol)
                assert abs(a - b) <= tol, w
            else:                    # a fixed-order sum against fsum: the summation bound
                tol = rows * U * float(ra[g][j])
                if abs(a - b) > 0:
                    WORST["sum"] = max(WORST["sum"], abs(a - b) / tol)
                assert abs(a - b) <= tol, w
    return rc, rv


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("k", [0, 3, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_every_engine_form_task_and_link(kind, k, case, monkeypatch):
    cls, link = CASES[case]
    rng = np.random.default_rng(100 + k)
    n, p, G = 300, 60, 11
    e = _engine(kind, p, k, monkeypatch, cls)
    mat, y = _random_matrix(n, p, rng, cls)
    groups = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 10], n, p=[.02, .03, .05, .1, .1, .1, .2, .2, .2]).astype(np.uint32)   # 5 and 9 stay empty
    groups[:1] = 9                                                                                              # ... and 9 holds one row
    z, pr = _scores(e, mat, link)
    _limits(4, 8, 16)   # all three forms, the forward in chunks of 16 rows
    got = e.metrics(mat, groups, G, link)
    rc, _ = _check(got, z, pr, y, groups, G, cls, link, (kind, k, case))
    assert rc[5][0] == 0 and rc[9][0] == 1 and max(c[0] for c in rc) > 8
    _limits()
    _same(e.metrics(mat, groups, G, link), got, "default limits")
    pooled = e.metrics(mat, None, None, link)
    _check(pooled, z, pr, y, None, 1, cls, link, (kind, k, case, "pooled"))
    print("largest share of the bars so far:", WORST)


# columns 3 and 4 are stored with the value 1e30: in fp64 tables w x overflows to +-inf (in fp32 tables the weights themselves are infinite, and the
# forward's padding slots turn such a row's score into NaN: more NaN scores, no infinite ones)
W_EDGE = np.array([0.5, 0.5, -0.25, 1e300, -1e300, np.nan, 0.0, -0.0, 1e-3, 2.0], np.float64)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("kind,link", [("seq64", mm.LINK_LOGISTIC), ("seq64", mm.LINK_PROBIT), ("mb64", mm.LINK_LOGISTIC), ("mb64", mm.LINK_PROBIT),
                                       ("mb32", mm.LINK_LOGISTIC)])   # (fp32 tables: NaN in place of the infinite scores, so no probit case)
def test_edge_scores_in_every_form(kind, link, form, monkeypatch):
    """all tied; two distinct values; -0 against +0; +-inf; NaN scores; groups of one class; empty and one-row groups.  (Under the probit link
    the NaN weight is a number: fmx_predict's table lookup, which feeds the model, is not defined for a NaN score.)"""
    rng = np.random.default_rng(7)
    p = len(W_EDGE)
    w = np.where(np.isnan(W_EDGE), 0.125, W_EDGE) if link == mm.LINK_PROBIT else W_EDGE
    e = _engine(kind, p, 3, monkeypatch, True, w0=0.0, w=w, v=np.zeros((3, p)), keep_w0=0)
    sets = [[0, 1], [0, 2], [6, 7], [3, 4, 0], [5, 0, 2], [5], list(range(p)), list(range(p)), [], [8], [0, 9], [3], [4, 5]]
    sizes = [30, 30, 20, 30, 30, 6, 70, 40, 0, 1, 12, 9, 9]
    cols, groups = [], []
    for g, (s, m) in enumerate(zip(sets, sizes)):
        cols += list(rng.choice(s, m)) if m else []
        groups += [g] * m
    n, G = len(cols), len(sets)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    groups = np.array(groups, np.uint32)
    y[groups == 10] = 1.0    # all positive
    y[groups == 11] = -1.0   # all negative
    order = rng.permutation(n)
    cols, groups, y = np.array(cols)[order], groups[order], y[order]
    mat = _one_hot(cols, np.where((cols == 3) | (cols == 4), 1e30, 1.0), p, y)
    z, pr = _scores(e, mat, link)
    assert (np.isnan(z).any() or link == mm.LINK_PROBIT) and (np.isinf(z).any() or kind == "mb32") and (np.isposinf(z).any() == np.isneginf(z).any()) and len(np.unique(z[groups == 0])) == 1 and len(np.unique(z[groups == 1])) == 2
    _limits(*FORMS[form])
    got = e.metrics(mat, groups, G, link)
    rc, rv = _check(got, z, pr, y, groups, G, True, link, (kind, link, form))
    assert rc[0][2] == rc[0][1] * (rc[0][0] - rc[0][1])               # all tied: pairs2 = P N
    assert rc[2][2] == rc[2][1] * (rc[2][0] - rc[2][1])               # -0 == +0
    assert rc[5][2] == rc[5][1] * (rc[5][0] - rc[5][1])               # NaN == NaN
    assert rc[8] == [0, 0, 0, 0] and np.isnan(got[0][8]).all()
    assert np.isnan(got[0][10, 0]) and np.isnan(got[0][11, 0]) and got[0][10, 5] == 1.0 and got[0][11, 5] == 0.0
    _limits()
    _same(e.metrics(mat, groups, G, link), got, "against the default limits")


SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 17, 40]


def _interleaved(sizes, rng):
    g = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)]).astype(np.uint32)
    return g[rng.permutation(len(g))]


@pytest.mark.parametrize("kind", ["mb32", "mb64"])
def test_form_boundaries_through_the_hook(kind, monkeypatch):
    rng = np.random.default_rng(21)
    p, k = 40, 3
    groups = _interleaved(SIZES, rng)
    n, G = len(groups), len(SIZES)
    e = _engine(kind, p, k, monkeypatch, True)
    from fmwr_amd import engine
    rp = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
    col = rng.integers(0, 6, 2 * n).astype(np.uint32)     # few distinct rows: ties inside the groups
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    mat = engine.Matrix.from_csr(rp, col, np.ones(2 * n, np.float32), p, y)
    z, pr = _scores(e, mat, mm.LINK_LOGISTIC)
    assert len(np.unique(z)) < n / 3
    _limits(4, 8)
    ref = e.metrics(mat, groups, G, mm.LINK_LOGISTIC)
    _check(ref, z, pr, y, groups, G, True, mm.LINK_LOGISTIC, "wave 4, lds 8")
    for form, (wave, lds) in FORMS.items():
        for chunk in (0, 16):
            _limits(wave, lds, chunk)
            _same(e.metrics(mat, groups, G, mm.LINK_LOGISTIC), ref, (form, chunk))
    for wave, lds in ((1, 2), (3, 4), (5, 7), (8, 9), (16, 17), (17, 39), (39, 40)):
        _limits(wave, lds)
        _same(e.metrics(mat, groups, G, mm.LINK_LOGISTIC), ref, (wave, lds))


def test_default_limits_on_their_boundaries(monkeypatch):
    rng = np.random.default_rng(22)
    sizes = [63, 64, 65, 1023, 1024, 1025, 2049]
    groups = _interleaved(sizes, rng)
    n, G, p = len(groups), len(sizes), 50
    for cls, link in ((True, mm.LINK_LOGISTIC), (False, mm.LINK_CLAMP)):
        e = _engine("mb32", p, 3, monkeypatch, cls)
        mat, y = _random_matrix(n, p, rng, cls, lens=(1, 4))   # short rows: many equal scores
        z, pr = _scores(e, mat, link)
        got = e.metrics(mat, groups, G, link)
        rc, _ = _check(got, z, pr, y, groups, G, cls, link, "default limits")
        assert [c[0] for c in rc] == sizes
        _limits(-1, -1)
        _same(e.metrics(mat, groups, G, link), got, "global form")
        _limits()
        _check(e.metrics(mat, None, 1, link), z, pr, y, None, 1, cls, link, "pooled: one group of 5 313 rows")


def _hip():
    import os
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library is not loadable")


class _Dev:
    """host arrays mirrored in buffers of the HIP runtime's own"""

    def __init__(self, *arrays):
        self.hip, self.host, self.ptr = _hip(), [np.ascontiguousarray(a) for a in arrays], []
        for a in self.host:
            d = ctypes.c_void_p()
            assert self.hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(a.nbytes, 8))) == 0
            if a.nbytes:
                assert self.hip.hipMemcpy(d, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), 1) == 0   # hipMemcpyHostToDevice
            self.ptr.append(d)

    def __getitem__(self, i):
        return self.ptr[i].value

    def read(self):
        out = [np.empty_like(a) for a in self.host]
        for d, h in zip(self.ptr, out):
            if h.nbytes:
                assert self.hip.hipMemcpy(h.ctypes.data_as(ctypes.c_void_p), d, ctypes.c_size_t(h.nbytes), 2) == 0   # hipMemcpyDeviceToHost
        return out

    def free(self):
        for d in self.ptr:
            self.hip.hipFree(d)


def _device_form(e, mat, r0, r1, groups, G, link, count=True):
    """fmx_metrics_device for rows [r0, r1); groups (uint32, indexed from r0) or None"""
    dev = _Dev(np.zeros(0, np.uint32) if groups is None else np.asarray(groups, np.uint32), np.full((G, 6), 7.0), np.full((G, 4), 7, np.int64))
    try:
        e.metrics_device(mat, r0, r1, None if groups is None else dev[0], G, dev[1], dev[2] if count else None, link)
        e.sync()
        _, value, cnt = dev.read()
    finally:
        dev.free()
    return value, cnt


@pytest.mark.parametrize("case", ["cls_logistic", "reg_none"])
def test_a_groups_bits_depend_on_its_own_rows_alone(case, monkeypatch):
    cls, link = CASES[case]
    rng = np.random.default_rng(31)
    p, k = 50, 3
    sizes = [3, 70, 0, 57, 9, 1]
    G = len(sizes)
    # rows [20, 130) hold every row of groups 1 and 4 (interleaved, with rows of group 3 among them)
    inner = _interleaved([0, 70, 0, 31, 9, 0], rng)
    outer = _interleaved([3, 0, 0, 9, 0, 1], rng)
    groups = np.concatenate([outer, np.full(7, 3), inner, np.full(10, 3)]).astype(np.uint32)
    n = len(groups)
    assert n == 140 and [int((groups == g).sum()) for g in range(G)] == sizes
    e = _engine("mb32", p, k, monkeypatch, cls)
    mat, y = _random_matrix(n, p, rng, cls, lens=(1, 3))
    z, pr = _scores(e, mat, link)
    _limits(4, 8)
    ref = e.metrics(mat, groups, G, link)
    _check(ref, z, pr, y, groups, G, cls, link)
    _same(e.metrics(mat, groups, G, link), ref, "a second call")
    # group ids renumbered
    perm = rng.permutation(G)
    got = e.metrics(mat, perm[groups].astype(np.uint32), G, link)
    _same((got[0][perm], got[1][perm]), ref, "renumbered")
    # n_groups enlarged with empty groups
    got = e.metrics(mat, groups, G + 5, link)
    _same((got[0][:G], got[1][:G]), ref, "more groups")
    assert np.isnan(got[0][G:]).all() and not got[1][G:].any()
    # the host form against the device form, with and without the counts
    dv = _device_form(e, mat, 0, n, groups, G, link)
    _same(dv, ref, "device form")
    assert _same_bits(_device_form(e, mat, 0, n, groups, G, link, count=False)[0], ref[0])
    # a sub-range that still holds the whole of groups 1 and 4: the other groups' rows dropped
    sub = _device_form(e, mat, 20, 130, groups[20:130], G, link)
    for g in (1, 4):
        _same((sub[0][g], sub[1][g]), (ref[0][g], ref[1][g]), ("sub-range", g))
    assert sub[1][3, 0] == 31 and sub[1][0, 0] == 0
    # ... and permuted: another matrix whose rows of the other groups are shuffled among their slots
    from fmwr_amd import engine
    rp, col, val, yy = mat.export()
    others = np.flatnonzero((groups != 1) & (groups != 4))
    src = np.arange(n)
    src[others] = rng.permutation(others)
    rp2 = np.concatenate([[0], np.cumsum(np.diff(rp)[src])]).astype(np.int64)
    idx = np.concatenate([np.arange(rp[s], rp[s + 1]) for s in src]).astype(np.int64)
    mat2 = engine.Matrix.from_csr(rp2, col[idx], val[idx], p, y[src])
    got = e.metrics(mat2, groups[src], G, link)
    for g in (1, 4):
        _same((got[0][g], got[1][g]), (ref[0][g], ref[1][g]), ("others permuted", g))
    # no group ids against one explicit group
    _same(e.metrics(mat, None, None, link), e.metrics(mat, np.zeros(n, np.uint32), 1, link), "NULL groups")
    _same(_device_form(e, mat, 0, n, None, 1, link), e.metrics(mat, None, None, link), "NULL groups, device form")
    # the device form ignores an id out of range: those rows belong to no group
    bad = groups.copy()
    bad[groups == 3] = np.where(rng.random(57) < 0.5, G, 2 ** 32 - 1)
    got = _device_form(e, mat, 0, n, bad, G, link)
    keep = groups != 3
    rc, rv, _ = mm.metrics(z[keep], pr[keep], y[keep], groups[keep], G, cls, link)
    assert got[1].tolist() == rc and got[1][3].tolist() == [0, 0, 0, 0] and np.isnan(got[0][3]).all()
    for g in (0, 1, 4, 5):
        _same((got[0][g], got[1][g]), (ref[0][g], ref[1][g]), ("bad ids", g))


def test_refusals_leave_the_outputs_alone(monkeypatch):
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(1)
    p, n = 30, 12
    e = _engine("mb32", p, 3, monkeypatch, True)
    reg = _engine("mb32", p, 3, monkeypatch, False)
    rank = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, num_factor=3, task=L.TASK_RANKING)
    mat, y = _random_matrix(n, p, rng, True)
    other, _ = _random_matrix(n, p + 1, rng, True)
    rp, col, val, _ = mat.export()
    bare = engine.Matrix.from_csr(rp, col, val, p)
    value, count = np.full((3, 6), 7.0), np.full((3, 4), 7, np.int64)
    pv, pc = value.ctypes.data_as(ctypes.c_void_p), count.ctypes.data_as(ctypes.c_void_p)
    groups = (np.arange(n) % 3).astype(np.uint32)
    pg = groups.ctypes.data_as(ctypes.c_void_p)
    dev = _Dev(groups, value, count)
    lib = L.lib()
    LG, NO = L.LINK_LOGISTIC, L.LINK_NONE
    calls = [
        lambda: lib.fmx_metrics(rank.h, mat.h, pg, 3, NO, pv, pc),            # a RANKING engine
        lambda: lib.fmx_metrics(e.h, bare.h, pg, 3, LG, pv, pc),              # no labels
        lambda: lib.fmx_metrics(e.h, other.h, pg, 3, LG, pv, pc),             # p mismatch
        lambda: lib.fmx_metrics(e.h, None, pg, 3, LG, pv, pc),
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 3, NO, pv, pc),               # a link of the other family
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 3, L.LINK_CLAMP, pv, pc),
        lambda: lib.fmx_metrics(reg.h, mat.h, pg, 3, LG, pv, pc),
        lambda: lib.fmx_metrics(reg.h, mat.h, pg, 3, L.LINK_PROBIT, pv, pc),
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 3, 4, pv, pc),
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 2, LG, pv, pc),               # a group id 2 with 2 groups
        lambda: lib.fmx_metrics(e.h, mat.h, None, 3, LG, pv, pc),             # no group ids: one group
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 0, LG, pv, pc),
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 2 ** 31, LG, pv, pc),
        lambda: lib.fmx_metrics(e.h, mat.h, pg, 3, LG, None, pc),             # NULL output
        lambda: lib.fmx_metrics_device(rank.h, mat.h, 0, n, dev[0], 3, NO, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, bare.h, 0, n, dev[0], 3, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, other.h, 0, n, dev[0], 3, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 0, n, dev[0], 3, NO, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 0, n, None, 3, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 0, n, dev[0], 0, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 2, 1, dev[0], 3, LG, dev[1], dev[2]),     # bad ranges
        lambda: lib.fmx_metrics_device(e.h, mat.h, -1, 1, dev[0], 3, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 0, n + 1, dev[0], 3, LG, dev[1], dev[2]),
        lambda: lib.fmx_metrics_device(e.h, mat.h, 0, n, dev[0], 3, LG, None, dev[2]),
    ]
    try:
        for i, call in enumerate(calls):
            assert call() == L.ERR_INVALID, i
            assert lib.fmx_last_error().decode(), i
        # an empty matrix and an empty range are fine and write nothing
        empty = engine.Matrix.from_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), p, np.zeros(0))
        assert lib.fmx_metrics(e.h, empty.h, pg, 3, LG, None, None) == L.OK
        assert lib.fmx_metrics_device(e.h, mat.h, 5, 5, dev[0], 3, LG, None, None) == L.OK
        e.sync()
        _, dvalue, dcount = dev.read()
    finally:
        dev.free()
    assert np.all(value == 7.0) and np.all(count == 7) and np.all(dvalue == 7.0) and np.all(dcount == 7)
    assert lib.fmx_metrics(e.h, mat.h, pg, 3, LG, pv, None) == L.OK   # the counts may be NULL
    assert not np.any(value == 7.0) and np.all(count == 7)


def test_parameters_are_not_modified_and_a_multi_gpu_engine_reads_its_primary_replica(monkeypatch):
    rng = np.random.default_rng(4)
    p, k, n, G = 60, 3, 200, 6
    mat, y = _random_matrix(n, p, rng, True)
    groups = rng.integers(0, G, n).astype(np.uint32)
    e = _engine("mb32", p, k, monkeypatch, True, n_gpus=2, gpus_share_device=1)
    one = _engine("mb32", p, k, monkeypatch, True)
    before = e.get_params()
    z, pr = _scores(e, mat, mm.LINK_LOGISTIC)
    got = e.metrics(mat, groups, G, mm.LINK_LOGISTIC)
    _check(got, z, pr, y, groups, G, True, mm.LINK_LOGISTIC)
    _same(one.metrics(mat, groups, G, mm.LINK_LOGISTIC), got, "one replica")
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_fm_metrics_end_to_end():
    import fmwr_amd as fm
    rng = np.random.default_rng(13)
    n, p = 400, 30
    X = sp.random(n, p, density=0.2, random_state=3, format="csr")
    X.data = rng.normal(0, 1, X.nnz)
    X.sort_indices()
    truth = X @ rng.normal(0, 1, p)
    y = np.where(truth + rng.normal(0, 0.5, n) > 0, 1.0, 0.0)
    users = rng.integers(100, 120, n) * 7   # any integer values
    fit = fm.fm_train(fm.fm_matrix(X, y), normalize=False, seed=1,
                      control=[fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=4000, solver=fm.SGD_solver())])
    out = fm.fm_metrics(fit, fm.fm_matrix(X, y), groups=users, normalize=False)
    pred = fm.predict(fit, fm.fm_matrix(X), normalize=False)
    auc = mm.rank_sum_auc(pred, y > 0)
    assert abs(out["pooled"]["auc"] - auc) < 1e-12 and auc > 0.6
    assert out["pooled"]["accuracy"] == np.mean((pred >= 0.5) == (y > 0))
    assert abs(out["pooled"]["brier"] - np.mean((pred - y) ** 2)) < 1e-12 and abs(out["pooled"]["mean_pred"] - pred.mean()) < 1e-12
    assert abs(out["pooled"]["logloss"] + np.mean(np.where(y > 0, np.log(pred), np.log1p(-pred)))) < 1e-9
    ids = np.unique(users)
    assert np.array_equal(out["groups"], ids) and np.array_equal(out["counts"]["rows"], [np.sum(users == u) for u in ids])
    per = [mm.rank_sum_auc(pred[users == u], y[users == u] > 0) for u in ids]
    assert np.allclose(out["per_group"]["auc"], per, rtol=0, atol=1e-12)
    rows = out["counts"]["rows"]
    assert abs(out["gauc"] - np.sum(np.array(per) * rows) / rows.sum()) < 1e-12 and abs(out["macro_auc"] - np.mean(per)) < 1e-12
    plain = fm.fm_metrics(fit, fm.fm_matrix(X, y), normalize=False)
    assert plain["groups"] is None and plain["pooled"] == out["pooled"] and abs(plain["gauc"] - plain["pooled"]["auc"]) < 1e-15
    # the planted case: scores that are user offsets only -- a high pooled AUC, and one half for every user
    z, yy, user = mm.planted_gauc(np.random.default_rng(3))
    levels = np.unique(z)
    Xp = sp.csr_matrix((np.ones(len(z)), (np.arange(len(z)), np.searchsorted(levels, z))), shape=(len(z), len(levels)))
    model = dict(fit["Model"], w0=0.0, w=levels.copy(), v=np.zeros((4, len(levels))))
    planted = fm.fm_metrics(dict(fit, Model=model), fm.fm_matrix(Xp, yy), groups=user, normalize=False)
    assert planted["gauc"] == 0.5 and planted["macro_auc"] == 0.5 and np.all(planted["per_group"]["auc"] == 0.5)
    assert planted["pooled"]["auc"] > 0.75
    # a REGRESSION model
    yr = truth + rng.normal(0, 0.1, n)
    fitr = fm.fm_train(fm.fm_matrix(X, yr), normalize=False, seed=1,
                       control=[fm.model_control("REGRESSION", **{"factor.number": 4}), fm.solver_control(max_iter=2000, solver=fm.SGD_solver())])
    outr = fm.fm_metrics(fitr, fm.fm_matrix(X, yr), groups=users, normalize=False)
    predr = fm.predict(fitr, fm.fm_matrix(X), normalize=False)
    y32 = yr.astype(np.float32).astype(np.float64)   # the device holds the labels in fp32
    assert abs(outr["pooled"]["mse"] - np.mean((predr - y32) ** 2)) < 1e-12 * max(1.0, np.mean((predr - y32) ** 2))
    assert outr["pooled"]["rmse"] == np.sqrt(outr["pooled"]["mse"]) and abs(outr["pooled"]["mae"] - np.mean(np.abs(predr - y32))) < 1e-12
    assert "gauc" not in outr and not outr["counts"]["positives"].any()
