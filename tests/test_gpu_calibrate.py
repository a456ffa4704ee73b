"""fmx_reliability / fmx_calibrate_platt / fmx_calibrate_isotonic / fmx_predict_calibrated (and the _device forms, and the fm_* functions) against
the numpy model of the definition (tests/calibrate_model.py), fed with fmx_predict's own z and p for the same engine and matrix: the integers, the
score bounds, the bins, the steps and the step predictions in every bit, ECE and MCE in every bit given the device's own table, the sums, the
log loss, the Platt predictions and (a, b) within the bars the project already uses; the invariances of a group's bits; the refusals."""
import ctypes
import math

import numpy as np
import pytest

from tests import calibrate_model as cm
from tests import metrics_model as mm

pytestmark = pytest.mark.gpu

KINDS = ["seq64", "mb32", "mb32_wir", "mb64"]
U = 2.0 ** -53
AB_BAR = 1e-11
WORST = {"sum": 0.0, "logloss": 0.0, "platt_pred": 0.0, "ab": 0.0}   # the largest share of each bar seen


def _engine(kind, p, k, monkeypatch, seed=0, w0=0.3, w=None, v=None, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    common = dict(num_factor=k, task=L.TASK_CLASSIFICATION, **kw)
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, **common)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), **common)
    rng = np.random.default_rng(seed + 7 * k + 1)
    e.set_params(w0, rng.normal(0, 0.5, p) if w is None else w, rng.normal(0, 0.4, (k, p)) if v is None else v)
    return e


def _hook(chunk=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_calibrate_limits(chunk))


@pytest.fixture(autouse=True)
def _default_limits():
    yield
    _hook()


def _random_matrix(n, p, rng, lens=(0, 9)):
    from fmwr_amd import engine
    ln = rng.integers(lens[0], lens[1], n)
    rp = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    col = rng.integers(0, p, int(rp[-1])).astype(np.uint32)
    val = rng.normal(0, 1, int(rp[-1])).astype(np.float32)
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0)
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


def _same_table(got, ref, what="", sel=None):
    for name in ("count", "sum_p", "lo_z", "hi_z", "nan_rows", "value"):
        a, b = (got[name], ref[name]) if sel is None else (got[name][sel[0]], ref[name][sel[1]])
        assert (np.array_equal(a, b) if a.dtype == np.int64 else _same_bits(a, b)), (what, name)


def _same_map(got, ref, what=""):
    for name in ref:
        if name != "kind":
            a, b = np.asarray(got[name]), np.asarray(ref[name])
            assert (_same_bits(a, b) if a.dtype == np.float64 else np.array_equal(a, b)), (what, name)


def _interleaved(sizes, rng):
    g = np.concatenate([np.full(s, i) for i, s in enumerate(sizes)]).astype(np.uint32)
    return g[rng.permutation(len(g))]


def _check_table(got, z, p, y, groups, G, B, binning, what=""):
    """a returned table against the model fed with z and p"""
    t = cm.table(z, p, y, groups, G, B, binning)
    assert got["count"].shape == (G, B, 2) and got["value"].shape == (G, 4)
    assert got["count"].tolist() == t["count"], (what, "counts")
    assert got["nan_rows"].tolist() == t["nan_rows"], (what, "nan_rows")
    assert _same_bits(got["lo_z"], t["lo_z"]) and _same_bits(got["hi_z"], t["hi_z"]), (what, "lo_z / hi_z")
    g_of = np.zeros(len(z), np.int64) if groups is None else np.asarray(groups, np.int64)
    for g in range(G):
        s = t["s"][g]
        for b in range(B):
            rows = t["count"][g][b][0]
            a, r = float(got["sum_p"][g, b]), float(t["sum_p"][g, b])
            if rows == 0 or math.isnan(r) or math.isinf(r):
                assert _same_bits(a, r if rows else 0.0), (what, g, b, a, r)
            else:
                tol = rows * U * float(t["sum_p_abs"][g, b])
                if abs(a - r) > 0:
                    WORST["sum"] = max(WORST["sum"], abs(a - r) / tol)
                assert abs(a - r) <= tol, (what, "sum_p", g, b, a, r)
        # ECE and MCE: the model's operations on the device's own table
        ece, mce = cm.ece_mce(got["count"][g].tolist(), got["sum_p"][g])
        assert _same_bits(got["value"][g, 0], ece) and _same_bits(got["value"][g, 1], mce), (what, "ECE / MCE", g, got["value"][g], ece, mce)
        for j, name in ((2, "brier"), (3, "logloss")):
            a, (r, ra) = float(got["value"][g, j]), t[name][g]
            if s == 0 or math.isnan(r) or math.isinf(r):
                assert _same_bits(a, r), (what, name, g, a, r)
            elif name == "logloss":
                tol = 1e-12 * max(1.0, abs(r))
                WORST["logloss"] = max(WORST["logloss"], abs(a - r) / tol)
                assert abs(a - r) <= tol, (what, name, g, a, r)
            else:
                tol = s * U * float(ra)
                if abs(a - r) > 0:
                    WORST["sum"] = max(WORST["sum"], abs(a - r) / tol)
                assert abs(a - r) <= tol, (what, name, g, a, r)
    if binning == cm.BINS_MASS:   # the bin of every row, recovered from the table's score bounds
        k = cm.order_key(z)
        with np.errstate(all="ignore"):
            lo, hi = cm.order_key(got["lo_z"]), cm.order_key(got["hi_z"])
        full = got["count"][:, :, 0] > 0
        for r in np.flatnonzero(t["bin"] >= 0):
            inside = np.flatnonzero(full[g_of[r]] & (lo[g_of[r]] <= k[r]) & (k[r] <= hi[g_of[r]]))
            assert inside.tolist() == [t["bin"][r]], (what, "the bin of row", r)
    return t


def _check_isotonic(fit, z, p, y, groups, G, B, what=""):
    t = cm.table(z, p, y, groups, G, B, cm.BINS_MASS)
    for g in range(G):
        ns, thr, val = cm.pav(t["count"][g], t["lo_z"][g])
        assert fit["n_steps"][g] == ns and _same_bits(fit["thr"][g], thr) and _same_bits(fit["val"][g], val), (what, g)


def _check_platt_pred(got, cal, z, groups, what=""):
    ref = cm.apply_map(cal, z, groups)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    ok = ~nan & (ref != 0)
    assert np.array_equal(got[~nan & ~ok], ref[~nan & ~ok]), what
    if ok.any():
        rel = np.abs(got[ok] - ref[ok]) / np.abs(ref[ok])
        WORST["platt_pred"] = max(WORST["platt_pred"], float(rel.max()) / 1e-12)
        assert rel.max() <= 1e-12, (what, rel.max())


@pytest.mark.parametrize("link", [mm.LINK_LOGISTIC, mm.LINK_PROBIT])
@pytest.mark.parametrize("k", [0, 3, 16])
@pytest.mark.parametrize("kind", KINDS)
def test_every_engine_form_and_link(kind, k, link, monkeypatch):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(100 + k)
    n, p, G = 300, 60, 11
    e = _engine(kind, p, k, monkeypatch)
    mat, y = _random_matrix(n, p, rng)
    groups = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 10], n, p=[.02, .03, .05, .1, .1, .1, .2, .2, .2]).astype(np.uint32)   # 5 stays empty
    groups[:1] = 9                                                                                              # ... and 9 holds one row
    z, pr = _scores(e, mat, link)
    before = e.get_params()
    _hook(16)   # the forward in calls of 16 rows
    tables = {}
    for binning in (L.BINS_WIDTH, L.BINS_MASS):
        tables[binning] = e.reliability(mat, groups, G, 10, binning, None, link)
        _check_table(tables[binning], z, pr, y, groups, G, 10, binning, (kind, k, link, binning))
    iso = e.calibrate_isotonic(mat, groups, G, 64)
    _check_isotonic(iso, z, pr, y, groups, G, 64, (kind, k))
    steps = e.predict_calibrated(mat, iso, groups, G)
    assert _same_bits(steps, cm.apply_map(iso, z, groups)), "STEPS predictions"
    fit = e.calibrate_platt(mat, groups, G, 0.1, 3)
    assert fit["rows"].tolist() == [int((groups == g).sum()) for g in range(G)] and fit["status"][5] == 0 and fit["ab"][5].tolist() == [1.0, 0.0]
    _check_platt_pred(e.predict_calibrated(mat, fit, groups, G), fit, z, groups, "PLATT predictions")
    ident = {"kind": "platt", "ab": np.array([[1.0, 0.0]])}
    assert _same_bits(e.predict_calibrated(mat, ident), e.predict(mat, L.LINK_LOGISTIC)), "(1, 0) is fmx_predict(LOGISTIC)"
    assert _same_bits(e.predict_calibrated(mat, None, link=link), pr), "no calibrator is fmx_predict(link)"
    # the reliability of the calibrated probabilities: the model fed with the device's own p
    for cal in (iso, fit):
        pc = e.predict_calibrated(mat, cal, groups, G)
        _check_table(e.reliability(mat, groups, G, 10, L.BINS_WIDTH, cal), z, pc, y, groups, G, 10, cm.BINS_WIDTH, (kind, k, cal["kind"]))
    _hook()
    for binning in (L.BINS_WIDTH, L.BINS_MASS):
        _same_table(e.reliability(mat, groups, G, 10, binning, None, link), tables[binning], "one forward call")
    _same_map(e.calibrate_isotonic(mat, groups, G, 64), iso)
    _same_map(e.calibrate_platt(mat, groups, G, 0.1, 3), fit)
    pooled = e.reliability(mat, None, None, 10, L.BINS_MASS, None, link)
    _check_table(pooled, z, pr, y, None, 1, 10, cm.BINS_MASS, "pooled")
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])
    print("largest share of the bars so far:", WORST)


SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 17, 40, 63, 64, 65, 1023, 1024, 1025, 2049]
_SIZES_CASE = {}


def _sizes_case(monkeypatch):
    """interleaved groups of every size, few distinct scores: one engine, matrix and forward for every B"""
    if not _SIZES_CASE:
        rng = np.random.default_rng(21)
        p, k = 40, 3
        groups = _interleaved(SIZES, rng)
        n = len(groups)
        e = _engine("mb64", p, k, monkeypatch)
        from fmwr_amd import engine
        rp = np.arange(0, 2 * n + 1, 2, dtype=np.int64)
        col = rng.integers(0, 9, 2 * n).astype(np.uint32)     # few distinct rows: ties inside the groups
        y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
        mat = engine.Matrix.from_csr(rp, col, np.ones(2 * n, np.float32), p, y)
        z, pr = _scores(e, mat, mm.LINK_LOGISTIC)
        assert len(np.unique(z)) < 100
        _SIZES_CASE.update(e=e, mat=mat, z=z, pr=pr, y=y, groups=groups)
    c = _SIZES_CASE
    return c["e"], c["mat"], c["z"], c["pr"], c["y"], c["groups"]


@pytest.mark.parametrize("B", [1, 2, 10, 64, 1024])
def test_group_sizes_and_bin_counts(B, monkeypatch):
    from fmwr_amd import _lib as L
    e, mat, z, pr, y, groups = _sizes_case(monkeypatch)
    G = len(SIZES)
    for binning in (L.BINS_WIDTH, L.BINS_MASS):
        got = e.reliability(mat, groups, G, B, binning)
        t = _check_table(got, z, pr, y, groups, G, B, binning, (B, binning))
        assert t["s"] == SIZES
    iso = e.calibrate_isotonic(mat, groups, G, B)
    _check_isotonic(iso, z, pr, y, groups, G, B, B)
    assert _same_bits(e.predict_calibrated(mat, iso, groups, G), cm.apply_map(iso, z, groups))
    if B == 1024:   # B >= s for the smaller groups: the exact isotonic regression, every distinct score a bin of its own
        t = cm.table(z, pr, y, groups, G, B, cm.BINS_MASS)
        g = SIZES.index(40)
        assert sum(1 for c in t["count"][g] if c[0]) == len(np.unique(cm.order_key(z[groups == g])))
    pooled = e.reliability(mat, None, None, B, L.BINS_MASS)
    _check_table(pooled, z, pr, y, None, 1, B, cm.BINS_MASS, ("pooled", B))
    print("largest share of the bars so far:", WORST)


# columns 3 and 4 are stored with the value 1e30: in fp64 tables w x overflows to +-inf (in fp32 tables the weights themselves are infinite, and the
# forward's padding slots turn such a row's score into NaN: more NaN scores, no infinite ones)
W_EDGE = np.array([0.5, 0.5, -0.25, 1e300, -1e300, np.nan, 0.0, -0.0, 1e-3, 2.0], np.float64)


@pytest.mark.parametrize("kind,link", [("seq64", mm.LINK_LOGISTIC), ("seq64", mm.LINK_PROBIT), ("mb64", mm.LINK_LOGISTIC), ("mb32", mm.LINK_LOGISTIC)])
def test_edge_scores(kind, link, monkeypatch):
    """all tied; two distinct values; -0 against +0; +-inf; NaN scores; groups of one class; empty and one-row groups.  (Under the probit link the
    NaN weight is a number: fmx_predict's table lookup, which feeds the model, is not defined for a NaN score.)"""
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(7)
    p = len(W_EDGE)
    w = np.where(np.isnan(W_EDGE), 0.125, W_EDGE) if link == mm.LINK_PROBIT else W_EDGE
    e = _engine(kind, p, 3, monkeypatch, w0=0.0, w=w, v=np.zeros((3, p)), keep_w0=0)
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
    assert (np.isnan(z).any() or link == mm.LINK_PROBIT) and (np.isinf(z).any() or kind == "mb32") and len(np.unique(z[groups == 0])) == 1
    assert len(np.unique(z[groups == 1])) == 2 and not z[groups == 2].any()
    both_zeros = {math.copysign(1, v) for v in z[groups == 2]} == {1.0, -1.0}   # (a forward that adds +0.0 leaves no -0)
    for B in (1, 3, 10, 64):
        for binning in (L.BINS_WIDTH, L.BINS_MASS):
            got = e.reliability(mat, groups, G, B, binning, None, link)
            t = _check_table(got, z, pr, y, groups, G, B, binning, (kind, link, B, binning))
            assert sum(1 for c in t["count"][0] if c[0]) == 1                                         # all tied: one bin
            if binning == L.BINS_MASS:
                assert sum(1 for c in t["count"][2] if c[0]) == 1                                     # -0 == +0: one run
                b0 = [c[0] > 0 for c in t["count"][2]].index(True)
                assert not both_zeros or (math.copysign(1, got["lo_z"][2, b0]) < 0 and math.copysign(1, got["hi_z"][2, b0]) > 0)   # ... from -0 to +0
            assert t["count"][8] == [[0, 0]] * B and np.isnan(got["value"][8]).all()
            if link == mm.LINK_LOGISTIC:
                assert got["nan_rows"][5] == 6 and np.isnan(got["value"][5]).all() and not got["count"][5].any()
        iso = e.calibrate_isotonic(mat, groups, G, B)
        _check_isotonic(iso, z, pr, y, groups, G, B, (kind, link, B))
        assert iso["n_steps"][8] == 0 and iso["n_steps"][10] == 1 and iso["val"][10, 0] == 1.0
        assert iso["val"][11, 0] == 0.0 if kind != "mb32" else iso["n_steps"][11] == 0   # (fp32 tables: that group's scores are NaN)
        ps = e.predict_calibrated(mat, iso, groups, G)
        assert _same_bits(ps, cm.apply_map(iso, z, groups))
        # a step map returns 0 and 1: the log loss is +inf where it is wrong, and the model says the same
        _check_table(e.reliability(mat, groups, G, 4, L.BINS_WIDTH, iso), z, ps, y, groups, G, 4, cm.BINS_WIDTH, (kind, link, B, "steps"))
    for lam in (0.0, 0.1):
        fit = e.calibrate_platt(mat, groups, G, lam, 4)
        for g in range(G):
            sel = groups == g
            a, b, rows, status = cm.platt(z[sel], y[sel], lam, 4, np.float64)
            assert fit["rows"][g] == rows, (lam, g)
            if rows == 0:   # (with rows the pivots of a one-class group sit on the edge of rounding: the status is not pinned there)
                assert fit["status"][g] == status and _same_bits(fit["ab"][g], [float(a), float(b)]), (lam, g)
            assert fit["status"][g] == 0 or np.isnan(fit["ab"][g]).all()
        _check_platt_pred(e.predict_calibrated(mat, fit, groups, G), fit, z, groups, ("edge", lam))
    print("largest share of the bars so far:", WORST)


@pytest.mark.parametrize("kind", KINDS)
def test_platt_against_the_long_double_model(kind, monkeypatch):
    """every case of calibrate_model.platt_cases as one group of one call: (a, b) within 1e-11 of max(|a|, |b|) of the long double model"""
    cases = cm.platt_cases()
    base = np.concatenate([[0], np.cumsum([len(c[1]) for c in cases])])
    p = int(base[-1])
    w = np.concatenate([c[1] for c in cases])
    e = _engine(kind, p, 3, monkeypatch, w0=0.0, w=w, v=np.zeros((3, p)), keep_w0=0)
    rng = np.random.default_rng(3)
    for lam in (0.0, 0.1):
        use = [i for i, c in enumerate(cases) if c[4] == lam]
        cols = np.concatenate([cases[i][2] + base[i] for i in use])
        y = np.concatenate([cases[i][3] for i in use])
        groups = np.concatenate([np.full(len(cases[i][2]), j) for j, i in enumerate(use)]).astype(np.uint32)
        order = rng.permutation(len(cols))
        cols, y, groups = cols[order], y[order], groups[order]
        mat = _one_hot(cols, np.ones(len(cols)), p, y)
        z, _ = _scores(e, mat, mm.LINK_LOGISTIC)
        _hook(16 if lam else 0)
        fit = e.calibrate_platt(mat, groups, len(use), lam, 8)
        for j, i in enumerate(use):
            sel = groups == j
            assert len(np.unique(z[sel])) >= 2 and (lam > 0 or len(np.unique(y[sel])) == 2)
            a, b, rows, status = cm.platt(z[sel], y[sel], lam, 8)
            assert status == 0 and fit["status"][j] == 0 and fit["rows"][j] == rows == len(cases[i][2]), cases[i][0]
            scale = max(abs(float(a)), abs(float(b)))
            err = max(abs(fit["ab"][j, 0] - float(a)), abs(fit["ab"][j, 1] - float(b))) / scale
            WORST["ab"] = max(WORST["ab"], err / AB_BAR)
            assert err <= AB_BAR, (cases[i][0], fit["ab"][j], float(a), float(b), err)
        _check_platt_pred(e.predict_calibrated(mat, fit, groups, len(use)), fit, z, groups, ("cases", lam))
    print("largest share of the bars so far:", WORST)


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


def _device_forms(e, mat, r0, r1, groups, G, B, binning, lam, steps, cal=None):
    """the four _device forms for rows [r0, r1); groups (uint32, indexed from r0) or None: (table, platt fit, isotonic fit, predictions)"""
    n = r1 - r0
    dev = _Dev(np.zeros(0, np.uint32) if groups is None else np.asarray(groups, np.uint32),
               np.full((G, B, 2), 7, np.int64), np.full((G, B), 7.0), np.full((G, B), 7.0), np.full((G, B), 7.0), np.full(G, 7, np.int64), np.full((G, 4), 7.0),
               np.full((G, 2), 7.0), np.full(G, 7, np.int64), np.full(G, 7, np.int32),
               np.full(G, 7, np.int32), np.full((G, B), 7.0), np.full((G, B), 7.0), np.full(n, 7.0))
    dg = None if groups is None else dev[0]
    try:
        e.reliability_device(mat, r0, r1, dg, G, B, binning, dev[1], dev[2], dev[3], dev[4], dev[5], dev[6])
        e.calibrate_platt_device(mat, r0, r1, dg, G, lam, steps, dev[7], dev[8], dev[9])
        e.calibrate_isotonic_device(mat, r0, r1, dg, G, B, dev[10], dev[11], dev[12])
        e.predict_calibrated_device(mat, r0, r1, dg, G, dev[13], cal)
        e.sync()
        o = dev.read()
    finally:
        dev.free()
    table = {"count": o[1], "sum_p": o[2], "lo_z": o[3], "hi_z": o[4], "nan_rows": o[5], "value": o[6]}
    return table, {"kind": "platt", "ab": o[7], "rows": o[8], "status": o[9]}, {"kind": "steps", "n_steps": o[10], "thr": o[11], "val": o[12]}, o[13]


@pytest.mark.parametrize("binning", [cm.BINS_WIDTH, cm.BINS_MASS])
def test_a_groups_bits_depend_on_its_own_rows_alone(binning, monkeypatch):
    from fmwr_amd import engine
    rng = np.random.default_rng(31)
    p, k, B, lam, steps = 50, 3, 7, 0.1, 3
    sizes = [3, 70, 0, 57, 9, 1]
    G = len(sizes)
    # rows [20, 130) hold every row of groups 1 and 4 (interleaved, with rows of group 3 among them)
    inner = _interleaved([0, 70, 0, 31, 9, 0], rng)
    outer = _interleaved([3, 0, 0, 9, 0, 1], rng)
    groups = np.concatenate([outer, np.full(7, 3), inner, np.full(10, 3)]).astype(np.uint32)
    n = len(groups)
    assert n == 140 and [int((groups == g).sum()) for g in range(G)] == sizes
    e = _engine("mb32", p, k, monkeypatch)
    mat, y = _random_matrix(n, p, rng, lens=(1, 3))
    z, pr = _scores(e, mat, mm.LINK_LOGISTIC)

    def host(m, gr, ng, cal=None):
        return e.reliability(m, gr, ng, B, binning), e.calibrate_platt(m, gr, ng, lam, steps), e.calibrate_isotonic(m, gr, ng, B)

    ref = host(mat, groups, G)
    _check_table(ref[0], z, pr, y, groups, G, B, binning)
    again = host(mat, groups, G)
    _same_table(again[0], ref[0], "a second call"), _same_map(again[1], ref[1], "a second call"), _same_map(again[2], ref[2], "a second call")
    # group ids renumbered
    perm = rng.permutation(G)
    got = host(mat, perm[groups].astype(np.uint32), G)
    _same_table({k_: v[perm] for k_, v in got[0].items()}, ref[0], "renumbered")
    for i in (1, 2):
        _same_map({k_: (v[perm] if k_ != "kind" else v) for k_, v in got[i].items()}, ref[i], "renumbered")
    # n_groups enlarged with empty groups
    got = host(mat, groups, G + 5)
    _same_table({k_: v[:G] for k_, v in got[0].items()}, ref[0], "more groups")
    assert np.isnan(got[0]["value"][G:]).all() and not got[0]["count"][G:].any() and not got[2]["n_steps"][G:].any()
    assert got[1]["ab"][G:].tolist() == [[1.0, 0.0]] * 5 and _same_bits(got[1]["ab"][:G], ref[1]["ab"]) and _same_bits(got[2]["val"][:G], ref[2]["val"])
    # the host forms against the device forms
    per_group = ref[1]
    dv = _device_forms(e, mat, 0, n, groups, G, B, binning, lam, steps, per_group)
    _same_table(dv[0], ref[0], "device form"), _same_map(dv[1], ref[1], "device form"), _same_map(dv[2], ref[2], "device form")
    assert _same_bits(dv[3], e.predict_calibrated(mat, per_group, groups, G))
    # a sub-range that still holds the whole of groups 1 and 4: the other groups' rows dropped
    sub = _device_forms(e, mat, 20, 130, groups[20:130], G, B, binning, lam, steps, per_group)
    for g in (1, 4):
        _same_table(sub[0], ref[0], ("sub-range", g), (g, g))
        assert _same_bits(sub[1]["ab"][g], ref[1]["ab"][g]) and _same_bits(sub[2]["val"][g], ref[2]["val"][g]) and _same_bits(sub[2]["thr"][g], ref[2]["thr"][g])
    assert sub[0]["count"][3, :, 0].sum() == 31 and not sub[0]["count"][0].any()
    assert _same_bits(sub[3], e.predict_calibrated(mat, per_group, groups, G)[20:130])
    # ... and permuted: another matrix whose rows of the other groups are shuffled among their slots
    rp, col, val, yy = mat.export()
    others = np.flatnonzero((groups != 1) & (groups != 4))
    src = np.arange(n)
    src[others] = rng.permutation(others)
    rp2 = np.concatenate([[0], np.cumsum(np.diff(rp)[src])]).astype(np.int64)
    idx = np.concatenate([np.arange(rp[s], rp[s + 1]) for s in src]).astype(np.int64)
    mat2 = engine.Matrix.from_csr(rp2, col[idx], val[idx], p, y[src])
    got = host(mat2, groups[src], G)
    for g in (1, 4):
        _same_table(got[0], ref[0], ("others permuted", g), (g, g))
        assert _same_bits(got[1]["ab"][g], ref[1]["ab"][g]) and _same_bits(got[2]["val"][g], ref[2]["val"][g])
    # no group ids against one explicit group
    a, b = host(mat, None, None), host(mat, np.zeros(n, np.uint32), 1)
    _same_table(a[0], b[0], "NULL groups"), _same_map(a[1], b[1], "NULL groups"), _same_map(a[2], b[2], "NULL groups")
    dv1 = _device_forms(e, mat, 0, n, None, 1, B, binning, lam, steps, a[1])
    _same_table(dv1[0], a[0], "NULL groups, device form"), _same_map(dv1[1], a[1]), _same_map(dv1[2], a[2])
    # a calibrator with one map against the same map repeated per group
    for one in (a[1], a[2]):
        rep = {k_: (np.repeat(np.asarray(v), G, axis=0) if k_ != "kind" else v) for k_, v in one.items()}
        assert _same_bits(e.predict_calibrated(mat, one), e.predict_calibrated(mat, rep, groups, G)), one["kind"]
        _same_table(e.reliability(mat, groups, G, B, binning, one), e.reliability(mat, groups, G, B, binning, rep), ("one map / repeated", one["kind"]))
    # the device forms ignore an id out of range: those rows belong to no group
    bad = groups.copy()
    bad[groups == 3] = np.where(rng.random(57) < 0.5, G, 2 ** 32 - 1)
    got = _device_forms(e, mat, 0, n, bad, G, B, binning, lam, steps, per_group)
    assert not got[0]["count"][3].any() and got[0]["nan_rows"][3] == 0 and got[1]["rows"][3] == 0 and got[2]["n_steps"][3] == 0 and np.isnan(got[3][groups == 3]).all()
    for g in (0, 1, 4, 5):
        _same_table(got[0], ref[0], ("bad ids", g), (g, g))
        assert _same_bits(got[1]["ab"][g], ref[1]["ab"][g]) and _same_bits(got[2]["val"][g], ref[2]["val"][g])


def test_refusals_leave_the_outputs_alone(monkeypatch):
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(1)
    p, n = 30, 12
    e = _engine("mb32", p, 3, monkeypatch)
    reg = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, num_factor=3, task=L.TASK_REGRESSION)
    rank = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, num_factor=3, task=L.TASK_RANKING)
    mat, y = _random_matrix(n, p, rng)
    other, _ = _random_matrix(n, p + 1, rng)
    rp, col, val, _ = mat.export()
    bare = engine.Matrix.from_csr(rp, col, val, p)
    out = np.full(3 * 1024 * 2, 7.0)
    o = out.ctypes.data_as(ctypes.c_void_p)
    groups = (np.arange(n) % 3).astype(np.uint32)
    pg = groups.ctypes.data_as(ctypes.c_void_p)
    dev = _Dev(groups, out)
    d = dev[1]
    lib = L.lib()
    LG, W = L.LINK_LOGISTIC, L.BINS_WIDTH

    def cal(**kw):
        c = L.Calibrator(struct_size=ctypes.sizeof(L.Calibrator), kind=L.CAL_PLATT, n_groups=1, platt=o.value)
        for name, v in kw.items():
            setattr(c, name, v)
        return ctypes.byref(c)
    ns = np.array([2, 5, 0], np.int32)
    calls = [
        lambda: lib.fmx_reliability(rank.h, mat.h, pg, 3, 10, W, None, LG, o, o, o, o, o, o),        # RANKING and REGRESSION engines
        lambda: lib.fmx_reliability(reg.h, mat.h, pg, 3, 10, W, None, LG, o, o, o, o, o, o),
        lambda: lib.fmx_calibrate_platt(reg.h, mat.h, pg, 3, 0.1, 8, o, o, o),
        lambda: lib.fmx_calibrate_isotonic(rank.h, mat.h, pg, 3, 10, o, o, o),
        lambda: lib.fmx_predict_calibrated(reg.h, mat.h, pg, 3, None, LG, o),
        lambda: lib.fmx_reliability(e.h, bare.h, pg, 3, 10, W, None, LG, o, o, o, o, o, o),           # no labels
        lambda: lib.fmx_reliability(e.h, other.h, pg, 3, 10, W, None, LG, o, o, o, o, o, o),          # p mismatch
        lambda: lib.fmx_reliability(e.h, None, pg, 3, 10, W, None, LG, o, o, o, o, o, o),
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 3, 10, W, None, L.LINK_NONE, o, o, o, o, o, o),   # no calibrator: LOGISTIC or PROBIT
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 3, 10, W, None, L.LINK_CLAMP, o, o, o, o, o, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, None, L.LINK_NONE, o),
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 3, 0, W, None, LG, o, o, o, o, o, o),             # the bins
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 3, 1025, W, None, LG, o, o, o, o, o, o),
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 3, 10, 2, None, LG, o, o, o, o, o, o),
        lambda: lib.fmx_reliability_device(e.h, mat.h, 0, n, dev[0], 2 ** 28 // 512 + 1, 512, W, None, LG, d, d, d, d, d, d),   # n_groups * B > 2^28
        lambda: lib.fmx_calibrate_isotonic_device(e.h, mat.h, 0, n, dev[0], 2 ** 28 // 512 + 1, 512, d, d, d),
        lambda: lib.fmx_calibrate_isotonic(e.h, mat.h, pg, 3, 0, o, o, o),
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 2, 10, W, None, LG, o, o, o, o, o, o),            # a group id 2 with 2 groups
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, pg, 2, 0.1, 8, o, o, o),
        lambda: lib.fmx_calibrate_isotonic(e.h, mat.h, pg, 2, 10, o, o, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 2, None, LG, o),
        lambda: lib.fmx_reliability(e.h, mat.h, None, 3, 10, W, None, LG, o, o, o, o, o, o),          # no group ids: one group
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, None, 3, 0.1, 8, o, o, o),
        lambda: lib.fmx_calibrate_isotonic_device(e.h, mat.h, 0, n, None, 3, 10, d, d, d),
        lambda: lib.fmx_reliability(e.h, mat.h, pg, 0, 10, W, None, LG, o, o, o, o, o, o),
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, pg, 2 ** 31, 0.1, 8, o, o, o),
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, pg, 3, -0.1, 8, o, o, o),                         # lambda, n_newton
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, pg, 3, float("nan"), 8, o, o, o),
        lambda: lib.fmx_calibrate_platt(e.h, mat.h, pg, 3, 0.1, 0, o, o, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, None, LG, None),                        # NULL output
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(struct_size=8), LG, o),             # the calibrator
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(kind=3), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(kind=L.CAL_NONE, link=L.LINK_CLAMP), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(n_groups=2), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, None, 3, cal(n_groups=3), LG, o),              # per-group maps need ids
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(platt=None), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(kind=L.CAL_STEPS, n_groups=3, max_steps=0, n_steps=ns.ctypes.data, thr=o.value, val=o.value), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(kind=L.CAL_STEPS, n_groups=3, max_steps=4, n_steps=ns.ctypes.data, thr=o.value, val=o.value), LG, o),
        lambda: lib.fmx_predict_calibrated(e.h, mat.h, pg, 3, cal(kind=L.CAL_STEPS, n_groups=3, max_steps=8, n_steps=ns.ctypes.data, thr=None, val=o.value), LG, o),
        lambda: lib.fmx_reliability_device(e.h, mat.h, 2, 1, dev[0], 3, 10, W, None, LG, d, d, d, d, d, d),   # bad ranges
        lambda: lib.fmx_calibrate_platt_device(e.h, mat.h, -1, 1, dev[0], 3, 0.1, 8, d, d, d),
        lambda: lib.fmx_calibrate_isotonic_device(e.h, mat.h, 0, n + 1, dev[0], 3, 10, d, d, d),
        lambda: lib.fmx_predict_calibrated_device(e.h, mat.h, 0, n, dev[0], 3, None, LG, None),
        lambda: lib.fmx_predict_calibrated_device(rank.h, mat.h, 0, n, dev[0], 3, None, LG, d),
    ]
    try:
        for i, call in enumerate(calls):
            assert call() == L.ERR_INVALID, i
            assert lib.fmx_last_error().decode(), i
        # an empty matrix and an empty range are fine and write nothing
        empty = engine.Matrix.from_csr(np.zeros(1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), p, np.zeros(0))
        assert lib.fmx_reliability(e.h, empty.h, pg, 3, 10, W, None, LG, o, o, o, o, o, o) == L.OK
        assert lib.fmx_calibrate_platt(e.h, empty.h, pg, 3, 0.1, 8, o, o, o) == L.OK
        assert lib.fmx_calibrate_isotonic_device(e.h, mat.h, 5, 5, dev[0], 3, 10, d, d, d) == L.OK
        assert lib.fmx_predict_calibrated_device(e.h, mat.h, 5, 5, dev[0], 3, None, LG, d) == L.OK
        e.sync()
        _, dout = dev.read()
    finally:
        dev.free()
    assert np.all(out == 7.0) and np.all(dout == 7.0)
    # every output may be NULL
    assert lib.fmx_reliability(e.h, mat.h, pg, 3, 10, W, None, LG, None, None, None, None, None, o) == L.OK and not np.any(out[:12] == 7.0) and np.all(out[12:] == 7.0)
    assert lib.fmx_calibrate_platt(e.h, mat.h, pg, 3, 0.1, 2, None, None, None) == L.OK and lib.fmx_calibrate_isotonic(e.h, mat.h, pg, 3, 10, None, None, None) == L.OK


def test_a_multi_gpu_engine_reads_its_primary_replica(monkeypatch):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(4)
    p, k, n, G = 60, 3, 200, 6
    mat, y = _random_matrix(n, p, rng)
    groups = rng.integers(0, G, n).astype(np.uint32)
    e = _engine("mb32", p, k, monkeypatch, n_gpus=2, gpus_share_device=1)
    one = _engine("mb32", p, k, monkeypatch)
    before = e.get_params()
    z, pr = _scores(e, mat, mm.LINK_LOGISTIC)
    got = e.reliability(mat, groups, G, 10, L.BINS_MASS)
    _check_table(got, z, pr, y, groups, G, 10, cm.BINS_MASS)
    _same_table(one.reliability(mat, groups, G, 10, L.BINS_MASS), got, "one replica")
    fit, iso = e.calibrate_platt(mat, groups, G, 0.1, 4), e.calibrate_isotonic(mat, groups, G, 16)
    _same_map(one.calibrate_platt(mat, groups, G, 0.1, 4), fit), _same_map(one.calibrate_isotonic(mat, groups, G, 16), iso)
    assert _same_bits(e.predict_calibrated(mat, fit, groups, G), one.predict_calibrated(mat, fit, groups, G))
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_split_train_calibrate_measure_end_to_end():
    import scipy.sparse as sp

    import fmwr_amd as fm
    rng = np.random.default_rng(13)
    n, levels = 6000, 200
    grid = np.linspace(-2.5, 2.5, levels)
    lvl = np.clip(np.rint(rng.normal(0, 1, n) * 40 + levels / 2), 0, levels - 1).astype(np.int64)
    y = (rng.random(n) < 1.0 / (1.0 + np.exp(-grid[lvl]))).astype(np.float64)
    X = sp.csr_matrix((np.ones(n), (np.arange(n), lvl)), shape=(n, levels))
    users = rng.integers(0, 3, n) * 5 + 2
    train, rest, mask = fm.fm_split(fm.fm_matrix(X, y), test_fraction=0.5, seed=3)
    fit = fm.fm_train(train, normalize=False, seed=1,
                      control=[fm.model_control("CLASSIFICATION", **{"factor.number": 2}), fm.solver_control(max_iter=500, solver=fm.SGD_solver())])
    # the planted model: twice too sure and shifted
    planted = dict(fit, Model=dict(fit["Model"], w0=0.0, w=2.0 * grid + 1.0, v=np.zeros((2, levels))))
    cal_part, eval_part, m2 = fm.fm_split(rest, test_fraction=0.5, seed=4)
    u_cal, u_eval = users[mask][~m2], users[mask][m2]
    before = fm.fm_reliability(planted, eval_part, normalize=False)
    pred = fm.predict(planted, fm.fm_matrix(X[mask][m2]), normalize=False)
    assert before["rows"].sum() == eval_part.dim[0] and abs(before["brier"][0] - np.mean((pred - y[mask][m2]) ** 2)) < 1e-12
    for method in ("platt", "isotonic"):
        cal = fm.fm_calibrate(planted, cal_part, method=method, bins=32, normalize=False)
        after = fm.fm_reliability(planted, eval_part, calibration=cal, normalize=False)
        print(method, "ECE", before["ece"][0], "->", after["ece"][0])
        assert after["ece"][0] <= before["ece"][0] and after["brier"][0] < before["brier"][0]
        pc = fm.fm_predict_calibrated(planted, fm.fm_matrix(X[mask][m2]), cal, normalize=False)
        assert abs(pc.mean() - y[mask][m2].mean()) < abs(pred.mean() - y[mask][m2].mean())
        per = fm.fm_calibrate(planted, cal_part, method=method, groups=u_cal, bins=32, normalize=False)
        assert np.array_equal(per["groups"], [2, 7, 12])
        seg = fm.fm_reliability(planted, eval_part, groups=u_eval, calibration=per, binning="mass", normalize=False)
        assert np.array_equal(seg["groups"], [2, 7, 12]) and np.array_equal(seg["rows"].sum(axis=1), [np.sum(u_eval == u) for u in (2, 7, 12)])
        assert np.all(seg["ece"] < before["ece"][0])
    fixed = fm.fm_reliability(planted, eval_part, calibration=fm.fm_prior_correction(1.0), normalize=False)
    assert _same_bits(fixed["ece"], before["ece"]) and np.array_equal(fixed["rows"], before["rows"])   # the identity map
