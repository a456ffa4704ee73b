"""The multiplier, link and loss arithmetic at saturated margins, on the device: every kernel that turns a raw score into a gradient multiplier, a
probability or a loss term, fed tests/margin_model.py's grid (the clamps, the rounding of 1 + t, the subnormals, DBL_MAX) and, in tests of their own,
+-inf and NaN -- and held to the longdouble truths and to the oracle by the bars tests/test_margin_cpu.py derives and checks on the CPU (tests/margin_cases.py: the shared builders).

The probe (margin_model.probe_matrix) gives every row its own features and a zero factor table, so y_hat is the row's stored weight in any
association and the row's multiplier can be read back: from w[3 j + 1] after one sequential step of rate 1, from GW[3 j + 1] of the exchange buffer
after fmx_grad.  Every figure is printed before it is asserted (`pytest -s`); profiles/margins.txt records a run."""
import ctypes
import functools
import time

import numpy as np
import pytest

import oracle
from tests import margin_model as mm
from tests import rows_cases as rc
from tests import margin_cases as mc
from tests import util

pytestmark = pytest.mark.gpu

LD = np.longdouble
BAR = mm.BAR
LO, HI = mc.LO, mc.HI
FP32_REL = 2.0 ** -24      # one rounding of the fp64 multiplier to the element type


def _fm():
    from fmwr_amd import engine, _lib as L
    return engine, L


def _share(err, bar):
    """the largest err / bar and where"""
    r = np.asarray(err, np.float64) / np.asarray(bar, np.float64)
    i = int(np.nanargmax(r))
    return float(r[i]), i


def _report(what, err, bar, at, t0=None):
    s, i = _share(err, bar)
    print(f"MARGINS| {what}: largest error {s:.3f} of its bar at a = {float(np.asarray(at)[i])!r}" + (f"; {time.time() - t0:.2f} s" if t0 else ""))
    return s


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ============================================================================================================ a. sequential classification
SEQ_FORMS = {"one_wave": {"FMX_SEQ_WINDOW": "0"}, "windowed": {"FMX_SEQ_WINDOW": "1"}, "pipelined": {}, "reassociated": {}}


def _seq_run(monkeypatch, form, k, y, margins=None, task=None, learn_rate=1.0, probe=None, **kw):
    """One fmx_train of n - 1 examples (rows 1 .. n - 1 once each) over the probe (of `margins`, or given); returns (w, v, probe)."""
    engine, L = _fm()
    pr = probe if probe is not None else mm.probe_matrix(margins)
    for name in ("FMX_SEQ_WINDOW", "FMX_SEQ_REASSOC"):
        monkeypatch.delenv(name, raising=False)
    for name, value in SEQ_FORMS[form].items():
        monkeypatch.setenv(name, value)
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION if task is None else task, solver=L.SOLVER_SGD, num_factor=k, keep_w0=0, learn_rate=learn_rate,
                      mode=L.MODE_SEQUENTIAL, random_step=1, seq_reassociate=int(form == "reassociated"), **kw)
    e.set_params(0.0, pr["w"], np.zeros((k, pr["p"])) if k else None)
    m = engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], np.asarray(y, np.float32))
    assert e.train(m, pr["n"] - 1) == pr["n"] - 1
    _, w, v = e.get_params()
    e.close(); m.close()
    return w, v, pr


@functools.lru_cache(maxsize=None)
def _oracle_cls(k, labels):
    a = mc.probe_margins()
    y = mc.label_sets(len(a))[labels]
    mult, ref, _ = mc.oracle_probe(k, y)
    return a, y, mult, ref


@pytest.mark.parametrize("form", list(SEQ_FORMS))
@pytest.mark.parametrize("labels", ["plus", "minus", "alternating"])
@pytest.mark.parametrize("k", [0, 8])
def test_sequential_classification_multiplier(monkeypatch, k, labels, form):
    t0 = time.time()
    a, y, omult, ref = _oracle_cls(k, labels)
    w, v, pr = _seq_run(monkeypatch, form, k, y, a)
    mult = -w[1::3]
    truth = mm.mult_cls(a, y)
    assert mult[0] == 0.0 and w[0] == a[0]                                   # row 0 is never visited (SURVEY A-2)
    a, y, mult, omult, truth = a[1:], y[1:], mult[1:], omult[1:], truth[1:]
    err = np.abs(mult.astype(LD) - truth).astype(np.float64)
    _report(f"seq {form} k={k} {labels} |mult - truth|", err, BAR, a, t0)
    assert np.all(err <= BAR)
    d = np.abs(mult - omult)
    obar = mm.RE_ABS_TO_ORACLE if form == "reassociated" else BAR
    _report(f"seq {form} k={k} {labels} |mult - oracle|", d, obar, a)
    assert np.all(d <= obar)
    # nothing else moved: w[3 j] by the plain formulas on the row's own multiplier, the free columns and every factor row still zero
    assert np.array_equal(w[0::3][1:], mc.plain_update(a, mult)) and np.all(w[2::3] == 0.0) and np.all(v == 0.0)
    if form == "reassociated":
        keep = (np.abs(a) <= 700.0) & (np.abs(truth) >= LD(2.0) ** -1000)
        u = np.where(keep, mm.ulp_error(mult, truth), 0.0)
        i = int(np.argmax(u))
        model_ulp = mm.re_model_max_ulp()[0]
        print(f"MARGINS| seq reassociated k={k} {labels}: largest relative error {u[i]:.3f} ulp at a = {a[i]!r}, y = {y[i]:+.0f} (model {model_ulp:.3f} ulp)")
        assert u[i] <= model_ulp + 1.0
        # the reassociated kernel really ran: its multiplier is not the bitwise kernels' in every bit (their exp and division are the library's)
        wp, _, _ = _seq_run(monkeypatch, "pipelined", k, mc.label_sets(len(a) + 1)[labels], mc.probe_margins())
        assert not np.array_equal(mult, -wp[1::3][1:])


def _own(pr, rows):
    m = np.zeros(pr["p"], bool)
    for r in rows:
        m[3 * r:3 * r + 3] = True
    return m


@pytest.mark.parametrize("form", list(SEQ_FORMS))
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_sequential_non_finite_margins(monkeypatch, form, sign):
    """Margins of +inf, -inf and NaN (from finite parameters: margin_model.NONFINITE_ROWS) in the middle of ordinary rows."""
    pa, rows = mc.nonfinite_probe(True)
    pb, _ = mc.nonfinite_probe(False)
    y = np.full(pa["n"], sign)
    w, v, _ = _seq_run(monkeypatch, form, 8, y, probe=pa)
    wb, vb, _ = _seq_run(monkeypatch, form, 8, y, probe=pb)
    mult = -w[1::3]
    pos, neg, nan = (rows[0], rows[1], rows[2]) if sign > 0 else (rows[1], rows[0], rows[2])
    # y a = +inf: the limit 0 (the reassociated form clamps at 700: 1 / (1 + e^700) = 9.9e-305); y a = -inf: -y exactly; NaN: NaN
    assert abs(mult[pos]) <= (1e-304 if form == "reassociated" else 0.0) and mult[neg] == -sign and np.isnan(mult[nan])
    own = _own(pa, rows)
    assert _same_bits(w[~own], wb[~own]) and _same_bits(v[:, ~own], vb[:, ~own])          # every other row: every bit as without them
    mine = _own(pa, [nan])
    assert np.isnan(w[mine]).all() and not np.isnan(w[~mine]).any()                          # NaN in the NaN row's own features only
    ref = mc.oracle_probe(8, y, probe=pa)[1]
    assert np.array_equal(np.isnan(v), np.isnan(ref["v"].reshape(8, pa["p"]))) and np.isnan(v[:, mine]).all() and not np.isnan(v[:, ~mine]).any()


# ============================================================================================================ b. the grid launcher
def test_grid_training_gives_each_engines_own_bits(monkeypatch):
    engine, L = _fm()
    a, y, _, _ = _oracle_cls(8, "alternating")
    rates = (1.0, 0.5)
    singles = [_seq_run(monkeypatch, "pipelined", 8, y, a, learn_rate=lr) for lr in rates]
    pr = singles[0][2]
    es = [engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=8, keep_w0=0, learn_rate=lr, mode=L.MODE_SEQUENTIAL, random_step=1)
          for lr in rates]
    for e in es:
        e.set_params(0.0, pr["w"], np.zeros((8, pr["p"])))
    m = engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], y.astype(np.float32))
    assert engine.Engine.train_grid(es, m, pr["n"] - 1) == pr["n"] - 1
    for e, (w, v, _) in zip(es, singles):
        _, gw, gv = e.get_params()
        assert _same_bits(gw, w) and _same_bits(gv, v)
        e.close()
    assert not np.array_equal(singles[0][0], singles[1][0])
    m.close()


# ============================================================================================================ c. mini-batch mode
MB_ENGINES = {"f64_k8": (8, True, None), "f32_k8": (8, False, None), "f32_k12": (12, False, None), "f32_k16": (16, False, "0"), "f32_k16_wir": (16, False, "1")}
MB_EMBED = {"f64_k8": "none", "f32_k8": "none", "f32_k12": "pad", "f32_k16": "bits", "f32_k16_wir": "bits"}
MB_FORMS = ["narrow4", "narrow1", "wide", "wide_pull", "wide_flat"]


def _grid(fp64):
    """MARGINS as an engine's tables can hold them as finite weights: all of it in fp64; in fp32 the values whose float rounding is finite (+-1e300
    and +-DBL_MAX are no floats; 2^-1074, 2^-1022 and 2^-60.. round to zero or stay: they are kept, the truth is taken at the value read back)."""
    if fp64:
        return mm.MARGINS
    with np.errstate(over="ignore"):
        return mm.MARGINS[np.isfinite(mm.MARGINS.astype(np.float32))]


def _mb_rows(form, k, fp64):
    """The smallest row count >= the grid's that lands a pointwise step in the form (rows_cases.static_form restates the launcher's rule)."""
    lpr = rc.lanes(k, fp64)
    n = len(_grid(fp64))
    rows = {"narrow4": n, "narrow1": max(n, 1024 * 64 // lpr)}.get(form, max(n, 512 * 256 // lpr))
    want = {"narrow4": rc.NARROW4, "narrow1": rc.NARROW1}.get(form, "wide")
    assert rc.static_form(rows, lpr) == want and (rows == n or rc.static_form(rows - 1, lpr) != want)
    return rows


def _ragged(pr, every=5):
    """The probe with column 3 j + 2 (weight 0, x = 1) added to every fifth row: rows of two lengths, which the pull and the flat kernel need;
    y_hat is still the row's weight exactly."""
    T = pr["n"]
    lens = np.where(np.arange(T) % every == 0, 3, 2)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([3 * j + np.arange(lens[j]) for j in range(T)]).astype(np.uint32)
    return dict(pr, rp=rp, col=col, val=np.ones(len(col), np.float32))


def _mb_engine(monkeypatch, name, p, rows, task, reduce=None, solver=None, **kw):
    engine, L = _fm()
    k, fp64, wir = MB_ENGINES[name]
    monkeypatch.delenv("FMX_W_IN_ROW", raising=False)
    if wir is not None:
        monkeypatch.setenv("FMX_W_IN_ROW", wir)      # read at engine creation
    e = engine.Engine(p, task=task, solver=L.SOLVER_SGD if solver is None else solver, num_factor=k, keep_w0=0, learn_rate=1.0, mode=L.MODE_MINIBATCH,
                      batch_rows=rows, state_fp64=int(fp64), batch_reduce=L.REDUCE_MEAN if reduce is None else reduce, **kw)
    if wir is not None:
        assert e.w_in_row() == (wir == "1")
    return e


def _cols_counter(L):
    a = (ctypes.c_int64 * 3)()
    L.check(L.lib().fmx_debug_cols_launches(a))
    return np.array(list(a), np.int64)


def _set_rows_variant(monkeypatch, form):
    for name in ("FMX_ROWS_PULL", "FMX_ROWS_FLAT"):
        monkeypatch.delenv(name, raising=False)
    if form == "wide_pull":
        monkeypatch.setenv("FMX_ROWS_PULL", "1")
    elif form == "wide_flat":
        monkeypatch.setenv("FMX_ROWS_FLAT", "1")


def _check_form(form, launches):
    slots = {"narrow4": [rc.NARROW4], "narrow1": [rc.NARROW1], "wide": [rc.WIDE_SERIAL, rc.WIDE_PIPELINED], "wide_pull": [rc.PULL], "wide_flat": [rc.FLAT]}[form]
    assert launches[slots].sum() >= 1 and launches.sum() == launches[slots].sum(), (form, [rc.FORM_NAMES[i] for i in np.nonzero(launches)[0]])


def _mb_grad(monkeypatch, name, form, pr, y, task, reduce=None, step=True, **kw):
    """fmx_grad on the probe as ONE step; returns (planes of the exchange buffer, weights as the engine holds them, w after one fmx_step or None)."""
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    e = _mb_engine(monkeypatch, name, pr["p"], pr["n"], task, reduce, **kw)
    with np.errstate(over="ignore"):
        e.set_params(0.0, pr["w"], np.zeros((k, pr["p"])))
    held = e.get_params()[1]
    m = engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], np.asarray(y, np.float32))
    _set_rows_variant(monkeypatch, form)
    before = rc._counter(L)
    e.grad(m, 0)
    buf = rc._read_buffer(e, util)
    _check_form(form, rc._counter(L) - before)
    planes = rc.split_buffer(buf, e.grad_layout(), pr["p"], rc.padded(k, fp64), k, False)
    planes = {key: np.array(val) for key, val in planes.items()}
    w1 = None
    if step:
        cols = _cols_counter(L)
        e.step(m, 0)
        w1 = e.get_params()[1]
        cols = _cols_counter(L) - cols
        if MB_EMBED[name] != "none":
            assert cols[1] + cols[2] >= 1 and cols[0] == 0, (name, cols)   # the multiplier came back out of the S rows through fm_cols_lean_k
    e.close(); m.close()
    return planes, held, w1


def _fp_bar(truth, fp64):
    t = np.abs(np.asarray(truth, LD)).astype(np.float64)
    return np.full(len(t), BAR) if fp64 else FP32_REL * t + BAR


@pytest.mark.parametrize("form", MB_FORMS)
@pytest.mark.parametrize("name", list(MB_ENGINES))
def test_minibatch_classification_multiplier(monkeypatch, name, form):
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    rows = _mb_rows(form, k, fp64)
    grid = _grid(fp64)
    assert len(grid) == len(mm.MARGINS) - (0 if fp64 else 4) and len(grid) % 2 == 0
    a = np.resize(grid, rows)
    y = np.where((np.arange(rows) // 2) % 2 == 0, 1.0, -1.0)     # the grid alternates a, -a: one label per pair gives every magnitude both signs of y a
    pr = mm.probe_matrix(a)
    if form in ("wide_pull", "wide_flat"):
        pr = _ragged(pr)
    for reduce in (L.REDUCE_MEAN, L.REDUCE_SUM):
        t0 = time.time()
        planes, held, w1 = _mb_grad(monkeypatch, name, form, pr, y, L.TASK_CLASSIFICATION, reduce)
        gw = np.asarray(planes["Gw"], np.float64)
        back = held[0::3]                                # fp32 tables: the margin's float rounding
        assert np.array_equal(back, a if fp64 else a.astype(np.float32).astype(np.float64)) and np.isfinite(back).all()
        truth = mm.mult_cls(back, y)
        mult = gw[1::3]
        err = np.abs(mult.astype(LD) - truth).astype(np.float64)
        bar = _fp_bar(truth, fp64)
        _report(f"mb {name} {form} {'mean' if reduce == L.REDUCE_MEAN else 'sum'} ({rows} rows) |GW - truth|", err, bar, back, t0)
        assert np.all(err <= bar)
        if fp64:
            P = oracle.params()
            om = np.array([oracle.grad_mult(P, float(ai), float(yi))[0] for ai, yi in zip(a[:2 * len(grid)], y[:2 * len(grid)])])   # (two copies of the grid: every (a, y))
            assert np.all(np.abs(mult - np.resize(om, rows)) <= BAR)
        assert _same_bits(gw[0::3], mult)                                                    # the row's other feature: the same one term
        extra = np.asarray(pr["rp"][1:] - pr["rp"][:-1]) == 3
        assert _same_bits(gw[2::3][extra], mult[extra]) and np.all(gw[2::3][~extra] == 0.0) and np.all(planes["Gv"] == 0.0)
        assert np.array_equal(np.asarray(planes["cw"], np.float64)[1::3], np.ones(rows))
        # one step of rate 1 without decay: w = 0 - GW, exactly, in the state type -- the multiplier after its trip through the S rows' embedded bits
        assert np.array_equal(w1[1::3], -mult)


@pytest.mark.parametrize("name", ["f64_k8", "f32_k8", "f32_k12", "f32_k16"])
def test_minibatch_non_finite_margins(monkeypatch, name):
    """fp64 tables: margins of +inf, -inf and NaN from finite parameters.  fp32 tables cannot overflow the forward's fp64 sums from finite
    parameters: there the NaN margin comes from a NaN weight and rides through the S rows' embedded bits."""
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    pb, rows = mc.nonfinite_probe(False)
    if fp64:
        pa, _ = mc.nonfinite_probe(True)
    else:
        before, after = mm.MARGINS[:80:2], mm.MARGINS[1200:1280:3]
        pa = mm.probe_rows([mm.point_row(0.25)] + [mm.point_row(a) for a in before] + [mm.point_row(0.5)] * 2 + [mm.NAN_WEIGHT_ROW] + [mm.point_row(a) for a in after])
    for sign in (1.0, -1.0):
        y = np.full(pa["n"], sign)
        ga, _, wa = _mb_grad(monkeypatch, name, "narrow4", pa, y, L.TASK_CLASSIFICATION)
        gb, _, wb = _mb_grad(monkeypatch, name, "narrow4", pb, y, L.TASK_CLASSIFICATION)
        mult = np.asarray(ga["Gw"], np.float64)[1::3]
        pos, neg, nan = (rows[0], rows[1], rows[2]) if sign > 0 else (rows[1], rows[0], rows[2])
        assert np.isnan(mult[nan]) and np.isnan(wa[3 * nan + 1])                              # NaN stays NaN, also through the embedded bits
        if fp64:
            assert mult[pos] == 0.0 and mult[neg] == -sign and wa[3 * neg + 1] == sign and wa[3 * pos + 1] == 0.0
        own = _own(pa, rows)
        assert _same_bits(ga["Gw"][~own], gb["Gw"][~own]) and _same_bits(ga["Gv"][:, ~own], gb["Gv"][:, ~own]) and _same_bits(wa[~own], wb[~own])
        mine = _own(pa, [nan])
        assert np.isnan(ga["Gw"][mine]).all() and not np.isnan(ga["Gw"][~mine]).any() and not np.isnan(ga["Gv"][:, ~mine]).any()
        assert np.isnan(wa[mine]).all() and not np.isnan(wa[~mine]).any()


# ---- the scheduled form's shape: a 262 144-row tile over a V table above 32 MB.  FMX_ROWS_SCHED is read once per process: two child processes.
SCHED_ROWS = 262144

_SCHED_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import margin_model as mm, rows_cases as rc, test_gpu_margins as g, util
out = sys.argv[1]
a, y = g._sched_problem()
pr = mm.probe_matrix(a)
def counters():
    s, m = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 2)()
    L.check(L.lib().fmx_debug_rows_sched_launches(s)); L.check(L.lib().fmx_debug_rows_merged_launches(m))
    return np.array(list(s) + list(m), np.int64)
os.environ["FMX_W_IN_ROW"] = "0"
e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=16, keep_w0=0, learn_rate=1.0, mode=L.MODE_MINIBATCH, batch_rows=g.SCHED_ROWS)
e.set_params(0.0, pr["w"], np.zeros((16, pr["p"])))
held = e.get_params()[1][0::3]
m = engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], y.astype(np.float32))
c0 = counters()
e.grad(m, 0)
buf = rc._read_buffer(e, util)
c1 = counters() - c0
planes = rc.split_buffer(buf, e.grad_layout(), pr["p"], 16, 16, False)
np.savez(os.path.join(out, "sched.npz"), gw=np.array(planes["Gw"]), gv_zero=np.bool_(np.all(planes["Gv"] == 0)), held=held, count=c1)
print("DONE")
"""


def _sched_problem():
    """the fp32 grid tiled over the rows in a fixed permutation, one label per consecutive pair of rows"""
    grid = _grid(False)
    a = np.resize(grid, SCHED_ROWS)[np.random.default_rng(262144).permutation(SCHED_ROWS)]
    return a, np.where((np.arange(SCHED_ROWS) // 2) % 2 == 0, 1.0, -1.0)


def test_minibatch_multiplier_at_the_scheduled_forms_shape(tmp_path):
    """fp32 state, k = 16, 262 144 rows, p = 3 x 262 144 (a 50 MB V table): the launcher's own rule sends the step to the scheduled form; the same
    step under FMX_ROWS_SCHED=0 goes to the merged form and must give the same GW in every bit."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for name, env in (("sched", {}), ("merged", {"FMX_ROWS_SCHED": "0"})):
        d = tmp_path / name
        d.mkdir()
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        r = subprocess.run([sys.executable, "-c", _SCHED_CHILD, str(d)], env=child_env, cwd=root, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "DONE" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        res[name] = dict(np.load(d / "sched.npz"))
    sc, mg = res["sched"]["count"], res["merged"]["count"]        # [scheduled, turned away, schedules built | merged, merged turned away]
    assert sc[0] == 1 and sc[1] == 0 and sc[3] == 0, sc
    assert mg[0] == 0 and mg[3] == 1, mg
    a, y = _sched_problem()
    back = res["sched"]["held"]
    assert np.array_equal(back, a.astype(np.float32).astype(np.float64))
    gw = np.asarray(res["sched"]["gw"], np.float64)
    truth = mm.mult_cls(back, y)
    err = np.abs(gw[1::3].astype(LD) - truth).astype(np.float64)
    bar = _fp_bar(truth, False)
    _report(f"mb f32_k16 scheduled ({SCHED_ROWS} rows) |GW - truth|", err, bar, back)
    assert np.all(err <= bar) and _same_bits(gw[0::3], gw[1::3]) and np.all(gw[2::3] == 0.0) and bool(res["sched"]["gv_zero"])
    assert _same_bits(res["sched"]["gw"], res["merged"]["gw"]) and bool(res["merged"]["gv_zero"])


# ============================================================================================================ d. ranking
@pytest.mark.parametrize("name", ["f64_k8", "f32_k8", "f32_k12", "f32_k16"])
def test_ranking_multiplier_and_pair_metrics(monkeypatch, name):
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    d = _grid(fp64)
    pr = mm.probe_matrix(d, "pair")
    t0 = time.time()
    e = _mb_engine(monkeypatch, name, pr["p"], pr["n"], L.TASK_RANKING)
    with np.errstate(over="ignore"):
        e.set_params(0.0, pr["w"], np.zeros((k, pr["p"])))
    back = e.get_params()[1][0::3]
    m = engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], np.ones(pr["n"], np.float32))
    e.grad(m, 0)
    planes = rc.split_buffer(rc._read_buffer(e, util), e.grad_layout(), pr["p"], rc.padded(k, fp64), k, False)
    gw = np.asarray(planes["Gw"], np.float64)
    m0, m1 = gw[1::3], gw[2::3]
    truth = mm.mult_bpr(back)
    err = np.abs(m0.astype(LD) - truth).astype(np.float64)
    bar = _fp_bar(truth, fp64)
    _report(f"ranking {name} |m0 - mult_bpr(d)|", err, bar, back, t0)
    assert np.all(err <= bar)
    assert np.array_equal(m1, -m0) and _same_bits(gw[0::3], m0)                      # the pair's other row: the exact negation
    # the pair accuracy over the whole grid, exactly: [d > 0] + 1/2 [d == 0], the exact count divided once
    acc = float(np.sum(np.where(back > 0, 1.0, np.where(back == 0, 0.5, 0.0)))) / len(back)
    assert e.evaluate(m, L.EVAL_PAIR_ACC) == acc and (back == 0).sum() >= 2
    e.step(m, 0)
    w1 = e.get_params()[1]
    assert np.array_equal(w1[1::3], -m0) and np.array_equal(w1[2::3], m0)            # and after the trip through the S rows
    e.close(); m.close()
    # the BPR loss over the grid without +-DBL_MAX: the loss at -DBL_MAX is DBL_MAX, and a double sum that holds it beside 1e300 overflows
    keep = np.abs(d) < mm.DBL_MAX
    pe = mm.probe_matrix(d[keep], "pair")
    e = _mb_engine(monkeypatch, name, pe["p"], pe["n"], L.TASK_RANKING)
    e.set_params(0.0, pe["w"], np.zeros((k, pe["p"])))
    dd = e.get_params()[1][0::3]
    assert keep.sum() >= len(d) - 2 and (dd > 700).any() and (dd < -700).any()
    m = engine.Matrix.from_csr(pe["rp"], pe["col"], pe["val"], pe["p"], np.ones(pe["n"], np.float32))
    want = float(np.sum(mm.bpr_loss(dd)) / LD(len(dd)))
    got = e.evaluate(m, L.EVAL_BPR)
    print(f"MARGINS| ranking {name} BPR loss: |got - want| = {abs(got - want) / (1e-12 * max(1.0, want)):.3f} of its bar")
    assert abs(got - want) <= 1e-12 * max(1.0, want)
    e.close(); m.close()


# ============================================================================================================ e. regression
def _reg_want(pr, preds, labels, held):
    """mult_reg at the prediction every row really has: the weight as the engine holds it (its float rounding in fp32 tables) for a finite
    prediction, the non-finite value itself for the rows built to overflow"""
    eff = np.where(np.isfinite(preds), held[0::3][:len(preds)], preds)
    return np.array([mm.mult_reg(p, y, LO, HI) for p, y in zip(eff, labels)])


@pytest.mark.parametrize("form", list(SEQ_FORMS))
def test_sequential_regression_multiplier_is_the_oracles_in_every_bit(monkeypatch, form):
    """No transcendental is involved: every bit.  The NaN prediction leaves std::min(max_target, NaN) = max_target, so its row gets max_target - y
    (tests/test_margin_cpu.py holds that rule to the C++ library itself)."""
    engine, L = _fm()
    pr, preds, y = mc.reg_probe(False)
    w, v, _ = _seq_run(monkeypatch, form, 8, y, probe=pr, task=L.TASK_REGRESSION, min_target=LO, max_target=HI)
    want = _reg_want(pr, preds, y, pr["w"])
    omult = mc.oracle_probe(8, y, probe=pr, task=oracle.REGRESSION, min_target=LO, max_target=HI)[0]
    assert _same_bits(omult[1:], want[1:])
    got = -w[1::3]
    bad = [(float(preds[i]), float(y[i]), float(got[i]), float(want[i])) for i in range(1, len(preds)) if got[i] != want[i]]
    assert not bad, bad
    assert np.isnan(preds).sum() == 4 and not np.isnan(got).any()


# every engine in the smallest form, the other forms on one fp64 and one fp32 engine
REG_MB = [(name, "narrow4") for name in MB_ENGINES] + [(name, form) for name in ("f64_k8", "f32_k16") for form in MB_FORMS[1:]]


@pytest.mark.parametrize("name,form", REG_MB)
def test_minibatch_regression_multiplier_is_the_oracles_after_one_rounding(monkeypatch, name, form):
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    pr0, preds0, y0 = mc.reg_probe(not fp64)
    lpr = rc.lanes(k, fp64)
    rows = max(pr0["n"], {"narrow4": 0, "narrow1": 1024 * 64 // lpr}.get(form, 512 * 256 // lpr))
    reps = -(-rows // pr0["n"])
    rows = reps * pr0["n"]                                # whole copies of the case list (rows of three entries among them: the pull and flat forms' ragged rows)
    assert rc.static_form(rows, lpr) == {"narrow4": rc.NARROW4, "narrow1": rc.NARROW1}.get(form, "wide")
    pr = dict(rp=np.concatenate([[0]] + [pr0["rp"][1:] + i * pr0["rp"][-1] for i in range(reps)]).astype(np.int64),
              col=np.concatenate([pr0["col"] + np.uint32(i * pr0["p"]) for i in range(reps)]).astype(np.uint32), val=np.tile(pr0["val"], reps),
              w=np.tile(pr0["w"], reps), p=reps * pr0["p"], n=rows)
    preds, y = np.tile(preds0, reps), np.tile(y0, reps)
    planes, held, w1 = _mb_grad(monkeypatch, name, form, pr, y, L.TASK_REGRESSION, min_target=LO, max_target=HI)
    want = _reg_want(pr, preds, y, held)
    if not fp64:
        want = want.astype(np.float32).astype(np.float64)
    got = np.asarray(planes["Gw"], np.float64)[1::3]
    bad = [(float(preds[i]), float(y[i]), float(got[i]), float(want[i])) for i in range(pr0["n"]) if got[i] != want[i]]
    assert not bad, bad
    assert np.array_equal(got, want) and np.array_equal(w1[1::3], -want) and np.isnan(preds).any()


# ============================================================================================================ f. FTRL and TDAP
def _ftrl_probe():
    """a spare row 0, MARGINS, and the three non-finite margins from finite parameters"""
    rows = [mm.point_row(0.25)] + [mm.point_row(a) for a in mm.MARGINS] + mm.NONFINITE_ROWS
    pr = mm.probe_rows(rows)
    return pr, np.where(((np.arange(pr["n"]) + 1) // 2) % 2 == 0, 1.0, -1.0)   # one label per (a, -a) pair of rows 1 ..: both signs of y a at every magnitude


def _hold_elementwise(got, ref, tol, what):
    """the solvers' existing bars (tests/test_gpu_train.py: 1e-11), taken per ELEMENT -- a table that holds 1e300 beside 0.03 has no useful norm --
    with NaN exactly where the oracle has NaN and an infinite value equal to the oracle's"""
    got, ref = np.asarray(got, np.float64).ravel(), np.asarray(ref, np.float64).ravel()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.nonzero(np.isnan(got) != np.isnan(ref))[0][:10])
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what
    ok = np.isfinite(ref)
    err = np.abs(got[ok] - ref[ok]) / np.maximum(1.0, np.abs(ref[ok]))
    i = int(np.argmax(err))
    print(f"MARGINS| {what}: largest elementwise error {err[i] / tol:.3f} of its bar")
    assert err[i] <= tol, (what, float(got[ok][i]), float(ref[ok][i]))


@pytest.mark.parametrize("form", ["one_wave", "windowed", "pipelined"])
def test_sequential_ftrl_on_the_probe_matches_the_oracle(monkeypatch, form):
    """FTRL at its default hyper-parameters, one pass: its first forward of a row reads the stored weight, so every margin of the grid is reached;
    a saturated margin makes g = 0 exactly, hence n = 0 and sigma = 0."""
    engine, L = _fm()
    pr, y = _ftrl_probe()
    P = oracle.params(k=8, k0=False)
    X = oracle.Matrix(pr["rp"], pr["col"], pr["val"], pr["p"])
    with np.errstate(all="ignore"):
        ref = oracle.ftrl_learn(P, X, y.astype(np.float32), 0.0, pr["w"], np.zeros(8 * pr["p"]), pr["n"] - 1)
    assert (ref["w"][1::3] == 0.0).sum() > 40 and np.isnan(ref["w"]).any()          # saturated rows: g = 0 left w = 0; the NaN row left NaN
    for name in ("FMX_SEQ_WINDOW", "FMX_SEQ_REASSOC"):
        monkeypatch.delenv(name, raising=False)
    for name, value in SEQ_FORMS[form].items():
        monkeypatch.setenv(name, value)
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_FTRL, num_factor=8, keep_w0=0, mode=L.MODE_SEQUENTIAL, random_step=1)
    e.set_params(0.0, pr["w"], np.zeros((8, pr["p"])))
    m = _matrix(pr, y)
    assert e.train(m, pr["n"] - 1) == pr["n"] - 1
    _, w, v = e.get_params()
    _hold_elementwise(w, ref["w"], 1e-11, f"seq ftrl {form} w")
    _hold_elementwise(v, ref["v"].reshape(8, pr["p"]), 1e-11, f"seq ftrl {form} v")
    e.close(); m.close()


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_minibatch_ftrl_on_the_probe_matches_the_oracle(reduce):
    engine, L = _fm()
    pr, y = _ftrl_probe()
    P = oracle.params(k=8, k0=False, batch_mean=(reduce == "mean"))
    X = oracle.Matrix(pr["rp"], pr["col"], pr["val"], pr["p"])
    mb = oracle.FtrlMinibatch(P, X, y, 0.0, pr["w"], np.zeros(8 * pr["p"]))
    with np.errstate(all="ignore"):
        mb.step(0, pr["n"])
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_FTRL, num_factor=8, keep_w0=0, mode=L.MODE_MINIBATCH, state_fp64=1, batch_rows=pr["n"],
                      batch_reduce=L.REDUCE_MEAN if reduce == "mean" else L.REDUCE_SUM)
    e.set_params(0.0, pr["w"], np.zeros((8, pr["p"])))
    m = _matrix(pr, y)
    e.step(m, 0)
    _, w, v = e.get_params()
    assert (mb.w[1::3] == 0.0).sum() > 40 and np.isnan(mb.w).any()
    _hold_elementwise(w, mb.w, 1e-11, f"mb64 ftrl {reduce} w")
    _hold_elementwise(v, mb.v.reshape(8, pr["p"]), 1e-11, f"mb64 ftrl {reduce} v")
    e.close(); m.close()


def _tdap_oracle_params(**kw):
    return oracle.params(k=8, k0=False, **kw)     # the solver's defaults: alpha 0.1, gamma 1e-4, no l1 / l2


@pytest.mark.parametrize("form", ["one_wave", "windowed", "pipelined"])
def test_sequential_tdap_on_the_probe_matches_the_oracle(monkeypatch, form):
    """TDAP at its default hyper-parameters, one pass.  Like FTRL it forwards the stored parameters and takes the multiplier before it touches any
    state, and every row is visited once: row j's forward reads w[3 j] = a_j.  A saturated margin makes g = 0, so u = 0 and delta = 0: the solver's
    own -z / delta = 0 / 0 is reached, and NaN must stand exactly where the oracle has it.  Bar: the solver's existing 1e-10, per element."""
    engine, L = _fm()
    pr, y = _ftrl_probe()
    P = _tdap_oracle_params()
    X = oracle.Matrix(pr["rp"], pr["col"], pr["val"], pr["p"])
    with np.errstate(all="ignore"):
        ref = oracle.tdap_learn(P, X, y.astype(np.float32), 0.0, pr["w"], np.zeros(8 * pr["p"]), pr["n"] - 1)
    for name in ("FMX_SEQ_WINDOW", "FMX_SEQ_REASSOC"):
        monkeypatch.delenv(name, raising=False)
    for name, value in SEQ_FORMS[form].items():
        monkeypatch.setenv(name, value)
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_TDAP, num_factor=8, keep_w0=0, mode=L.MODE_SEQUENTIAL, random_step=1)
    e.set_params(0.0, pr["w"], np.zeros((8, pr["p"])))
    m = _matrix(pr, y)
    assert e.train(m, pr["n"] - 1) == pr["n"] - 1
    _, w, v = e.get_params()
    print(f"MARGINS| seq tdap {form}: oracle w holds {int(np.isnan(ref['w']).sum())} NaN, {int((ref['w'] == 0).sum())} zeros of {pr['p']}")
    _hold_elementwise(w, ref["w"], 1e-10, f"seq tdap {form} w")
    _hold_elementwise(v, ref["v"].reshape(8, pr["p"]), 1e-10, f"seq tdap {form} v")
    e.close(); m.close()


@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_minibatch_tdap_on_the_probe_matches_the_oracle(reduce):
    engine, L = _fm()
    pr, y = _ftrl_probe()
    P = _tdap_oracle_params(batch_mean=(reduce == "mean"))
    X = oracle.Matrix(pr["rp"], pr["col"], pr["val"], pr["p"])
    mb = oracle.TdapMinibatch(P, X, y, 0.0, pr["w"], np.zeros(8 * pr["p"]))
    with np.errstate(all="ignore"):
        mb.step(0, pr["n"])
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_TDAP, num_factor=8, keep_w0=0, mode=L.MODE_MINIBATCH, state_fp64=1, batch_rows=pr["n"],
                      batch_reduce=L.REDUCE_MEAN if reduce == "mean" else L.REDUCE_SUM)
    e.set_params(0.0, pr["w"], np.zeros((8, pr["p"])))
    m = _matrix(pr, y)
    e.step(m, 0)
    _, w, v = e.get_params()
    print(f"MARGINS| mb64 tdap {reduce}: oracle w holds {int(np.isnan(mb.w).sum())} NaN, {int((mb.w == 0).sum())} zeros of {pr['p']}")
    _hold_elementwise(w, mb.w, 1e-11, f"mb64 tdap {reduce} w")
    _hold_elementwise(v, mb.v.reshape(8, pr["p"]), 1e-11, f"mb64 tdap {reduce} v")
    e.close(); m.close()


# ============================================================================================================ an infinite PARAMETER
# The mini-batch forward (fm_rows_forward_k, its pull and flat siblings) pads a short gather round with (the round's first column, x = +0): the loads
# stay unconditional and the hot loop straight-line.  An infinite weight in that column then meets 0 x inf = NaN, where the
# reference's forward gives +-inf.  The divergence is documented, not fixed; these tests pin what the device gives, so that it cannot change unseen:
#   one lane group per row (narrow1, wide):   infinite weight in the row's FIRST column -> y_hat NaN;  in a later column -> +-inf, the reference's value
#   four lane groups per row (narrow4):       each group pads with its own first entry: a two-entry row is NaN wherever the infinite weight stands
#   never: a finite value, or any change to another row.
def _inf_rows(inf_on):
    first = lambda v: [(v, 1.0), (0.0, 1.0)]
    second = lambda v: [(0.0, 1.0), (v, 1.0)]
    inf = float("inf")
    special = [first(inf), second(inf), first(-inf), second(-inf)] if inf_on else [mm.point_row(0.5)] * 4
    return [mm.point_row(0.25)] + [mm.point_row(a) for a in mm.MARGINS[100:140:2]] + special + [mm.point_row(a) for a in mm.MARGINS[200:230:3]], np.arange(21, 25)


def _inf_expected(split4):
    """y_hat of the four special rows (inf first, inf second, -inf first, -inf second)"""
    nan, inf = float("nan"), float("inf")
    return np.array([nan, nan, nan, nan]) if split4 else np.array([nan, inf, nan, -inf])


@pytest.mark.parametrize("form", ["narrow4", "narrow1", "wide"])
@pytest.mark.parametrize("name", ["f64_k8", "f32_k16"])
def test_an_infinite_weight_in_the_minibatch_gradient(monkeypatch, name, form):
    engine, L = _fm()
    k, fp64, _ = MB_ENGINES[name]
    lpr = rc.lanes(k, fp64)
    rows_a, special = _inf_rows(True)
    rows_b, _ = _inf_rows(False)
    total = max(len(rows_a), {"narrow4": 0, "narrow1": 1024 * 64 // lpr}.get(form, 512 * 256 // lpr))
    fill = [mm.point_row(a) for a in np.resize(_grid(fp64), total - len(rows_a))]
    pa, pb = mm.probe_rows(rows_a + fill), mm.probe_rows(rows_b + fill)
    y = np.ones(total)
    ga, _, wa = _mb_grad(monkeypatch, name, form, pa, y, L.TASK_CLASSIFICATION)
    gb, _, wb = _mb_grad(monkeypatch, name, form, pb, y, L.TASK_CLASSIFICATION)
    yh = _inf_expected(form == "narrow4")
    with np.errstate(all="ignore"):
        want = mm.mult_cls(yh, np.ones(4)).astype(np.float64)          # y = +1: +inf -> -0, -inf -> -1, NaN -> NaN
    got = np.asarray(ga["Gw"], np.float64)
    mult = np.array([got[3 * r + (1 if i % 2 == 0 else 0)] for i, r in enumerate(special)])    # read at the row's finite-weight feature
    print(f"MARGINS| infinite weight, grad {name} {form}: multipliers {mult.tolist()} (expected {want.tolist()})")
    assert np.array_equal(mult, want, equal_nan=True)
    own = _own(pa, special)
    assert _same_bits(ga["Gw"][~own], gb["Gw"][~own]) and _same_bits(ga["Gv"][:, ~own], gb["Gv"][:, ~own]) and _same_bits(wa[~own], wb[~own])


@pytest.mark.parametrize("kind", ["seq64", "mb64", "mb32"])
def test_an_infinite_weight_in_predict(kind):
    """fmx_predict over few rows takes the four-lane-group form: NaN wherever the infinite weight stands; every other row unchanged in every bit."""
    engine, L = _fm()
    c = LINK_ENGINES[kind]
    out = []
    for inf_on in (True, False):
        rows, special = _inf_rows(inf_on)
        pr = mm.probe_rows(rows)
        e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=4, keep_w0=0,
                          mode=L.MODE_SEQUENTIAL if c["mode"] == "seq" else L.MODE_MINIBATCH, state_fp64=int(c["fp64"] and c["mode"] == "mb"))
        e.set_params(0.0, pr["w"], np.zeros((4, pr["p"])))
        m = _matrix(pr)
        out.append((e.predict(m), e.predict(m, L.LINK_LOGISTIC)))
        e.close(); m.close()
    (ra, la), (rb, lb) = out
    print(f"MARGINS| infinite weight, predict {kind}: raw {ra[special].tolist()} logistic {la[special].tolist()}")
    assert np.array_equal(ra[special], _inf_expected(True), equal_nan=True) and np.isnan(la[special]).all()
    other = np.ones(len(ra), bool)
    other[special] = False
    assert _same_bits(ra[other], rb[other]) and _same_bits(la[other], lb[other])


# ============================================================================================================ g. links
LINK_ENGINES = {"seq64": dict(mode="seq", fp64=True), "mb64": dict(mode="mb", fp64=True), "mb32": dict(mode="mb", fp64=False)}


def _score_setup(kind, scores, task=None, nonfinite=False, k=4, **kw):
    """An engine and a matrix whose row j scores scores[j]: one entry per row (column 3 j, x = 1, the score as its weight; w0 = 0, zero factors).
    nonfinite: three more rows scoring +inf, -inf and NaN from finite parameters (fp64 tables), or one row with a NaN weight (fp32 tables, which
    also keep only the scores whose float rounding is finite).  Returns (engine, probe, the score every row must have)."""
    engine, L = _fm()
    c = LINK_ENGINES[kind]
    z = np.asarray(scores, np.float64)
    if not c["fp64"]:
        with np.errstate(over="ignore"):
            z = z[np.isfinite(z.astype(np.float32))]
    rows, special = [[(a, 1.0)] for a in z], []
    if nonfinite and c["fp64"]:
        rows += [[(mm.BIG_W, mm.BIG_X)], [(-mm.BIG_W, mm.BIG_X)], [(mm.BIG_W, mm.BIG_X), (-mm.BIG_W, mm.BIG_X)]]
        special = mm.NONFINITE
    elif nonfinite:
        rows += [[(float("nan"), 1.0)]]
        special = [float("nan")]
    pr = mm.probe_rows(rows)
    e = engine.Engine(pr["p"], task=L.TASK_CLASSIFICATION if task is None else task, solver=L.SOLVER_SGD, num_factor=k,
                      mode=L.MODE_SEQUENTIAL if c["mode"] == "seq" else L.MODE_MINIBATCH, state_fp64=int(c["fp64"] and c["mode"] == "mb"), **kw)
    e.set_params(0.0, pr["w"], np.zeros((k, pr["p"])))
    stored = e.get_params()[1][0::3][:len(z)]
    assert np.array_equal(stored, z if c["fp64"] else z.astype(np.float32).astype(np.float64))
    return e, pr, np.concatenate([stored, special])


def _matrix(pr, y=None):
    engine, L = _fm()
    return engine.Matrix.from_csr(pr["rp"], pr["col"], pr["val"], pr["p"], None if y is None else np.asarray(y, np.float32))


@pytest.mark.parametrize("kind", list(LINK_ENGINES))
def test_predict_links_at_saturated_scores(kind):
    engine, L = _fm()
    e, pr, score = _score_setup(kind, mm.MARGINS, task=L.TASK_REGRESSION, nonfinite=True, min_target=LO, max_target=HI)
    m = _matrix(pr)
    # NONE: the stored score (0 + w x with x = 1: the value; -0 comes back as the +0 the sum starts from)
    raw = e.predict(m)
    fin = ~np.isnan(score)
    assert _same_bits(raw[fin], np.where(score[fin] == 0, 0.0, score[fin])) and np.isnan(raw[~fin]).all() and np.isnan(raw[-1])   # bit for bit; a stored -0: 0 + (-0) x 1 = +0
    # LOGISTIC: 1 / (1 + exp(-z)) -- exp within an ulp moves it by at most 2^-52 relative, the addition and the division 2^-53 each; where exp(-z)
    # overflows the truth is subnormal and the device gives 0: the first normal number
    t0 = time.time()
    p = e.predict(m, L.LINK_LOGISTIC)
    truth = mm.logistic(score)
    fin = ~np.isnan(score)
    err = np.abs(p[fin].astype(LD) - truth[fin]).astype(np.float64)
    bar = (LD(2.0) ** -51 * truth[fin]).astype(np.float64) + 2.0 ** -1022
    _report(f"predict {kind} LOGISTIC |p - truth|", err, bar, score[fin], t0)
    assert np.all(err <= bar) and np.isnan(p[~fin]).all()
    assert np.all(p[fin] >= 0.0) and np.all(p[fin] <= 1.0) and (p == 1.0).any() and (p == 0.0).any()
    # CLAMP: the oracle's clamp in every bit, NaN staying NaN
    want = raw.copy()
    oracle.lib().fmo_clamp(want.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(want)), ctypes.c_double(LO), ctypes.c_double(HI))
    assert _same_bits(e.predict(m, L.LINK_CLAMP), want) and np.isnan(want[-1]) and (want == LO).any() and (want == HI).any()
    # PROBIT: the table link at the finite scores
    zf = np.isfinite(score)
    got = e.predict(m, L.LINK_PROBIT)
    np.testing.assert_allclose(got[zf], oracle.fast_pnorm(score[zf]), rtol=0, atol=1e-15)
    e.close(); m.close()


@pytest.mark.parametrize("kind", list(LINK_ENGINES))
def test_topk_logistic_values_are_predicts_and_the_order_is_the_raw_scores(kind):
    """One context whose only feature (column 2: in no item) weighs 0, the scored rows as items: the returned values are fmx_predict's for the same
    (context, item) rows bit for bit, and the order is that of the raw score, NaN last -- also where hundreds of items share the probability 1 or 0."""
    engine, L = _fm()
    e, pr, score = _score_setup(kind, np.concatenate([mm.MARGINS[:4], mm.MARGINS[4::3]]), nonfinite=True)   # +0 and -0 among them: one score
    n = pr["n"]
    assert n <= 1024                                      # fmx_topk's largest K: every item is returned
    items = _matrix(pr)
    ctx = engine.Matrix.from_csr(np.array([0, 1], np.int64), np.array([2], np.uint32), np.ones(1, np.float32), pr["p"])
    idx, val = e.topk(ctx, items, n, link=L.LINK_LOGISTIC)
    idx, val = idx[0], val[0]
    assert sorted(idx.tolist()) == list(range(n))
    # the concatenated rows, columns ascending: the context's column 2 comes after item 0's column 0 and before every other item's
    rows_c, rows_v = [], []
    for j in range(n):
        c = list(pr["col"][pr["rp"][j]:pr["rp"][j + 1]]) + [2]
        x = list(pr["val"][pr["rp"][j]:pr["rp"][j + 1]]) + [1.0]
        o = np.argsort(c, kind="stable")
        rows_c.append(np.asarray(c)[o]); rows_v.append(np.asarray(x)[o])
    rp = np.concatenate([[0], np.cumsum([len(c) for c in rows_c])]).astype(np.int64)
    pairs = engine.Matrix.from_csr(rp, np.concatenate(rows_c).astype(np.uint32), np.concatenate(rows_v).astype(np.float32), pr["p"])
    p = e.predict(pairs, L.LINK_LOGISTIC)
    assert np.array_equal(e.predict(pairs), score, equal_nan=True)
    assert _same_bits(val, p[idx])
    raw = score[idx]
    nn = int(np.sum(~np.isnan(score)))
    assert not np.isnan(raw[:nn]).any() and np.isnan(raw[nn:]).all() and np.all(np.diff(raw[:nn]) <= 0)
    ties = np.diff(raw[:nn]) == 0
    assert ties.any() and np.all(np.diff(idx[:nn])[ties] > 0)            # equal raw scores (-0 and +0): the lower index first
    e.close(); items.close(); ctx.close(); pairs.close()


# ============================================================================================================ h. fmx_evaluate
EVAL_N = [1, 255, 256, 257, 4095, 4096, 4097, 8193]


def _eval_scores(n, saturated):
    rng = np.random.default_rng(1000 + n)
    pool = mm.MARGINS if saturated else mm.MARGINS[np.abs(mm.MARGINS) <= 30.0]
    return pool[rng.permutation(np.resize(np.arange(len(pool)), n))]


def _device_auc(p, y):
    """The device's stated rule: tmp = y > 0 ? p : -p, a STABLE sort by |tmp| (ties keep row order), then core/Evaluation.h:55-78's accumulation."""
    tmp = np.where(y > 0, p, -p)
    tmp = tmp[np.argsort(np.abs(tmp), kind="stable")]
    area = cum = 0.0
    for t in tmp:
        if t > 0:
            cum += 1.0
        else:
            area += cum
    if cum == 0 or cum == len(tmp):
        return 1.0
    area /= cum * (len(tmp) - cum)
    return 1 - area if area < 0.5 else area


@pytest.mark.parametrize("saturated", [False, True], ids=["moderate", "saturated"])
@pytest.mark.parametrize("n", EVAL_N)
def test_evaluate_classification_metrics_at_the_slab_edges(n, saturated):
    """LL, ACC and AUC against oracle.evaluate on the engine's own predict output.  With a probability of exactly 1 both sides give a NaN
    log-likelihood (log(1 - 1 - 1e-20), whatever the label: 0 x NaN).  The AUC with ties across the classes (equal probabilities, hundreds of them at
    0.5, 0 and 1) is held to a numpy restatement of the DEVICE's rule -- a stable sort by |tmp| in row order -- not to the reference, whose order
    of ties is the C library's qsort; without such ties it is the oracle's."""
    engine, L = _fm()
    e, pr, _ = _score_setup("seq64", _eval_scores(n, saturated))
    m0 = _matrix(pr)
    p = e.predict(m0, L.LINK_LOGISTIC)
    if saturated and n > 300:
        assert (p == 1.0).any() and (p == 0.0).any() and (p == 0.5).any()
    rng = np.random.default_rng(n)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0).astype(np.float32)
    m = _matrix(pr, y)
    want = oracle.evaluate(oracle.CLASSIFICATION, oracle.LL, p, y)
    got = e.evaluate(m, L.EVAL_LL)
    assert np.isnan(want) == bool((p == 1.0).any())
    assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12 * max(1.0, abs(want)), (got, want)
    assert e.evaluate(m, L.EVAL_ACC) == oracle.evaluate(oracle.CLASSIFICATION, oracle.ACC, p, y)
    got = e.evaluate(m, L.EVAL_AUC)
    assert abs(got - _device_auc(p, y)) <= 1e-12, (got, _device_auc(p, y))
    # no ties across the classes: every group of equal probabilities gets one label -- the reference's own number
    _, inv = np.unique(p, return_inverse=True)
    y1 = np.where(inv % 2 == 0, 1.0, -1.0).astype(np.float32)
    m1 = _matrix(pr, y1)
    want = oracle.evaluate(oracle.CLASSIFICATION, oracle.AUC, p, y1)
    assert abs(e.evaluate(m1, L.EVAL_AUC) - want) <= 1e-12, want
    e.close(); m0.close(); m.close(); m1.close()


@pytest.mark.parametrize("n", EVAL_N)
def test_evaluate_regression_metrics_at_the_slab_edges(n):
    engine, L = _fm()
    e, pr, _ = _score_setup("seq64", _eval_scores(n, True), task=L.TASK_REGRESSION, min_target=LO, max_target=HI)
    m0 = _matrix(pr)
    pred = e.predict(m0, L.LINK_CLAMP)
    if n > 300:
        assert (pred == LO).any() and (pred == HI).any()
    y = np.random.default_rng(n).normal(0, 2, n).astype(np.float32)
    m = _matrix(pr, y)
    for metric, oid in ((L.EVAL_RMSE, oracle.RMSE), (L.EVAL_MSE, oracle.MSE), (L.EVAL_MAE, oracle.MAE)):
        want = oracle.evaluate(oracle.REGRESSION, oid, pred, y)
        got = e.evaluate(m, metric)
        assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (metric, got, want)
    e.close(); m0.close(); m.close()
