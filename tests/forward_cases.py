"""Cases, the high-precision model and the child process shared by tests/test_gpu_forward_forms.py and tests/test_forward_cases_cpu.py.

The FORWARD-ONLY face of phase 1 (the TRAIN = false instances of fm_rows_forward_k / _dyn_k / _flat_k in fm_batch_kernels.hip, their link_apply and
qout epilogue, and launch_rows_forward's slab loop) is what fmx_predict, every evaluation call and -- through topk_project -- fmx_project and every
ranking call read a model with.  Its observables are held here per row to a model of the same operation, in every form the launcher can select:

    fmx_predict_device  FMX_LINK_NONE, and the task's own link (LOGISTIC for classification, CLAMP to [-0.2, 0.3] for regression)
    fmx_project_device  with_w0 = 0 and 1:  base[r], s[r][f]

Model, per stored entry (an unsorted row or a column stored twice needs nothing special), in np.longdouble (64-bit significand) from the engine's own
get_params():   s_f = sum_j x_j v_jf,    y = [k0] w0 + [k1] sum_j w_j x_j + 1/2 sum_f (s_f^2 - sum_j (x_j v_jf)^2),    base = y with and without w0.
tests/test_forward_cases_cpu.py holds it to a Fraction loop.

Bars -- derived, not measured.  u = 2^-53, gamma(n) = n u / (1 - n u); a row has n entries, the table kp padded factors (the padding adds exact zeros).
Every accumulation on the device is fp64, in an order that differs by form (one lane group per row, four with a butterfly, pieces of a chunk in the
flat form), so every bound below is the any-order one: a term that passes through at most m roundings carries a factor within gamma(m) of 1.
  tmp = v x     fp32 tables: both factors are floats widened to double, 24 x 24 significand bits: EXACT, not counted (t = 0).
                fp64 tables: one rounding (t = 1).
  s_f           n terms, n - 1 additions:                        |s_f - truth| <= gamma(n - 1 + t) sum_j |x v_f|  <=  gamma(n) sum_j |x v_f|
                fmx_project hands out (float) s_f for fp32 tables: plus half a float ulp of the truth (taken at |truth| + the fp64 bound)
  s_f^2         the sum's error twice and the product's rounding: 2 (n - 1 + t) + 1, relative to (sum_j |x v_f|)^2
  q             tmp^2: 2 t + 1 roundings.  The static and the pull kernel keep one q per factor (n - 1 additions); the flat kernel keeps ONE q per
                lane over its VEC factors (VEC = 4 floats or 2 doubles: VEC n - 1 additions), relative to sum (x v_f)^2
  1/2 (..)      the subtraction 1; the halving exact; over the factors VEC - 1 additions in the lane and log2(lanes) shuffles: at most kp - 1
  lin           w0 and n products (t each), n additions: n + t
  y = lin + pair   1
The longest chain is max(2 n + 2 t + kp + 1, VEC n + 2 t + kp + 2, n + t + 1) <= N_r = VEC n_r + kp + 4, so
  |y - truth| <= gamma(N_r) A_r,     A_r = [k0] |w0| + [k1] sum |w x| + 1/2 sum_f ((sum_j |x v_f|)^2 + sum_j (x v_f)^2).
The model's own error is the same count at u = 2^-64: MODEL_SLACK = 2^-11 of the bar, added to it.  A bar that is 0 (an empty row without w0) means an
exact zero.  Link outputs are held on the call's own raw output with the bars of tests/test_gpu_margins.py (LOGISTIC 2^-51 relative to
margin_model.logistic + 2^-1022; CLAMP the oracle's clamp in every bit).

Everything above `child_main` runs without a GPU.  `child_main` is what a fresh child process executes per set of process-wide switches:
`python -m tests.forward_cases <job.json>`.  A child asserts nothing about the numerics: per case, call and variant it writes the largest share of each
bar, the exact properties as booleans, the difference of fmx_debug_rows_forward_launches and a digest of the raw outputs."""
import ctypes
import hashlib
import json
import os
import sys
import time

import numpy as np

from tests import rows_cases as rc
from tests.rows_cases import (FLAT, LATE_ROWS, MIN_P, NARROW1, NARROW4, PULL, TAIL_ROWS, WIDE_PIPELINED, WIDE_SERIAL, _cached, _special_rows, expected_form, labels,
                              lanes, padded, problem, quiet_features, start_params, static_form)

ROOT = rc.ROOT
LD = np.longdouble
U = 2.0 ** -53
MODEL_SLACK = 2.0 ** -11
LO, HI = -0.2, 0.3                 # regression's clamps (rows_cases.engine_options)
SLAB, PROJ_SLAB = 1 << 18, 1 << 16   # launch_rows_forward's launches, project_run's slabs
GUARD = 64                         # elements in front of and behind every output
FILL = 0x7FF8DEADBEEF0123          # the NaN every output and guard element holds before a call
P = MIN_P + 257

CHILDREN = [("default", {}), ("serial", {"FMX_ROWS_SERIAL": "1"}), ("pipelined", {"FMX_ROWS_SERIAL": "0"})]
ALL, PINNED = ["default", "serial", "pipelined"], ["serial", "pipelined"]


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def fp64_tables(case):
    return bool(case["fp64"] or case["seq"])


def case_lanes(case):
    return lanes(case["k"], fp64_tables(case))


def chain(n, case):
    """N_r of the module's docstring"""
    t = fp64_tables(case)
    return (2 if t else 4) * np.asarray(n, np.float64) + padded(case["k"], t) + 4


# --------------------------------------------------------------------------------------------------------------------- cases
def _case(name, kind, k, fp64, rows, values, children, **opts):
    lpr = lanes(k, bool(fp64) or bool(opts.get("seq")))
    limit = opts.pop("limit", None)
    if limit is None:   # rows_cases' truncated step: a wide call stays wide where it can, 21 rows above the threshold
        edge = -(-512 * 256 // lpr) + 21
        limit = edge if static_form(rows, lpr) == "wide" and edge < rows else (rows * 5 // 8) | 1
    assert limit <= rows - LATE_ROWS
    c = dict(name=name, kind=kind, k=k, fp64=bool(fp64), rows=rows, values=bool(values), children=list(children), limit=limit, task="classification", keep_w0=1,
             keep_w1=1, w_in_row=0, seq=0, p=P)
    c.update(opts)
    return c


def instance_of(form, case):
    return (min(form, WIDE_SERIAL), fp64_tables(case), case_lanes(case))


def _predict_cases():
    """One case per (form, element type, lanes) instance of the three static forms: the first of rows_cases.CASES that reaches it with its full step,
    value kinds alternating.  A wide call of 65 536 rows or more would be timed by an engine that is not pinned: pinned children only."""
    out, seen = [], set()
    for c in rc.CASES:
        if c["children"][0] not in ("default", "serial") or c["task"] != "classification" or c["w_in_row"] or c["tile_rows"] or c["chunks"] > 1 \
                or not c["keep_w0"] or not c["keep_w1"] or c["solver"] != "sgd":
            continue
        lpr = lanes(c["k"], c["fp64"])
        form = static_form(c["rows"], lpr)
        inst = (WIDE_SERIAL if form == "wide" else form, c["fp64"], lpr)
        if inst in seen:
            continue
        seen.add(inst)
        values = len(out) % 2 == 0
        wide = form == "wide"
        children = (PINNED if c["rows"] >= 65536 else ALL) if wide else ["default"]
        name = f"predict_{'wide' if wide else rc.FORM_NAMES[form]}_{'f64' if c['fp64'] else 'f32'}_k{c['k']}_{'val' if values else 'onehot'}"
        out.append(_case(name, "predict", c["k"], c["fp64"], c["rows"], values, children, limit=c["limit"]))
    return out


def _cases():
    out = _predict_cases()
    small = 960 + TAIL_ROWS
    # the projection: always 256-thread workgroups, one lane group per row: every lanes instance at 997 rows
    for i, (k, fp64) in enumerate([(3, 0), (6, 0), (12, 0), (32, 0), (64, 0), (128, 0), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (128, 1)]):
        out.append(_case(f"project_{'f64' if fp64 else 'f32'}_k{k}_{'val' if i % 2 else 'onehot'}", "project", k, fp64, small, i % 2, ALL))
    # k = 16 under the other things the forward reads, in each form; one value kind each, rotating
    extras = [("wir", dict(w_in_row=1)), ("now0", dict(keep_w0=0)), ("now1", dict(keep_w1=0)), ("regr", dict(task="regression")), ("seq", dict(seq=1)), ("k0", dict(k=0))]
    for a, (form, rows) in enumerate((("narrow4", small), ("narrow1", 16384 + TAIL_ROWS), ("wide", 32768 + TAIL_ROWS))):
        for b, (tag, opts) in enumerate(extras):
            v = (a + b) % 2 == 0
            opts = dict(opts)
            k = opts.pop("k", 16)
            r = rows
            if tag == "k0" and form != "narrow4":
                r = (65536 if form == "narrow1" else 131072) + TAIL_ROWS   # one lane per row
            if tag == "seq" and form == "narrow1":
                r = 8192 + TAIL_ROWS   # fp64 tables: eight lanes per row
            got = static_form(r, lanes(k, bool(opts.get("seq"))))
            assert got == "wide" if form == "wide" else rc.FORM_NAMES[got] == form
            out.append(_case(f"extra_{form}_{tag}_{'val' if v else 'onehot'}", "extra", k, False, r, v, ((PINNED if r >= 65536 else ALL) if got == "wide" else ["default"]), **opts))
    # a small hand-made matrix: unsorted rows, a column stored twice in a row, an all-empty range, r1 == r0
    out.append(_case("hand_f32_k5", "hand", 5, False, 0, True, ["default"], p=48, limit=-LATE_ROWS))
    out.append(_case("hand_f64_k5", "hand", 5, True, 0, True, ["default"], p=48, limit=-LATE_ROWS))
    # the seams: launch_rows_forward's second launch, project_run's second slab.  Timed by an engine that is not pinned: pinned children only
    for k, fp64 in ((3, False), (2, True)):
        t = "f64" if fp64 else "f32"
        out.append(_case(f"seam_predict_{t}_k{k}", "seam_predict", k, fp64, 87397, not fp64, PINNED))   # 3 x 87 397 = 262 191 rows >= 2^18 + 37
        out.append(_case(f"seam_project_{t}_k{k}", "seam_project", k, fp64, 21861, fp64, PINNED))      # 3 x 21 861 = 65 583 rows >= 2^16 + 37
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()


def cases_of(child):
    return [c for c in CASES if child in c["children"]]


def case_calls(case):
    """The calls of a case, in order: (op, r0, r1).  predict: the first step, the second, and a range that starts at an odd row inside the second step
    (not workgroup-aligned) and ends the truncated count later (the last workgroup partly filled).  project: those three and both steps as one call."""
    rows, lim, kind = case["rows"], case["limit"], case["kind"]
    three = [(0, rows), (rows, 2 * rows), (rows + 2, rows + 2 + lim)]
    if kind == "predict":
        return [("predict", a, b) for a, b in three]
    if kind == "project":
        return [("project", a, b) for a, b in three + [(0, 2 * rows)]]
    if kind == "extra":
        return [("predict", a, b) for a, b in three] + [("project", 0, 997), ("project", 3, 1000), ("project", 0, 1000)]
    if kind == "hand":
        n, (e0, e1) = len(HAND_ROWS), HAND_EMPTY
        return [(op, a, b) for op in ("predict", "project") for a, b in ((0, n), (e0, e1), (1, n - 1), (5, 5))]
    if kind == "seam_predict":
        return [("predict", 0, SLAB + 37)]
    assert kind == "seam_project"
    return [("project", 0, PROJ_SLAB + 37), ("project", PROJ_SLAB - 5, PROJ_SLAB + 37), ("project", 0, PROJ_SLAB), ("project", PROJ_SLAB, PROJ_SLAB + 37)]


def model_rows(case):
    return max(b for _, _, b in case_calls(case))


def call_is_wide(case, op, n):
    return n > 0 and (op == "project" or static_form(n, case_lanes(case)) == "wide")


def variants_of(case, op, n):
    """The opt-in kernels exist for wide launches of matrices whose rows differ in length"""
    return ["pull", "flat", "plain"] if call_is_wide(case, op, n) and case["kind"] != "hand" else ["plain"]


def expected_launches(case, op, n, child, variant):
    """The six slots one call must add to fmx_debug_rows_forward_launches.  predict: launches of 2^18 rows in the form of the CALL's row count;
    project: slabs of 2^16 rows, always wide (fixed_schedule)."""
    want = [0] * 6
    if n == 0:
        return want
    if op == "project":
        form = PULL if variant == "pull" else FLAT if variant == "flat" else WIDE_PIPELINED if child == "pipelined" else WIDE_SERIAL
        assert child in PINNED or n < 65536
        want[form] = -(-n // PROJ_SLAB)
    else:
        want[expected_form(n, case_lanes(case), child, variant)] = -(-n // SLAB)
    return want


# --------------------------------------------------------------------------------------------------------------------- matrices
HAND_ROWS = [[(7, 1.5), (3, -2.0), (40, 0.25), (11, 1.0)],                 # unsorted
             [(5, 1.0), (5, 2.0), (9, -1.0)],                              # a column stored twice
             [], [(0, 3.0)], [(47, -0.5), (46, 0.5), (45, 2.0), (47, 1.0), (1, 1.0)],   # unsorted and twice
             [], [], [], [], [],                                          # an all-empty range
             [(2, 1.0), (1, 1.0), (0, 1.0)], [(30, 0.125)] * 7, [(12, 1.0), (13, -1.0)]]
HAND_EMPTY = (5, 10)


def hand_problem():
    lens = [len(r) for r in HAND_ROWS]
    rp = np.zeros(len(lens) + 1, np.int64)
    rp[1:] = np.cumsum(lens)
    return dict(n=len(lens), p=48, rows=0, rp=rp, col=np.array([c for r in HAND_ROWS for c, _ in r], np.uint32), val=np.array([x for r in HAND_ROWS for _, x in r], np.float32))


def matrix_key(case):
    return (case["kind"] == "hand", case["rows"], case["p"], case["values"])


def case_problem(case):
    if case["kind"] == "hand":
        return hand_problem()
    return problem(case["rows"], case["p"], case["values"], 29 + case["rows"] % 1000 + (1 if case["values"] else 0))


def case_params(case):
    if case["kind"] == "hand":   # small rows: weights of the order of one
        rng = np.random.default_rng(3)
        f = lambda *s: rng.normal(0, 0.5, s).astype(np.float32).astype(np.float64)   # noqa: E731
        return float(f(1)[0]), f(case["p"]), f(case["k"], case["p"])
    w0, w, v = start_params(case["p"], max(case["k"], 1), rc.case_seed(case), case["task"])   # (w0 and w are drawn before v: the same at every k)
    return w0, w, v[:case["k"]]


# --------------------------------------------------------------------------------------------------------------------- the model
def _row_sums(rp, r0, r1):
    """sum over each row's entries, in entry order, of an array over the entries of rows [r0, r1)"""
    n = np.diff(rp[r0:r1 + 1])
    live = n > 0
    starts = (rp[r0:r1] - rp[r0])[live]

    def rowsum(t):
        out = np.zeros(r1 - r0, t.dtype)
        if len(t):
            out[live] = np.add.reduceat(t, starts)
        return out
    return n, rowsum


def model(prob, case, params, r0, r1, dtype=LD, drop_entry=None, factors=None):
    """Rows [r0, r1): y0 (without w0), s[R][k] in `dtype`; the scales A0 (y0's absolute sum), As[R][k] = sum |x v_f| in float64; n the rows' entries.
    drop_entry: an entry index of the matrix that is left out; factors: only the first `factors` factors take part (the planted faults of the CPU checks)."""
    rp, k = prob["rp"], case["k"] if factors is None else factors
    w0, w, v = params
    e0, e1 = int(rp[r0]), int(rp[r1])
    col = prob["col"][e0:e1].astype(np.int64)
    x = prob["val"][e0:e1].astype(dtype)
    if drop_entry is not None and e0 <= drop_entry < e1:
        x = x.copy()
        x[drop_entry - e0] = 0
    n, rowsum = _row_sums(rp, r0, r1)
    R = r1 - r0
    lin, a_lin = np.zeros(R, dtype), np.zeros(R)
    if case["keep_w1"]:
        wx = w[col].astype(dtype) * x
        lin, a_lin = rowsum(wx), rowsum(np.abs(wx).astype(np.float64))
    pair, a_pair = np.zeros(R, dtype), np.zeros(R)
    s, a_s = np.zeros((R, case["k"]), dtype), np.zeros((R, case["k"]))
    for f in range(k):
        vx = v[f, col].astype(dtype) * x
        sf, qf, af = rowsum(vx), rowsum(vx * vx), rowsum(np.abs(vx).astype(np.float64))
        pair += sf * sf - qf
        a_pair += af * af + qf.astype(np.float64)
        s[:, f], a_s[:, f] = sf, af
    return dict(y0=lin + pair / 2, s=s, A0=a_lin + 0.5 * a_pair, As=a_s, n=n.astype(np.int64))


def with_w0(case, params, mod):
    """(y, A) with the bias as the engine adds it"""
    if not case["keep_w0"]:
        return mod["y0"], mod["A0"]
    return mod["y0"] + LD(params[0]), mod["A0"] + abs(params[0])


def y_bar(case, A, n):
    return gamma(chain(n, case)) * A * (1 + MODEL_SLACK)


def s_bar(case, mod):
    """fp64 tables: gamma(n) sum |x v_f|; fp32 tables: plus half a float ulp of the truth, taken at |truth| + the fp64 bound (the float rounds the device's sum)"""
    b = gamma(mod["n"])[:, None] * mod["As"] * (1 + MODEL_SLACK)
    if not fp64_tables(case):
        with np.errstate(over="ignore"):
            b = b + 0.5 * np.spacing((np.abs(mod["s"]).astype(np.float64) + b).astype(np.float32)).astype(np.float64)
    return b


def share(got, truth, bar):
    """(the largest |got - truth| / bar over the elements whose bar is not 0 -- inf if anything there is not finite --, every element whose bar is 0 is an exact 0)"""
    got, bar = np.asarray(got, np.float64), np.asarray(bar, np.float64)
    err = np.abs(got.astype(LD) - truth).astype(np.float64)
    live = bar > 0
    r = float(np.max(err[live] / bar[live])) if live.any() else 0.0
    return (r if np.isfinite(r) else float("inf")), bool(np.all(got[~live] == 0) and not np.signbit(got[~live]).any())


def logistic_share(p, raw):
    """tests/test_gpu_margins.py::test_predict_links_at_saturated_scores: |p - truth| <= 2^-51 truth + 2^-1022, truth = margin_model.logistic(the raw output)"""
    from tests import margin_model as mm
    truth = mm.logistic(raw)
    err = np.abs(p.astype(LD) - truth).astype(np.float64)
    bar = (LD(2.0) ** -51 * truth).astype(np.float64) + 2.0 ** -1022
    r = float(np.max(err / bar)) if len(p) else 0.0
    return r if np.isfinite(r) else float("inf")


def clamp_exact(got, raw):
    """the oracle's clamp of the raw output, in every bit"""
    import oracle
    want = np.array(raw, np.float64)
    oracle.lib().fmo_clamp(want.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(want)), ctypes.c_double(LO), ctypes.c_double(HI))
    return bool(np.array_equal(got.view(np.uint64), want.view(np.uint64)))


def slice_model(mod, a, b):
    return {name: val[a:b] for name, val in mod.items()}


# --------------------------------------------------------------------------------------------------------------------- the child process
def _counter(L):
    a = (ctypes.c_int64 * 6)()
    L.check(L.lib().fmx_debug_rows_forward_launches(a))
    return np.array(list(a), np.int64)


class Guarded:
    """A float64 device output of n elements between two guard zones, every element pre-filled with one NaN bit pattern"""

    def __init__(self, util, n):
        self.n = int(n)
        self.buf = util.DevBuf(self.n + 2 * GUARD)
        self.buf.upload(np.full(self.n + 2 * GUARD, FILL, np.uint64).view(np.float64))
        self.ptr = self.buf.ptr.value + GUARD * 8

    def read(self):
        """(the n elements, guards intact)"""
        a = self.buf.numpy()
        self.buf.free()
        g = a.view(np.uint64)
        return a[GUARD:GUARD + self.n].copy(), bool(np.all(g[:GUARD] == FILL) and np.all(g[GUARD + self.n:] == FILL))


def _digest(*arrays):
    h = hashlib.blake2b(digest_size=16)
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _engine(case, engine, L):
    regr = case["task"] == "regression"
    o = dict(task=L.TASK_REGRESSION if regr else L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=case["k"], keep_w0=case["keep_w0"], keep_w1=case["keep_w1"])
    if case["seq"]:
        o.update(mode=L.MODE_SEQUENTIAL)
    else:
        o.update(mode=L.MODE_MINIBATCH, batch_rows=max(case["rows"], 64), state_fp64=int(case["fp64"]))
    if regr:
        o.update(min_target=LO, max_target=HI)
    if case["w_in_row"]:
        os.environ["FMX_W_IN_ROW"] = "1"   # read at engine creation
    try:
        return engine.Engine(case["p"], **o)
    finally:
        os.environ.pop("FMX_W_IN_ROW", None)


def _predict_call(case, e, m, L, util, r0, r1, mod, params):
    n = r1 - r0
    link = L.LINK_CLAMP if case["task"] == "regression" else L.LINK_LOGISTIC
    raw_b, lnk_b = Guarded(util, n), Guarded(util, n)
    before = _counter(L)
    L.check(L.lib().fmx_predict_device(e.h, m.h, ctypes.c_int64(r0), ctypes.c_int64(r1), ctypes.c_void_p(raw_b.ptr), ctypes.c_int(L.LINK_NONE)))
    e.sync()
    launches = _counter(L) - before
    L.check(L.lib().fmx_predict_device(e.h, m.h, ctypes.c_int64(r0), ctypes.c_int64(r1), ctypes.c_void_p(lnk_b.ptr), ctypes.c_int(link)))
    e.sync()
    (raw, g0), (lnk, g1) = raw_b.read(), lnk_b.read()
    y, A = with_w0(case, params, mod)
    sh, zero = share(raw, y, y_bar(case, A, mod["n"]))
    empty = mod["n"] == 0
    r = dict(y=sh, zero_bar_zero=zero, guards=bool(g0 and g1), launches=[int(x) for x in launches], digest=_digest(raw, lnk), rows=int(n), compared=int(len(raw)),
             empty=int(empty.sum()), empty_exact=bool(np.array_equal(raw[empty].view(np.uint64), np.full(int(empty.sum()), params[0] if case["keep_w0"] else 0.0).view(np.uint64))))
    if case["task"] == "regression":
        r.update(clamp_exact=clamp_exact(lnk, raw), clamped_low=int((lnk == LO).sum()), clamped_high=int((lnk == HI).sum()))
    else:
        r.update(logistic=logistic_share(lnk, raw))
    return r, raw


def _project_call(case, e, m, L, util, r0, r1, mod, params):
    n, k = r1 - r0, case["k"]
    out = {}
    launches = []
    for w in (0, 1):
        b, s = Guarded(util, n), Guarded(util, n * k)
        before = _counter(L)
        e.project_device(m, r0, r1, b.ptr, s.ptr if k else None, with_w0=bool(w))
        e.sync()
        launches.append([int(x) for x in _counter(L) - before])
        out[w] = b.read() + s.read()
    (b0, g0, s0, g1), (b1, g2, s1, g3) = out[0], out[1]
    y, A = with_w0(case, params, mod)
    sh0, z0 = share(b0, mod["y0"], y_bar(case, mod["A0"], mod["n"]))
    sh1, z1 = share(b1, y, y_bar(case, A, mod["n"]))
    shs, zs = share(s0.reshape(n, k), mod["s"], s_bar(case, mod))
    empty = mod["n"] == 0
    # base(with_w0 = 1) - base(with_w0 = 0) is w0 up to both sides' bars (the difference itself taken in long double); without a bias: the same bits
    w0 = LD(params[0]) if case["keep_w0"] else LD(0)
    dbar = y_bar(case, A, mod["n"]) + y_bar(case, mod["A0"], mod["n"])
    derr = np.abs((b1.astype(LD) - b0.astype(LD)) - w0).astype(np.float64)
    live = dbar > 0
    dsh = float(np.max(derr[live] / dbar[live])) if live.any() else 0.0
    r = dict(base0=sh0, base1=sh1, s=shs, w0_step=dsh if np.isfinite(dsh) else float("inf"), zero_bar_zero=bool(z0 and z1 and zs and np.all(derr[~live] == 0)),
             guards=bool(g0 and g1 and g2 and g3), launches=launches[0], launches_w0=launches[1], digest=_digest(b0, b1, s0), rows=int(n), compared=int(len(b0)),
             s_same=bool(np.array_equal(s0.view(np.uint64), s1.view(np.uint64))), empty=int(empty.sum()),
             same_without_bias=bool(case["keep_w0"] or np.array_equal(b0.view(np.uint64), b1.view(np.uint64))),
             empty_exact=bool(np.all(b0[empty].view(np.uint64) == 0) and np.all(s0.reshape(n, k)[empty].view(np.uint64) == 0)
                              and np.array_equal(b1[empty].view(np.uint64), np.full(int(empty.sum()), float(w0)).view(np.uint64))))
    return r, (b0, b1, s0.reshape(n, k))


def _set_variant(variant):
    rc._set_variant(variant)


def _run_case(job, case, prob, engine, L, util):
    params = case_params(case)
    m = engine.Matrix.from_csr(prob["rp"], prob["col"], prob["val"], case["p"], labels(prob["n"], 1, case["task"]))
    e = _engine(case, engine, L)
    e.set_params(*params)
    held = e.get_params()
    same = bool(held[0] == params[0] and np.array_equal(held[1], params[1]) and np.array_equal(held[2], params[2]))
    M = model_rows(case)
    t0 = time.time()
    key = hashlib.blake2b(np.float64(held[0]).tobytes() + held[1].tobytes() + held[2].tobytes(), digest_size=8).hexdigest()
    mod = _cached(os.path.join(job["ref"], f"{case['name']}.{key}.npz"), lambda: model(prob, case, held, 0, M))
    t_model = time.time() - t0
    out = dict(params_held=same, w_in_row=bool(e.w_in_row()) if not fp64_tables(case) else False, calls=[], model_seconds=t_model)
    kept = {}   # (r0, r1) -> the plain projection of that range: a row's bits must not depend on the range
    for op, r0, r1 in case_calls(case):
        sub = slice_model(mod, r0, r1)
        call = dict(op=op, r0=r0, r1=r1, variants={})
        for variant in variants_of(case, op, r1 - r0):
            _set_variant(variant)
            try:
                r, raw = (_predict_call if op == "predict" else _project_call)(case, e, m, L, util, r0, r1, sub, held)
            finally:
                _set_variant("plain")
            if op == "project" and variant == "plain":
                r["same_as"] = {}
                for (a, b), (p0, p1, ps) in kept.items():
                    lo, hi = max(a, r0), min(b, r1)
                    if lo < hi:
                        r["same_as"][f"{a}:{b}"] = bool(all(np.array_equal(u[lo - a:hi - a].view(np.uint64), w[lo - r0:hi - r0].view(np.uint64))
                                                            for u, w in zip((p0, p1, ps), raw)))
                kept[(r0, r1)] = raw
            call["variants"][variant] = r
        out["calls"].append(call)
    e.close()
    m.close()
    return out


def child_main(path):
    with open(path) as f:
        job = json.load(f)
    from fmwr_amd import _lib as L
    from fmwr_amd import engine
    from tests import util
    t0 = time.time()
    results, probs = {}, {}
    for case in job["cases"]:
        key = matrix_key(case)
        if key not in probs:
            probs.clear()    # cases come sorted by matrix: one at a time stays resident
            probs[key] = _cached(os.path.join(job["ref"], "matrix.%d.%d.%d.%d.npz" % key), lambda: case_problem(case))
        t1 = time.time()
        try:
            results[case["name"]] = _run_case(job, case, probs[key], engine, L, util)
        except L.FmxError as err:
            if err.status not in (L.ERR_INVALID, L.ERR_STATE):   # anything the device reported ends the child
                raise
            results[case["name"]] = dict(error=str(err), calls=[])   # a call the library refused: the parent's test of this case fails with its words
        results[case["name"]]["seconds"] = time.time() - t1
    with open(job["out"], "w") as f:
        json.dump(dict(seconds=time.time() - t0, cases=results), f)
    print("DONE", len(job["cases"]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main(sys.argv[1])
