"""CPU self-checks of tests/forward_cases.py: the long-double model is a Fraction loop's, the derived bars are wide enough for a correct
implementation (the oracle's forward; fp64 evaluations of the kernels' expressions in 20 random entry orders, in the four-lane-group order and in the
lane tree's) and tight enough for a planted fault (an entry of the longest row dropped, two neighbouring rows' outputs swapped, s shifted by one
factor, one factor too few), and the case table reaches every form and instance it says it does."""
from fractions import Fraction

import numpy as np
import pytest

import oracle
from tests import forward_cases as fc
from tests import rows_cases as rc
from tests import util

LD = np.longdouble
SMALL = [c for c in fc.CASES if c["rows"] <= 1000]   # every matrix of at most ~1 000 rows per step (the hand-made one among them)


def _exact(x):
    """a long double as a Fraction: its 64-bit significand is the exact sum of two doubles"""
    hi = float(x)
    return Fraction(hi) + Fraction(float(x - LD(hi)))


def _fraction_model(prob, case, params, r):
    """(y without w0, s[k]) of row r, exactly"""
    w0, w, v = params
    e = range(int(prob["rp"][r]), int(prob["rp"][r + 1]))
    x = [Fraction(float(prob["val"][i])) for i in e]
    col = [int(prob["col"][i]) for i in e]
    y = sum((Fraction(float(w[j])) * a for j, a in zip(col, x)), Fraction(0)) if case["keep_w1"] else Fraction(0)
    s = []
    for f in range(case["k"]):
        t = [Fraction(float(v[f, j])) * a for j, a in zip(col, x)]
        s.append(sum(t, Fraction(0)))
        y += (s[-1] ** 2 - sum((u * u for u in t), Fraction(0))) / 2
    return y, s


@pytest.mark.parametrize("fp64", [False, True], ids=["f32_tables", "f64_tables"])
def test_model_equals_a_fraction_loop(fp64):
    """The hand-made matrix and a small ragged one: every y0 and s_f of the long-double model against exact rational arithmetic, within the chain
    count at u = 2^-64 -- which is what MODEL_SLACK adds to the bars."""
    rp, col, val = util.random_csr(60, 48, 9, 4)
    ragged = dict(n=60, p=48, rows=0, rp=rp, col=col, val=val)
    for prob in (fc.hand_problem(), ragged):
        case = fc._case("cpu", "hand", 5, fp64, 0, True, ["default"], p=48, limit=-rc.LATE_ROWS)
        rng = np.random.default_rng(11)
        params = fc.case_params(case) if not fp64 else (float(rng.normal()), rng.normal(0, 0.5, 48), rng.normal(0, 0.5, (5, 48)))   # doubles that are no floats
        mod = fc.model(prob, case, params, 0, prob["n"])
        u_ld = float(np.finfo(LD).eps) / 2
        assert u_ld <= 2.0 ** -64
        worst = 0.0
        for r in range(prob["n"]):
            y, s = _fraction_model(prob, case, params, r)
            N = float(fc.chain(mod["n"][r], case))
            ey = abs(_exact(mod["y0"][r]) - y)
            assert ey <= Fraction(N * u_ld * 1.01 * mod["A0"][r]), (r, float(ey))
            for f in range(5):
                es = abs(_exact(mod["s"][r, f]) - s[f])
                assert es <= Fraction(float(mod["n"][r]) * u_ld * 1.01 * mod["As"][r, f]), (r, f, float(es))
            bar = float(fc.y_bar(case, mod["A0"][r], mod["n"][r]))
            if bar > 0:
                worst = max(worst, float(ey) / bar)
            assert bool(mod["A0"][r] == 0) == bool(mod["n"][r] == 0)
        print("model against Fraction, share of the bar:", worst)
        assert worst <= fc.MODEL_SLACK


def test_gamma_and_chain_are_what_the_docstring_says():
    assert fc.gamma(1) == fc.U / (1 - fc.U) and abs(fc.gamma(5000) / (5000 * fc.U) - 1) < 1e-12
    f32, f64 = dict(k=16, fp64=False, seq=0), dict(k=16, fp64=True, seq=0)
    assert fc.chain(12, f32) == 4 * 12 + 16 + 4 and fc.chain(12, f64) == 2 * 12 + 16 + 4 and fc.chain(0, dict(k=0, fp64=False, seq=0)) == 8
    assert fc.chain(12, dict(k=16, fp64=False, seq=1)) == fc.chain(12, f64)   # a sequential engine's tables are fp64
    for case in (f32, f64):   # the longest chain of the docstring, for every row length and both kernels' q
        t, vec = (1, 2) if case["fp64"] else (0, 4)
        kp = fc.padded(16, case["fp64"])
        for n in (1, 2, 12, 5000):
            assert max(2 * n + 2 * t + kp + 1, vec * n + 2 * t + kp + 2, n + t + 1) <= fc.chain(n, case)


# --------------------------------------------------------------------------------------------------------------------- wide enough
def _device_like(prob, case, params, r0, r1, order, split=1, tree=False):
    """The kernels' expressions in fp64 numpy: tmp = v x; s += tmp, q += tmp tmp over a row's entries in `order` (a key per entry: entries of a row are
    added by ascending key), as `split` interleaved partial sums that meet in a butterfly; pair = sum_f 1/2 (s^2 - q) front to back, or with `tree`
    per lane of VEC factors and then pairwise across the lanes; y = lin + pair."""
    rp, k = prob["rp"], case["k"]
    w0, w, v = params
    e0, e1 = int(rp[r0]), int(rp[r1])
    row = np.repeat(np.arange(r1 - r0), np.diff(rp[r0:r1 + 1]))
    perm = np.lexsort((order[e0:e1], row))
    col, x = prob["col"][e0:e1].astype(np.int64)[perm], prob["val"][e0:e1].astype(np.float64)[perm]
    pos = np.arange(e1 - e0) - (rp[r0:r1] - e0)[row]   # the entry's index inside its row
    R = r1 - r0

    def rowsum(t):
        parts = []
        for sub in range(split):
            sel = pos % split == sub
            parts.append(np.bincount(row[sel], t[sel], R))   # a bin's weights are added in entry order
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] for i in range(0, len(parts), 2)]
        return parts[0]
    lin = np.full(R, w0 if case["keep_w0"] else 0.0)
    if case["keep_w1"]:
        lin = lin + rowsum(w[col] * x)
    s = np.zeros((R, k))
    halves = []
    for f in range(k):
        tmp = v[f, col] * x
        s[:, f] = rowsum(tmp)
        halves.append(0.5 * (s[:, f] * s[:, f] - rowsum(tmp * tmp)))
    if tree and k:
        vec = 2 if fc.fp64_tables(case) else 4
        halves += [np.zeros(R)] * (fc.padded(k, fc.fp64_tables(case)) - k)
        lanes = [sum(halves[i + 1:i + vec], halves[i]) for i in range(0, len(halves), vec)]
        while len(lanes) > 1:
            lanes = [lanes[i] + lanes[i + 1] for i in range(0, len(lanes), 2)]
        pair = lanes[0]
    else:
        pair = sum(halves, np.zeros(R))
    return lin + pair, s


def _oracle_y(prob, case, params, r0, r1):
    rp = prob["rp"]
    X = oracle.Matrix(rp[r0:r1 + 1] - rp[r0], prob["col"][rp[r0]:rp[r1]], prob["val"][rp[r0]:rp[r1]], prob["p"])
    P = oracle.params(task=oracle.CLASSIFICATION, k=case["k"], k0=bool(case["keep_w0"]), k1=bool(case["keep_w1"]))
    return oracle.predict_batch(P, X, params[0], params[1], np.asarray(params[2], np.float64).ravel())


WIDE_ENOUGH = {}


@pytest.mark.parametrize("case", SMALL, ids=[c["name"] for c in SMALL])
def test_bars_are_wide_enough_for_a_correct_implementation(case):
    prob, params = fc.case_problem(case), fc.case_params(case)
    R = prob["n"] if case["kind"] == "hand" else case["rows"]
    mod = fc.model(prob, case, params, 0, R)
    y, A = fc.with_w0(case, params, mod)
    ybar, sbar = fc.y_bar(case, A, mod["n"]), fc.s_bar(case, mod)
    worst = dict(y=0.0, s=0.0)

    def hold(got_y, got_s, what):
        if not fc.fp64_tables(case):
            got_s = got_s.astype(np.float32).astype(np.float64)   # fmx_project hands out floats
        sy, zy = fc.share(got_y, y, ybar)
        ss, zs = fc.share(got_s, mod["s"], sbar)
        assert sy <= 1.0 and ss <= 1.0 and zy and zs, (case["name"], what, sy, ss)
        worst["y"], worst["s"] = max(worst["y"], sy), max(worst["s"], ss)
    sy, zy = fc.share(_oracle_y(prob, case, params, 0, R), y, ybar)   # the oracle's forward: fp64, a row's entries front to back
    assert sy <= 1.0 and zy, (case["name"], "oracle.predict_batch", sy)
    worst["oracle"] = sy
    rng = np.random.default_rng(rc.case_seed(case))
    nnz = len(prob["col"])
    for i in range(20):
        hold(*_device_like(prob, case, params, 0, R, rng.random(nnz)), f"random order {i}")
    front = np.arange(nnz, dtype=np.float64)
    hold(*_device_like(prob, case, params, 0, R, front, split=4), "four lane groups per row")
    hold(*_device_like(prob, case, params, 0, R, front, tree=True), "the lane tree")
    print(case["name"], "largest shares of the bars:", worst)
    WIDE_ENOUGH[case["name"]] = worst


# --------------------------------------------------------------------------------------------------------------------- tight enough
@pytest.mark.parametrize("case", fc.CASES, ids=[c["name"] for c in fc.CASES])
def test_bars_are_tight_enough_to_catch_a_fault(case):
    """Each planted fault leaves the bar on EVERY row it affects.  (Evaluated in fp64: a fault is many orders above its rounding.)"""
    prob, params = fc.case_problem(case), fc.case_params(case)
    hand = case["kind"] == "hand"
    R = prob["n"] if hand else min(fc.model_rows(case), 2 * case["rows"])
    k = case["k"]
    mod = fc.model(prob, case, params, 0, R, dtype=np.float64)
    y, A = fc.with_w0(case, params, mod)
    ybar, sbar = fc.y_bar(case, A, mod["n"]), fc.s_bar(case, mod)
    n = mod["n"]
    # 1. one entry of the longest row is dropped (the 5 000-entry row of the first step)
    long_row = int(np.argmax(n))
    assert hand or n[long_row] == rc.LONG_ROW
    entry = int(prob["rp"][long_row]) + int(n[long_row]) // 2
    bad = fc.model(prob, case, params, long_row, long_row + 1, dtype=np.float64, drop_entry=entry)
    assert abs(float(bad["y0"][0] - mod["y0"][long_row])) > ybar[long_row], (case["name"], "dropped entry, y")
    if k:
        assert np.all(np.abs(bad["s"][0] - mod["s"][long_row]) > sbar[long_row]), (case["name"], "dropped entry, s")
    # 2. the outputs of rows 2 i and 2 i + 1 change places: every row whose neighbour's truth differs
    even = (R // 2) * 2
    swap = np.arange(even).reshape(-1, 2)[:, ::-1].ravel()
    moved = y[:even][swap] != y[:even]
    assert (hand or moved.sum() > 0.9 * even) and moved.any() and np.all(np.abs(y[:even][swap] - y[:even])[moved] > ybar[:even][moved]), (case["name"], "swapped rows, y")
    if k:
        ds = np.abs(mod["s"][:even][swap] - mod["s"][:even])
        moved = (ds > 0).any(axis=1)
        assert (hand or moved.sum() > 0.9 * even) and moved.any() and np.all((ds > sbar[:even]).any(axis=1)[moved]), (case["name"], "swapped rows, s")
    # 3. s shifted by one factor: every row with an entry
    if k >= 2:
        ds = np.abs(np.roll(mod["s"], 1, axis=1) - mod["s"])
        assert np.all((ds > sbar).any(axis=1)[n >= 1]), (case["name"], "s shifted by one factor")
    # 4. k - 1 factors: s of the last factor on every row with an entry, y on every row with two
    if k >= 1:
        less = fc.model(prob, case, params, 0, R, dtype=np.float64, factors=k - 1)
        assert np.all((np.abs(less["s"] - mod["s"])[:, k - 1] > sbar[:, k - 1])[n >= 1]), (case["name"], "k - 1 factors, s")
        assert np.all((np.abs(less["y0"] - mod["y0"]) > ybar)[n >= 2]), (case["name"], "k - 1 factors, y")


# --------------------------------------------------------------------------------------------------------------------- the case table
def _form(rows, lpr):
    """rows_wg_threads and rows_split of fmx_internal.h, restated: 64 or 256 threads, four lane groups per row or one"""
    wg = 64 if rows * lpr < 512 * 256 else 256
    split = 4 if lpr <= 16 and rows * lpr < 1024 * 64 else 1
    return "wide" if wg == 256 else (rc.NARROW4 if split == 4 else rc.NARROW1)


def test_case_table_reaches_every_form_and_instance_and_holds_every_seam_and_extra_once():
    names = [c["name"] for c in fc.CASES]
    assert len(set(names)) == len(names)
    seen, instances, projected = set(), set(), set()
    for child, _ in fc.CHILDREN:
        mine = fc.cases_of(child)
        assert mine, child
        for c in mine:
            lpr = fc.case_lanes(c)
            assert c["kind"] == "hand" or (c["rows"] % 64 == fc.TAIL_ROWS and c["p"] >= rc.MIN_P)
            for op, r0, r1 in fc.case_calls(c):
                n = r1 - r0
                assert 0 <= r0 <= r1 <= (13 if c["kind"] == "hand" else 3 * c["rows"])
                assert rc.static_form(n, lpr) == _form(n, lpr)
                # an engine that is not pinned times wide launches of 65 536 rows or more: its schedule would not be predictable
                assert child in fc.PINNED or not (fc.call_is_wide(c, op, n) and n >= 65536), (child, c["name"])
                for variant in fc.variants_of(c, op, n):
                    want = fc.expected_launches(c, op, n, child, variant)
                    for f, count in enumerate(want):
                        if count:
                            seen.add(f)
                            if f < rc.PULL:
                                instances.add(fc.instance_of(f, c))
                                if op == "project":
                                    projected.add(fc.instance_of(f, c))
    assert seen == set(range(6))
    want = {(rc.NARROW4, t, L) for t in (False, True) for L in (1, 2, 4, 8, 16)}
    want |= {(f, t, L) for f in (rc.NARROW1, rc.WIDE_SERIAL) for t in (False, True) for L in (1, 2, 4, 8, 16, 32, 64) if t or L <= 32}
    assert instances == want and len(want) == 17 + 19, (want - instances, instances - want)
    assert projected == {(rc.WIDE_SERIAL, t, L) for t in (False, True) for L in (1, 2, 4, 8, 16, 32, 64) if t or L <= 32}
    # one predict case per instance, taken from rows_cases.CASES, value kinds alternating; the third range starts at an odd row and ends before the step does
    pred = [c for c in fc.CASES if c["kind"] == "predict"]
    assert len(pred) == 36 and {c["values"] for c in pred} == {False, True}
    by_name = {(c["k"], c["fp64"], c["rows"]) for c in rc.CASES}
    for c in pred:
        assert (c["k"], c["fp64"], c["rows"]) in by_name
        (_, a0, a1), (_, b0, b1), (_, c0, c1) = fc.case_calls(c)
        assert (a0, a1, b0, b1) == (0, c["rows"], c["rows"], 2 * c["rows"]) and c0 % 2 == 1 and c["rows"] < c0 and c1 - c0 == c["limit"] and c1 < 2 * c["rows"]
        assert max(i for i, _ in rc._special_rows(c["rows"])) < c["limit"]   # the long rows lie inside it, two rows off their workgroup's start
    # the extras once per form, the seams once per element type, the hand-made matrix in both
    kinds = lambda kind: [c for c in fc.CASES if c["kind"] == kind]   # noqa: E731
    for form in ("narrow4", "narrow1", "wide"):
        mine = [c for c in kinds("extra") if f"_{form}_" in c["name"]]
        assert len(mine) == 6 and sum(c["w_in_row"] for c in mine) == 1 and sum(not c["keep_w0"] for c in mine) == 1 and sum(not c["keep_w1"] for c in mine) == 1
        assert sum(c["task"] == "regression" for c in mine) == 1 and sum(c["seq"] for c in mine) == 1 and sum(c["k"] == 0 for c in mine) == 1
        assert {c["values"] for c in mine} == {False, True}
        for c in mine:
            f = rc.static_form(c["rows"], fc.case_lanes(c))
            assert (f == "wide") if form == "wide" else rc.FORM_NAMES[f] == form
    assert [(c["k"], c["fp64"]) for c in kinds("seam_predict")] == [(3, False), (2, True)] == [(c["k"], c["fp64"]) for c in kinds("seam_project")]
    for c in kinds("seam_predict"):
        assert fc.case_calls(c) == [("predict", 0, 2 ** 18 + 37)] and fc.expected_launches(c, "predict", 2 ** 18 + 37, "serial", "plain")[rc.WIDE_SERIAL] == 2
    for c in kinds("seam_project"):
        calls = fc.case_calls(c)
        assert calls[0] == ("project", 0, 2 ** 16 + 37) and calls[1] == ("project", 2 ** 16 - 5, 2 ** 16 + 37)
        assert fc.expected_launches(c, "project", 2 ** 16 + 37, "pipelined", "plain")[rc.WIDE_PIPELINED] == 2
    assert [c["fp64"] for c in kinds("hand")] == [False, True]
    assert len(kinds("project")) == 13


def test_hand_made_matrix_holds_what_it_claims():
    prob = fc.hand_problem()
    rp, col = prob["rp"], prob["col"].astype(np.int64)
    rows = [col[rp[i]:rp[i + 1]] for i in range(prob["n"])]
    assert any(len(r) > 1 and np.any(np.diff(r) < 0) for r in rows), "an unsorted row"
    assert any(len(np.unique(r)) < len(r) for r in rows), "a column stored twice"
    e0, e1 = fc.HAND_EMPTY
    assert all(len(rows[i]) == 0 for i in range(e0, e1)) and len(rows[e0 - 1]) and len(rows[e1])
    assert ("predict", 5, 5) in fc.case_calls(fc.CASES[[c["name"] for c in fc.CASES].index("hand_f32_k5")])
    # the generated matrices: the rows that meet the staged chunks' boundaries, in both steps every range reads
    prob = fc.case_problem(next(c for c in fc.CASES if c["name"].startswith("project_f32_k3")))
    lens = np.diff(prob["rp"])
    ghost, late = fc.quiet_features(prob["p"])
    assert not np.isin(prob["col"], ghost).any() and np.isin(prob["col"], late).any()
    for step in (0, 1):
        for i, length in fc._special_rows(997):
            assert lens[step * 997 + i] == length
    assert (lens == 0).sum() > 20 and (lens == 1).sum() > 20
