"""CPU self-checks of tests/rows_cases.py: the vectorised restatement of fmo_batch_sums is the oracle's, the hand-shaped matrices have the rows they
claim to have where the kernels' chunk boundaries fall, and the case table reaches every form and every compiled instance it says it does."""
import numpy as np
import pytest

import oracle
from tests import rows_cases as rc


def _small_case(**opts):
    return rc._case("cpu", opts.pop("k", 5), False, 997, opts.pop("values", True), **opts)


@pytest.mark.parametrize("opts", [dict(), dict(values=False), dict(task="regression"), dict(keep_w0=0, keep_w1=0, k=3), dict(solver="ftrl_sum", k=8)],
                         ids=["val", "onehot", "regression_clamped", "no_w0_no_w1", "ftrl_sum"])
def test_restatement_equals_the_oracles_batch_sums(opts):
    """Every sum of sums_reference against oracle.batch_sums (fmo_batch_sums) on the same rows and parameters: 1e-13 of the element's absolute sum
    (measured: 2e-15), counts equal, and an element the oracle leaves at 0 is 0."""
    case = _small_case(**opts)
    prob = rc.problem(case["rows"], case["p"], case["values"], 5)
    y = rc.labels(prob["n"], 5, case["task"])
    w0, w, v = rc.start_params(case["p"], case["k"], 5, case["task"])
    P = rc.oracle_params(case)
    X = oracle.Matrix(prob["rp"], prob["col"], prob["val"], prob["p"])
    for b0, b1 in ((0, 997), (997, 997 + 601)):
        # the multiplier as the tests take it (oracle.predict_batch, then oracle.grad_mult) against fmo_batch_sums' own route (fmo_predict row by
        # row, another association of the score): 1e-13 of the multiplier's own un-cancelled scale, |y_hat| + |y| for regression's y_hat - y
        m = rc.multipliers(P, prob, y, w0, w, v, b0, b1)
        scores = np.array([oracle.predict(P, X, w0, w, v.ravel(), i)[0] for i in range(b0, b1)])
        m_rows = np.array([oracle.grad_mult(P, float(s), float(y[b0 + i]))[0] for i, s in enumerate(scores)])
        assert np.max(np.abs(m - m_rows) / (np.abs(scores) + np.abs(y[b0:b1]) if case["task"] == "regression" else 1.0)) < 1e-13
        ref = rc.sums_reference(prob, case["k"], m_rows, w0, w, v, b0, b1)
        acc = oracle.batch_sums(P, X, y, w0, w, v.ravel(), b0, b1)
        k, p = case["k"], case["p"]
        assert np.array_equal(ref["cw"], acc["cw"]) and ref["rows"] == b1 - b0
        worst = max(rc.worst_ratio(ref["Gv"], acc["Gv"].reshape(k, p), ref["Av"]), rc.worst_ratio(ref["Qv"], acc["Qv"].reshape(k, p), ref["AQv"]),
                    rc.worst_ratio(ref["Gw"], acc["Gw"], ref["Aw"]), rc.worst_ratio(ref["Qw"], acc["Qw"], ref["AQw"]),
                    abs(ref["G0"] - acc["G0"]) / ref["A0"], abs(ref["Q0"] - acc["Q0"]) / ref["Q0"])
        print("restatement against fmo_batch_sums:", worst)
        assert worst < 1e-13
        dead = acc["cw"] == 0
        assert dead.sum() > 0 and np.all(ref["Gv"][:, dead] == 0) and np.all(ref["Gw"][dead] == 0) and np.all(ref["Av"][:, dead] == 0)
        # the absolute sums bound the sums they scale
        assert np.all(np.abs(ref["Gv"]) <= ref["Av"] * (1 + 1e-12)) and np.all(np.abs(ref["Gw"]) <= ref["Aw"] * (1 + 1e-12))
        if case["task"] == "regression":   # both clamps take part
            yh = oracle.predict_batch(P, oracle.Matrix(prob["rp"][b0:b1 + 1] - prob["rp"][b0], prob["col"][prob["rp"][b0]:prob["rp"][b1]],
                                                       prob["val"][prob["rp"][b0]:prob["rp"][b1]], p), w0, w, v.ravel())
            assert np.sum(yh > 0.3) > 10 and np.sum(yh < -0.2) > 10


def test_a_planted_fault_in_one_row_shows_per_element():
    """One row's factor sums lose their last entry: the per-element figure of the features of that row leaves the bar by orders of magnitude."""
    case = _small_case(k=16)
    prob = rc.problem(case["rows"], case["p"], True, 5)
    y = rc.labels(prob["n"], 5, case["task"])
    w0, w, v = rc.start_params(case["p"], 16, 5)
    m = rc.multipliers(rc.oracle_params(case), prob, y, w0, w, v, 0, 997)
    good = rc.sums_reference(prob, 16, m, w0, w, v, 0, 997)
    row = 300
    assert prob["rp"][row + 1] - prob["rp"][row] >= 3
    bad_prob = dict(prob, val=prob["val"].copy())
    # the same sums with the row's last entry missing from s: restated as that entry's x = 0 in a copy, its own gradient terms left out of the comparison
    last = int(prob["rp"][row + 1]) - 1
    bad_prob["val"][last] = 0.0
    bad = rc.sums_reference(bad_prob, 16, m, w0, w, v, 0, 997)
    cols = prob["col"][prob["rp"][row]:last].astype(np.int64)
    ratio = np.abs(bad["Gv"][:, cols] - good["Gv"][:, cols]) / good["Av"][:, cols]
    assert ratio.max() > 100 * 1e-5


@pytest.mark.parametrize("values", [False, True], ids=["onehot", "val"])
@pytest.mark.parametrize("rows", [997, 2085])
def test_matrices_hold_the_rows_that_meet_the_chunk_boundaries(rows, values):
    prob = rc.problem(rows, rc.MIN_P + 257, values, 3)
    rp, col, val = prob["rp"], prob["col"], prob["val"]
    assert len(rp) == 3 * rows + 1 and rp[-1] == len(col) == len(val)
    lens = np.diff(rp)
    row_of = np.repeat(np.arange(prob["n"]), lens)
    assert np.all((np.diff(col.astype(np.int64)) > 0) | (np.diff(row_of) > 0)), "columns ascend inside every row"
    assert np.all(val == 1.0) != values
    for s in range(3):
        step = lens[s * rows:(s + 1) * rows]
        assert np.sum(step == 0) > 5 and np.sum(step == 1) > 5 and 10 < np.median(step) < 14
        assert step[259] == rc.LONG_ROW and step[385] == rc.NARROW_CHUNK and step[512] == rc.WIDE_CHUNK and step[0] == 508 and step[256] == 2044
        start = rp[s * rows:(s + 1) * rows + 1] - rp[s * rows]
        # one-wave workgroups of 2, 4, ... 64 rows and wide ones of 4 .. 256: some row lies across a multiple of the chunk, counted from the
        # workgroup's first entry, in a workgroup of every size; the exact-chunk rows end on one where they start a workgroup
        for chunk, sizes in ((rc.NARROW_CHUNK, (2, 4, 8, 16, 32, 64)), (rc.WIDE_CHUNK, (4, 8, 16, 32, 64, 128, 256))):
            for rpw in sizes:
                first = start[(np.arange(rows) // rpw) * rpw]
                a, b = start[:-1] - first, start[1:] - first
                across = (a // chunk != (b - 1) // chunk) & (b > a)
                short = across & (step <= 16)
                assert across.sum() >= 2 and short.sum() >= 1, (chunk, rpw)
        assert (start[513] - start[512]) == rc.WIDE_CHUNK and 512 % 256 == 0
    # features that occur nowhere, and features whose only rows are the last ones of every step: inactive in every truncated step
    ghost, late = rc.quiet_features(prob["p"])
    assert len(ghost) >= 60 and not np.isin(col, ghost).any()
    where = row_of[np.isin(col, late)] % rows
    assert len(where) == 3 * len(late) and where.min() == rows - rc.LATE_ROWS
    assert np.array_equal(np.unique(col[np.isin(col, late)]), late)
    assert all(c["limit"] <= c["rows"] - rc.LATE_ROWS for c in rc.CASES + rc.COMPACT_CASES)
    # the truncated step keeps every hand-placed row active
    assert all(max(i for i, _ in rc._special_rows(c["rows"])) < c["limit"] for c in rc.CASES + rc.COMPACT_CASES)


def test_long_rows_keep_a_multiplier_worth_testing():
    """A saturated score would switch the long rows' gradient off: at the start parameters every hand-placed long row's multiplier stays away from 0."""
    for k in (3, 16, 128):
        case = rc._case("cpu", k, False, 997, True)
        prob = rc.problem(997, case["p"], True, 3)
        y = rc.labels(prob["n"], 1, "classification")
        m = rc.multipliers(rc.oracle_params(case), prob, y, *rc.start_params(case["p"], k, 1), 0, 997)
        for i, length in rc._special_rows(997):
            if length >= 500:
                assert 0.02 < abs(m[i]) < 0.98, (k, i, length, m[i])


def test_case_table_reaches_every_form_and_every_compiled_instance():
    names = [c["name"] for c in rc.CASES + rc.COMPACT_CASES]
    assert len(set(names)) == len(names)
    seen, instances = set(), set()
    for child, _ in rc.CHILDREN:
        mine = rc.cases_of(child)
        assert mine, child
        for c in mine:
            lpr = rc.lanes(c["k"], c["fp64"])
            assert c["rows"] % 64 != 0 and c["p"] >= rc.MIN_P
            for _, _, active in rc.case_steps(c):
                for variant in rc.variants_of(c, active):
                    f = rc.expected_form(active, lpr, child, variant)   # (asserts that an unpinned step is below the tuner's threshold)
                    seen.add(f)
                    if f in (rc.NARROW4, rc.NARROW1, rc.WIDE_SERIAL, rc.WIDE_PIPELINED):
                        instances.add((min(f, rc.WIDE_SERIAL), c["fp64"], lpr))
    assert seen == set(range(6))
    # launch_rows_t compiles fm_rows_forward_k for L lanes per row where L * SPLIT fits the workgroup: both element types
    # that an engine can reach (at most 128 factors: 32 lanes of fp32, 64 of fp64)
    want = {(rc.NARROW4, t, L) for t in (False, True) for L in (1, 2, 4, 8, 16)}
    want |= {(f, t, L) for f in (rc.NARROW1, rc.WIDE_SERIAL) for t in (False, True) for L in (1, 2, 4, 8, 16, 32, 64) if t or L <= 32}
    assert all(c["k"] <= 128 for c in rc.CASES + rc.COMPACT_CASES)
    assert instances == want, (want - instances, instances - want)
    # each of them with real values and with one-hot rows
    both = {}
    for c in rc.CASES:
        both.setdefault(c["name"].rsplit("_", 1)[0], set()).add(c["values"])
    plain = [n for n in both if not any(t in n for t in ("_wir", "_regr", "_now0", "_now1", "_ftrlsum", "_tiles", "_chunks"))]
    assert plain and all(both[n] == {False, True} for n in plain)
    # the three multiplier-embedding modes, the w-in-row stride, and a truncated step that changes form
    modes = {rc.embed_mode(c["k"], c["fp64"], child) for child, _ in rc.CHILDREN for c in rc.cases_of(child) if not c["fp64"]}
    assert modes == {"none", "pad", "bits"}
    assert {rc.embed_mode(k, False, "embed_wide") for k in (24, 48)} == {"pad"} and {rc.embed_mode(k, False, "embed_wide") for k in (32, 64)} == {"bits"}
    assert any(c["w_in_row"] and rc.padded(c["k"], False) <= 16 for c in rc.CASES)
    c = next(c for c in rc.CASES if c["name"] == "narrow1_f32_k3_64k_val")
    assert [rc.expected_form(a, 1, "default") for _, _, a in rc.case_steps(c)] == [rc.NARROW1, rc.NARROW1, rc.NARROW4]
    # the headline instance: fp32, k = 16, 32 768 + 37 rows, wide in all three steps
    c = next(c for c in rc.CASES if c["name"] == "wide_f32_k16_val")
    assert c["rows"] == 32805 and [rc.static_form(a, 4) for _, _, a in rc.case_steps(c)] == ["wide"] * 3 and c["limit"] % 64 != 0


def test_launcher_rule_restated():
    assert rc.static_form(1024, 4) == rc.NARROW4 and rc.static_form(16384, 4) == rc.NARROW1 and rc.static_form(16383, 4) == rc.NARROW4
    assert rc.static_form(32767, 4) == rc.NARROW1 and rc.static_form(32768, 4) == "wide"
    assert rc.static_form(1000, 32) == rc.NARROW1 and rc.static_form(2048, 64) == "wide"
    assert [rc.lanes(k, False) for k in (3, 6, 8, 12, 16, 24, 32, 48, 64, 128)] == [1, 2, 2, 4, 4, 8, 8, 16, 16, 32]
    assert [rc.lanes(k, True) for k in (2, 4, 8, 16, 32, 64, 128)] == [1, 2, 4, 8, 16, 32, 64]
