"""Every runtime form of the mini-batch step's second half (per-feature gradient sums and the update, fm_batch_kernels.hip) against the fp64
oracle -- oracle.SgdMinibatch / FtrlMinibatch / TdapMinibatch on the rows the engine holds -- instead of against one another.

tests/test_gpu_cols_lean.py holds the specialised list-by-list kernel to the general one bit for bit; both share sums_add, embed_store /
embed_take, cols_finish and the directory built in fm_ingest.hip, so a fault in any of those is two identical wrong answers there.  Here:

A. the lean test's 29 cases (same matrices, seeds, init_normal and fmx_train) with fp64 tables (the general kernel on the same directory, inline
   entry, long lists and cols_finish, no rounding room: 1e-11) and with fp32 tables under the launcher's own rule (V_RTOL, and the launch
   counters say the expected lean instance ran); features that occur in no row keep their bits.
B. a hand-made matrix in which chosen features occur in exactly L rows of a step, L on the kernels' own boundaries (a round of four entries, the
   inline first entry, long_min = 64, LIST_SEG = 1024), in three directory regimes, stepped twice in full and once truncated in the middle of
   those lists -- through every form the switches select, each in a fresh child process (the switches are read once per process).
C. a list-by-list tile with more than 2 048 long-list segments: the long-list kernels on the side stream, counted by fmx_debug_long_launches.

Bars: fp32 tables V_RTOL (1e-5, tests/test_gpu_train.py), fp64 tables 1e-11, normwise on V and w, on w0 relative to max(1, |w0|).  The largest
errors seen per form are recorded in profiles/step_forms_parity.txt."""
import json
import os
import subprocess
import sys

import pytest

from tests import step_cases as sc
from tests.test_gpu_train import V_RTOL

ROOT = sc.ROOT
WIDE_TOL = 1e-11   # the project's bar for fp64 state (test_sparse_tiles_with_lists_of_a_few_entries)
TABLES = dict(sgd=1, sgd_l1=2, ftrl=3, tdap=6)   # (V, w) and the solver's optimizer tables in a checkpoint

# name -> environment of the child; "default" also runs every case with state_fp64 = 1
FORMS = [("default", {}),                                  # the launcher's own rule
         ("general", {"FMX_COLS_LEAN": "0"}),              # the general list-by-list kernel
         ("never_ahead", {"FMX_COLS_AHEAD_MIN": "0"}),     # the lean kernel, row ids never one round ahead
         ("always_ahead", {"FMX_COLS_AHEAD_MIN": "1"}),    # ... always
         ("staged", {"FMX_DIRECT_LISTS": "0"}),            # the staged form on every tile
         ("staged_dense", {"FMX_DIRECT_DENSE": "0"}),      # the staged form on dense tiles only
         ("flat", {"FMX_BUF_GATHER": "0"}),                # flat gathers (what runs once the workspace reaches 2 GiB): fp32 goes to the general kernel
         ("side_table", {"FMX_EMBED_MULT": "0"}),          # the multiplier from the side table instead of the S row
         ("main_stream", {"FMX_LONG_SIDE": "0"})]          # the long-list kernels on the main stream


def _child(tmp, name, env, cases, fp64):
    """One child process over all `cases`; its figures.  A non-zero return code raises, so the fixture that called starts no further child."""
    job = dict(cases=cases, ref=str(tmp), out=str(tmp / f"{name}.json"), fp64=bool(fp64))
    with open(tmp / f"{name}.job", "w") as f:
        json.dump(job, f)
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
    child_env.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.step_cases", str(tmp / f"{name}.job")], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    with open(job["out"]) as f:
        out = json.load(f)
    print(f"step forms child {name}: {out['seconds']:.1f} s for {len(cases)} cases")
    return out["cases"]


def _runs(tmp_path_factory, label, forms, cases):
    tmp = tmp_path_factory.mktemp(label)
    try:
        return {name: _child(tmp, name, env, cases, fp64=(name == "default")) for name, env in forms}
    finally:   # the references (p x k doubles per case) go; the children's figures (*.json) stay in pytest's temporary directory
        for f in os.listdir(tmp):
            if not f.endswith(".json"):
                os.remove(tmp / f)


def _within(r, tol, what):
    print(what, {k: r[k] for k in ("err_v", "err_w", "err_w0")}, "bar", tol)
    assert r["finite"] and r["moved"], what
    assert r["err_v"] < tol and r["err_w"] < tol and r["err_w0"] < tol, (what, r["err_v"], r["err_w"], r["err_w0"])


# ------------------------------------------------------------------------------------------------------------------------------------ A
LEAN_CASES = [dict(c, part="A", index=i) for i, c in enumerate(sc.CASES)]


@pytest.fixture(scope="module")
def lean_runs(tmp_path_factory):
    return _runs(tmp_path_factory, "step_forms_a", FORMS[:1], LEAN_CASES)["default"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAN_CASES, ids=[c["name"] for c in LEAN_CASES])
def test_lean_cases_with_fp64_tables_match_the_oracle(lean_runs, case):
    """ST = double: the general kernel over the same directory, inline entry, long lists and cols_finish -- everything the two fp32 kernels share."""
    r = lean_runs[case["name"]]["fp64"]
    assert r["done"] == sc.TOTAL
    _within(r, WIDE_TOL, (case["name"], "fp64"))
    general, plain, ahead = r["counters"][:3]
    assert general == r["steps"] == 4 and plain == 0 and ahead == 0, r["counters"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAN_CASES, ids=[c["name"] for c in LEAN_CASES])
def test_lean_cases_with_fp32_tables_match_the_oracle_on_the_expected_kernel(lean_runs, case):
    r = lean_runs[case["name"]]["fp32"]
    assert r["done"] == sc.TOTAL
    _within(r, V_RTOL, (case["name"], "fp32"))
    general, plain, ahead = r["counters"][:3]
    assert general + plain + ahead == r["steps"] == 4, r["counters"]
    if case["k"] > 16:   # the specialised kernel is compiled for rows of up to 16 padded factors
        assert plain == 0 and ahead == 0, r["counters"]
    else:                # the launcher's rule: dense directories here average 8 entries per list (ahead), uniform columns over 400 000 features one (not)
        assert general == 0, r["counters"]
        if case["name"].startswith("dense_"):
            assert plain == 0, r["counters"]
        if case["name"].startswith("sparse_uniform"):
            assert ahead == 0, r["counters"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", LEAN_CASES, ids=[c["name"] for c in LEAN_CASES])
def test_lean_cases_leave_features_that_occur_in_no_row_alone(lean_runs, case):
    for run in ("fp32", "fp64"):
        r = lean_runs[case["name"]][run]
        assert r["untouched_kept"], (case["name"], run)
    if case["p"] > sc.N * sc.Z:
        assert r["untouched"] > 0


# ------------------------------------------------------------------------------------------------------------------------------------ B
@pytest.fixture(scope="module")
def ladder_runs(tmp_path_factory):
    return _runs(tmp_path_factory, "step_forms_b", FORMS, sc.LADDER_CASES)


def _list_by_list(case, form):
    """Does phase 2 of this case walk list by list (and count in fmx_debug_cols_launches) under this form?"""
    return not (form == "staged" or (form == "staged_dense" and case["regime"] == "dense"))


def _expected_kernels(case, form, wide):
    """(general, plain, ahead) launches of the case's three steps."""
    if not _list_by_list(case, form):
        return (0, 0, 0)
    if wide or case["k"] > 16 or form in ("general", "flat"):
        return (3, 0, 0)
    if form == "never_ahead":
        return (0, 3, 0)
    if form == "always_ahead":
        return (0, 0, 3)
    # the launcher's rule: ids ahead from four entries per list on average -- ~63 (dense, over all p lists) and ~7.6 (inline) against ~1.2 (single)
    return (0, 3, 0) if case["regime"] == "single" else (0, 0, 3)


LADDER_RUNS = [(c, f) for c in sc.LADDER_CASES for f, _ in FORMS] + [(c, "fp64") for c in sc.LADDER_CASES]


@pytest.mark.gpu
@pytest.mark.parametrize("case,form", LADDER_RUNS, ids=[f"{c['name']}-{f}" for c, f in LADDER_RUNS])
def test_ladder_through_every_form_matches_the_oracle(ladder_runs, case, form):
    wide = form == "fp64"
    r = ladder_runs["default" if wide else form][case["name"]]["fp64" if wide else "fp32"]
    # the regime the fillers were meant to set (the builder's own arithmetic: tests/test_step_cases_cpu.py)
    if case["regime"] == "dense":
        assert not r["sparse"] and r["entries0"] >= sc.REGIMES["dense"]["p"]
    elif case["regime"] == "inline":
        assert r["sparse"] and 2 * r["lists0"] <= r["entries0"] < 16 * r["lists0"], (r["lists0"], r["entries0"])
    else:
        assert r["sparse"] and r["entries0"] < 2 * r["lists0"], (r["lists0"], r["entries0"])
    _within(r, WIDE_TOL if wide else V_RTOL, (case["name"], form))
    assert r["untouched_kept"] and r["untouched"] > 0, (case["name"], form)   # the feature that occurs in inactive rows only is one of them
    # the features whose entries are all inactive in the truncated step: the oracle leaves them alone there, and so does the engine -- parameters and
    # every optimizer table bit for bit across that step, and still the oracle's values
    assert r["oracle_ghost_still"] and r["tables"] == TABLES[case["solver"]]
    assert r["ghost_still"], (case["name"], form)
    tol = WIDE_TOL if wide else V_RTOL
    assert r["ghost_err_v"] < tol and r["ghost_err_w"] < tol, (case["name"], form, r["ghost_err_v"], r["ghost_err_w"])
    # the form that was meant to run did run
    assert tuple(r["counters"][:3]) == _expected_kernels(case, "default" if wide else form, wide), (case["name"], form, r["counters"])
    # the lists of 65, 1023, 1024, 1025 and 2049 entries went through the long-list kernels in every step; too few segments for the side stream
    assert r["counters"][3:] == [3, 0], (case["name"], form, r["counters"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", sc.LADDER_CASES, ids=[c["name"] for c in sc.LADDER_CASES])
def test_ladder_forms_that_add_in_the_same_order_give_the_same_bits(ladder_runs, case):
    """Pairs of forms that read the same values and add them in the same order: the whole checkpoint (scalars, parameters, optimizer tables)
    bit for bit.  EMBED_BITS (k = 16) against the side table is not among them by design: its S rows lose two mantissa bits."""
    state = {f: ladder_runs[f][case["name"]]["fp32"]["state_digest"] for f, _ in FORMS}
    assert state["flat"] == state["general"], "flat against buffer-descriptor gathers, both in the general kernel"
    assert state["main_stream"] == state["default"], "the long-list kernels on another stream"
    if case["k"] != 16:   # EMBED_PAD (k = 12, 6) stores the multiplier as is in a padding slot; k = 8 and 32 embed nothing
        assert state["side_table"] == state["default"], "the multiplier from the side table"
    for form in ("general", "never_ahead", "always_ahead"):   # tests/test_gpu_cols_lean.py's claim, on the ladder
        assert state[form] == state["default"], form


# ------------------------------------------------------------------------------------------------------------------------------------ C
@pytest.fixture(scope="module")
def side_runs(tmp_path_factory):
    return _runs(tmp_path_factory, "step_forms_c", [FORMS[0], FORMS[-1]], sc.SIDE_CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sc.SIDE_CASES, ids=[c["name"] for c in sc.SIDE_CASES])
def test_long_lists_on_the_side_stream_match_the_oracle(side_runs, case):
    side, main = side_runs["default"][case["name"]], side_runs["main_stream"][case["name"]]
    for r, run, tol, want in ((side["fp32"], "side", V_RTOL, [0, 2]), (side["fp64"], "side fp64", WIDE_TOL, [0, 2]), (main["fp32"], "main", V_RTOL, [2, 0])):
        assert r["sparse"] and 2 * r["lists0"] <= r["entries0"] < 16 * r["lists0"], (run, r["lists0"], r["entries0"])   # a sparse tile, list by list
        _within(r, tol, (case["name"], run))
        assert r["untouched_kept"] and r["untouched"] > 0, run
        assert r["counters"][0] + r["counters"][1] + r["counters"][2] == 2 and (run == "side fp64" or r["counters"][0] == 0), (run, r["counters"])
        assert r["counters"][3:] == want, (run, r["counters"])   # [main stream, side stream] launch pairs of the two steps
    assert side["fp32"]["state_digest"] == main["fp32"]["state_digest"], "same kernels, another stream: same bits"
