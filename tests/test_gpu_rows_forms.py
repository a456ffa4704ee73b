"""Every form of the mini-batch step's FIRST half (fm_rows_forward_k, fm_rows_forward_dyn_k, fm_rows_forward_flat_k in fm_batch_kernels.hip: per
row the factor sums and the gradient multiplier, per workgroup the w0 partial sums) against the fp64 oracle, through the gradient sums.

fmx_grad leaves GV[F][kp] | GW[F] | CNT[F] (| QV | QW) and the tail {sum M, sum M^2, rows / 4096, rows % 4096} in the exchange buffer;
oracle.batch_sums (fmo_batch_sums, restated vectorised in tests/rows_cases.py and held to it in tests/test_rows_cases_cpu.py) computes the same
quantities in fp64.  Every ELEMENT of the buffer is compared, relative to that element's un-cancelled absolute sum -- a whole-step comparison of
the parameters divides one row's fault by the length of the feature's list, and the wide forms run only where lists are long.  Before every
fmx_grad the oracle takes the engine's own get_params(); between the steps fmx_apply moves the parameters.

The launcher picks the form from the step's row count x lanes per row; the cases (rows_cases.CASES) are the smallest steps that still select
each form, for every (element type, lanes per row) instance compiled, on matrices whose rows meet the staged chunk's boundaries (a 5 000-entry
row, rows of exactly 512 and 2 048 entries, short rows across a boundary), real-valued and one-hot, three steps each: batch 0, batch 1 (a row
count that is no multiple of 64) and a third step truncated by rows_limit.  fmx_debug_rows_launches says which form each of them ran.  Switches
that are read once per process get a fresh child process each (rows_cases.CHILDREN); FMX_ROWS_PULL and FMX_ROWS_FLAT are read per call and run
inside every child on the wide steps.

Bars, per element against its absolute sum: fp32 tables V_RTOL (1e-5, tests/test_gpu_train.py), fp64 tables 1e-11; counts, the row count and the
zeros of features that occur in no active row exact.  The largest ratios seen per form are recorded in profiles/rows_forms_parity.txt."""
import json
import os
import subprocess
import sys

import pytest

from tests import rows_cases as rc
from tests.test_gpu_train import V_RTOL

ROOT = rc.ROOT
WIDE_TOL = 1e-11   # the project's bar for fp64 state (tests/test_gpu_step_forms.py)


def _child(tmp, name, env, cases):
    """One child process over all `cases`; its figures.  A non-zero return code raises, so the fixture that called starts no further child."""
    job = dict(cases=cases, ref=str(tmp), out=str(tmp / f"{name}.json"))
    with open(tmp / f"{name}.job", "w") as f:
        json.dump(job, f)
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
    child_env.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.rows_cases", str(tmp / f"{name}.job")], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    with open(job["out"]) as f:
        out = json.load(f)
    print(f"rows forms child {name}: {out['seconds']:.1f} s for {len(cases)} cases")
    return out["cases"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rows_forms")
    out = {}
    try:
        for name, env in rc.CHILDREN:
            cases = sorted(rc.cases_of(name), key=lambda c: (rc.matrix_key(c), c["name"]))   # one matrix resident at a time
            out[name] = _child(tmp, name, env, cases)
    finally:   # the matrices and references the children share go; their figures (*.json) stay in pytest's temporary directory
        for f in os.listdir(tmp):
            if not f.endswith(".json"):
                os.remove(tmp / f)
    return out


RUNS = [(child, c) for child, _ in rc.CHILDREN for c in rc.cases_of(child)]


def _bars(case, r, what):
    tol = WIDE_TOL if case["fp64"] else V_RTOL
    figures = {q: r[q] for q in ("gv", "gw", "g0", "qv", "qw", "q0") if q in r}
    print(what, figures, "bar", tol)
    assert r["finite"], what
    assert r["cnt_exact"] and r["rows_exact"], what
    assert r["dead"] > 0 and r["dead_zero"], what        # features that occur in no active row: sums exactly 0
    assert r["pad_zero"] and r["spare_zero"] and r["zero_scale_zero"], what
    assert rc.has_q(case) == ("qv" in r), what
    for q, v in figures.items():
        assert v < tol, (what, q, v, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("child,case", RUNS, ids=[f"{child}-{c['name']}" for child, c in RUNS])
def test_gradient_sums_match_the_oracle_in_the_form_that_was_meant_to_run(runs, child, case):
    res = runs[child][case["name"]]
    assert "error" not in res, res["error"]
    lpr = rc.lanes(case["k"], case["fp64"])
    steps = rc.case_steps(case)
    assert len(res["steps"]) == len(steps) == 3
    if case.get("compact"):
        assert res["usable"] and res["rec_elems"] == rc.padded(case["k"], case["fp64"]) * (2 if rc.has_q(case) else 1) + 4
    else:
        assert res["moved"] and res["blocks"] == case["chunks"] and res["w_in_row"] == bool(case["w_in_row"])
    for (batch, limit, active), step in zip(steps, res["steps"]):
        assert step["rows"] == active
        assert list(step["variants"]) == rc.variants_of(case, active)
        for variant, r in step["variants"].items():
            what = (child, case["name"], f"step {batch}", variant)
            _bars(case, r, what)
            # which form ran: one launch per tile of the step, all in the expected slot
            tiles = 1 if not case["tile_rows"] else 3
            want = [0] * 6
            want[rc.expected_form(active, lpr, child, variant)] = tiles
            assert r["launches"] == want, (what, r["launches"], rc.FORM_NAMES)
            if case.get("compact"):
                assert r["ids_ascending"] and r["no_q_slot_zero"], what
        # the claims the code makes: the pull kernel adds in the static kernel's order (same bits, whole buffer); the flat kernel
        # associates a row's sums differently and is held to the bar above only
        v = step["variants"]
        if "pull" in v:
            assert v["pull"]["digest"] == v["plain"]["digest"], (child, case["name"], batch, "pull against the static kernel")


WIDE_BOTH = [c for c in rc.cases_of("serial") if c in rc.cases_of("pipelined")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_BOTH, ids=[c["name"] for c in WIDE_BOTH])
def test_serial_and_pipelined_schedules_give_the_same_bits(runs, case):
    """Both schedules add a row's terms in the same order: the whole exchange buffer bit for bit, in every step (the parameters move between the
    steps by what the buffer holds, so equal buffers keep the runs together) -- and both are the oracle's sums (the test above)."""
    a, b = runs["serial"][case["name"]], runs["pipelined"][case["name"]]
    lpr = rc.lanes(case["k"], case["fp64"])
    for (batch, limit, active), sa, sb in zip(rc.case_steps(case), a["steps"], b["steps"]):
        assert sa["variants"]["plain"]["digest"] == sb["variants"]["plain"]["digest"], (case["name"], batch)
        if rc.static_form(active, lpr) == "wide":   # really two schedules
            assert sa["variants"]["plain"]["launches"][rc.WIDE_SERIAL] > 0 and sb["variants"]["plain"]["launches"][rc.WIDE_PIPELINED] > 0
    if "default" in case["children"]:   # an engine that never measured runs the serial schedule
        d = runs["default"][case["name"]]
        assert [s["variants"]["plain"]["digest"] for s in d["steps"]] == [s["variants"]["plain"]["digest"] for s in a["steps"]]


@pytest.mark.gpu
def test_every_form_and_instance_was_reached(runs):
    """The counters of all children together: all six slots, and every (form, element type, lanes) instance of the static kernel."""
    seen, instances = [0] * 6, set()
    for child, _ in rc.CHILDREN:
        for c in rc.cases_of(child):
            for step in runs[child][c["name"]]["steps"]:
                for r in step["variants"].values():
                    for f, n in enumerate(r["launches"]):
                        seen[f] += n
                        if n and f < rc.PULL:
                            instances.add((min(f, rc.WIDE_SERIAL), c["fp64"], rc.lanes(c["k"], c["fp64"])))
    print(dict(zip(rc.FORM_NAMES, seen)))
    assert all(n > 0 for n in seen), dict(zip(rc.FORM_NAMES, seen))
    assert len(instances) == (5 + 6 + 6) + (5 + 7 + 7), sorted(instances)   # fp32 rows of up to 32 lanes (128 factors), fp64 rows of up to 64
