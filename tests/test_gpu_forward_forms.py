"""Every form of the FORWARD-ONLY face of phase 1 (the TRAIN = false instances of fm_rows_forward_k, fm_rows_forward_dyn_k, fm_rows_forward_flat_k in
fm_batch_kernels.hip: link_apply and the qout stores; launch_rows_forward's slab loop, the form chosen from the call's row count, fixed_schedule)
against a long-double model of the same operation, per row: fmx_predict_device raw and under the task's link, fmx_project_device's base and s.

tests/forward_cases.py holds the cases (the smallest calls that still select each form, for every (element type, lanes per row) instance, over three
row ranges each: aligned, second step, and an odd start with a partly filled last workgroup), the model, the derived bars (any-order fp64 bounds, written
out in its docstring) and the child; tests/test_forward_cases_cpu.py holds the model to a Fraction loop and shows the bars both wide enough for a correct
implementation and tight enough for a planted fault.  fmx_debug_rows_forward_launches says which form each call ran.  Switches that are read once per
process get a fresh child each (forward_cases.CHILDREN); FMX_ROWS_PULL and FMX_ROWS_FLAT are read per call and run inside every child on the wide calls.
Every output sits between guard zones pre-filled with one NaN: a row left out, or a store outside [r0, r1), shows.

The largest shares seen per form are recorded in profiles/forward_forms_parity.txt."""
import json
import os
import subprocess
import sys

import pytest

from tests import forward_cases as fc
from tests import rows_cases as rc

ROOT = fc.ROOT


def _child(tmp, name, env, cases):
    """One child process over all `cases`; its figures.  A non-zero return code raises, so the fixture that called starts no further child."""
    job = dict(cases=cases, ref=str(tmp), out=str(tmp / f"{name}.json"))
    with open(tmp / f"{name}.job", "w") as f:
        json.dump(job, f)
    child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
    child_env.update(env)
    r = subprocess.run([sys.executable, "-m", "tests.forward_cases", str(tmp / f"{name}.job")], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    with open(job["out"]) as f:
        out = json.load(f)
    print(f"forward forms child {name}: {out['seconds']:.1f} s for {len(cases)} cases, "
          f"{sum(c.get('model_seconds', 0.0) for c in out['cases'].values()):.1f} s of them in the model")
    return out["cases"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("forward_forms")
    out = {}
    try:
        for name, env in fc.CHILDREN:
            cases = sorted(fc.cases_of(name), key=lambda c: (fc.matrix_key(c), c["name"]))   # one matrix resident at a time
            out[name] = _child(tmp, name, env, cases)
    finally:   # the matrices and models the children share go; their figures (*.json) stay in pytest's temporary directory
        for f in os.listdir(tmp):
            if not f.endswith(".json"):
                os.remove(tmp / f)
    return out


RUNS = [(child, c) for child, _ in fc.CHILDREN for c in fc.cases_of(child)]
SHARES = {"predict": ("y", "logistic"), "project": ("base0", "base1", "s", "w0_step")}


def _calls(runs, child, case):
    res = runs[child][case["name"]]
    assert "error" not in res, res["error"]
    calls = fc.case_calls(case)
    assert len(res["calls"]) == len(calls)
    for (op, r0, r1), call in zip(calls, res["calls"]):
        assert (call["op"], call["r0"], call["r1"]) == (op, r0, r1)
        assert list(call["variants"]) == fc.variants_of(case, op, r1 - r0)
        yield op, r0, r1, call["variants"]


@pytest.mark.gpu
@pytest.mark.parametrize("child,case", RUNS, ids=[f"{child}-{c['name']}" for child, c in RUNS])
def test_every_row_matches_the_model_in_the_form_that_was_meant_to_run(runs, child, case):
    res = runs[child][case["name"]]
    assert "error" not in res, res["error"]
    assert res["params_held"] and res["w_in_row"] == bool(case["w_in_row"])
    for op, r0, r1, variants in _calls(runs, child, case):
        for variant, r in variants.items():
            what = (child, case["name"], op, r0, r1, variant)
            figures = {q: r[q] for q in SHARES[op] if q in r}
            print(what, figures, "of the bar")
            # no row is left out: every row of the range was compared (or held to an exact zero), and nothing outside the range was written
            assert r["rows"] == r["compared"] == r1 - r0, what
            assert r["guards"], what
            for q, v in figures.items():
                assert v <= 1.0, (what, q, v)
            # exact: an empty row is [k0] w0 and s = 0 in every bit; a row whose absolute sum is 0 is an exact zero
            assert r["empty_exact"] and r["zero_bar_zero"], what
            if case["kind"] != "hand" and r1 - r0 > 600:
                assert r["empty"] > 0, what
            if op == "predict":
                if case["task"] == "regression":
                    assert r["clamp_exact"] and "logistic" not in r, what
                    if r1 - r0 > 600:
                        assert r["clamped_low"] > 10 and r["clamped_high"] > 10, what   # both clamps act
                else:
                    assert "logistic" in r, what
                assert r["launches"] == fc.expected_launches(case, op, r1 - r0, child, variant), (what, r["launches"], rc.FORM_NAMES)
            else:
                assert r["s_same"] and r["same_without_bias"], what   # the bias changes base alone; without one, nothing
                want = fc.expected_launches(case, op, r1 - r0, child, variant)
                assert r["launches"] == want and r["launches_w0"] == want, (what, r["launches"], r["launches_w0"], rc.FORM_NAMES)
        # the claim the code makes: the pull kernel adds in the static kernel's order -- the same bits, links included; the flat kernel associates a
        # row's sums differently and is held to the bars above only
        if "pull" in variants:
            assert variants["pull"]["digest"] == variants["plain"]["digest"], (child, case["name"], op, r0, r1, "pull against the static kernel")


PROJECTED = [(child, c) for child, c in RUNS if any(op == "project" for op, _, _ in fc.case_calls(c))]


@pytest.mark.gpu
@pytest.mark.parametrize("child,case", PROJECTED, ids=[f"{child}-{c['name']}" for child, c in PROJECTED])
def test_a_projected_rows_bits_do_not_depend_on_the_range(runs, child, case):
    """fixed_schedule: fmx_project takes 256-thread workgroups and one lane group per row whatever the call's row count, so base and s of a row are the
    same bits from every range that holds it -- three overlapping pairs of ranges per case, across the 2^16-row slab seam where the case has one."""
    pairs = 0
    for op, r0, r1, variants in _calls(runs, child, case):
        if op == "project":
            same = variants["plain"]["same_as"]
            assert all(same.values()), (child, case["name"], r0, r1, same)
            pairs += len(same)
    assert pairs >= 3, pairs


WIDE_ALL = [c for c in fc.CASES if "serial" in c["children"]]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WIDE_ALL, ids=[c["name"] for c in WIDE_ALL])
def test_serial_pipelined_and_default_children_give_the_same_bits(runs, case):
    """Both request schedules add a row's terms in the same order: every output of every call and variant bit for bit -- and an engine that never
    measured runs the serial one."""
    a, b = runs["serial"][case["name"]], runs["pipelined"][case["name"]]
    digests = lambda res: [[call["variants"][v]["digest"] for v in call["variants"]] for call in res["calls"]]   # noqa: E731
    assert digests(a) == digests(b) and len(a["calls"]) == len(fc.case_calls(case))
    two = 0
    for (op, r0, r1), ca, cb in zip(fc.case_calls(case), a["calls"], b["calls"]):
        if fc.call_is_wide(case, op, r1 - r0):   # really two schedules
            assert ca["variants"]["plain"]["launches"][rc.WIDE_SERIAL] > 0 and cb["variants"]["plain"]["launches"][rc.WIDE_PIPELINED] > 0
            two += 1
    assert two > 0
    if "default" in case["children"]:
        assert digests(runs["default"][case["name"]]) == digests(a)


@pytest.mark.gpu
def test_every_form_and_instance_was_reached_by_forward_only_launches(runs):
    """The counters of all children together: all six slots, and every (form, element type, lanes) instance of the static kernel; the projection
    reaches every wide instance on its own."""
    seen, instances, projected = [0] * 6, set(), set()
    for child, case in RUNS:
        for call in runs[child][case["name"]]["calls"]:
            for r in call["variants"].values():
                for f, n in enumerate(r["launches"]):
                    seen[f] += n
                    if n and f < rc.PULL:
                        instances.add(fc.instance_of(f, case))
                        if call["op"] == "project":
                            projected.add(fc.instance_of(f, case))
    print(dict(zip(rc.FORM_NAMES, seen)))
    assert all(n > 0 for n in seen), dict(zip(rc.FORM_NAMES, seen))
    assert len(instances) == (5 + 6 + 6) + (5 + 7 + 7), sorted(instances)   # fp32 rows of up to 32 lanes (128 factors), fp64 rows of up to 64
    assert len(projected) == 6 + 7, sorted(projected)
