"""The merged form of phase 1 (fm_rows_merged_k, fm_batch_kernels.hip: a lane group walks four rows as one column-ordered stream) gives the bits of
the per-row form it replaces (fm_rows_forward_k): the same seeded runs with FMX_ROWS_MERGE=0 (never) and =2 (wherever the form's other conditions hold,
whatever the launch's row count) must leave identical w0, w, V and checkpoints after three mini-batch steps, identical exchange buffers after
fmx_grad and identical predictions.  The switch is read once per process, hence child processes; a third child runs
with no switch at all: at these sizes the launcher's own rule sends nothing to the merged form.

The form exists on the large-step path only (256-thread workgroups: steps of at least 32 768 rows of four lanes), so every step is two tiles: 32 768
ordinary rows of 30 sorted entries, then a tail tile cut by rows_limit to the row count under test -- 1, 63, 64, 65, 255, 256, 257 and 1 000 rows: a
last workgroup that is partly filled, lane groups with one to four rows, slots without a row.  The tails:
  mixed     rows of 0, 1, 29, 30, 31 and 64 entries next to each other (the longest row no longer tells the host that the blocks fit: the
            device count runs)
  unsorted  rows whose entries are not ascending, with a column stored twice: the row's own order must still decide the bits
  ties      rows g, 64 + g, 128 + g and 192 + g -- the four rows of one lane group -- hold the same columns: every head ties
  p64       64 features: every row meets every other
  overflow  40 entries per row: a 256-row block exceeds the stage, the launch is counted in out[1] and takes the per-row form
  values    real values, and k8, eight factors: not the form's data, nothing is counted
Both table layouts (w beside V, and w in the V row: FMX_W_IN_ROW=1, read at engine creation).  fmx_debug_rows_merged_launches says per operation how
many launches took the merged form and how many were turned away by the stage, so a case that does not reach the form it is meant for fails instead
of comparing the per-row form with itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = 32768                 # rows of the first tile: the smallest step of four-lane rows that takes 256-thread workgroups
TAIL = 1000                  # rows of the tail tile
TAILS = [1, 63, 64, 65, 255, 256, 257, 1000]
STAGE = 9216                 # ids a workgroup of the merged form stages (fm_batch_kernels.hip: MERGE_STAGE)

CASES = [dict(name="mixed", p=6000, k=16, tail="mixed", values=0, wir=0, tails=TAILS, fits=1, form=1),
         dict(name="mixed_wir", p=6000, k=16, tail="mixed", values=0, wir=1, tails=[65, 257, 1000], fits=1, form=1),
         dict(name="unsorted", p=6000, k=16, tail="unsorted", values=0, wir=0, tails=[257, 1000], fits=1, form=1),
         dict(name="ties", p=6000, k=16, tail="ties", values=0, wir=0, tails=[257, 1000], fits=1, form=1),
         dict(name="p64", p=64, k=16, tail="plain", values=0, wir=0, tails=[257, 1000], fits=1, form=1),
         dict(name="p64_wir", p=64, k=16, tail="plain", values=0, wir=1, tails=[1000], fits=1, form=1),
         dict(name="overflow", p=6000, k=16, tail="long", values=0, wir=0, tails=[257, 1000], fits=0, form=1),
         dict(name="values", p=6000, k=16, tail="mixed", values=1, wir=0, tails=[1000], fits=1, form=0),
         dict(name="k8", p=6000, k=8, tail="mixed", values=0, wir=0, tails=[1000], fits=1, form=0)]
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}), ("merged", {"FMX_ROWS_MERGE": "2"}), ("rule", {})]


def tail_lengths(kind):
    if kind == "mixed":
        return np.resize(np.array([0, 1, 29, 30, 31, 64, 30, 0, 64, 31, 1], np.int64), TAIL)
    if kind == "long":
        return np.full(TAIL, 40, np.int64)
    return np.full(TAIL, 30, np.int64)


def problem(case, seed):
    """CSR of HEAD rows of 30 ascending columns (one per stratum of the features), then the case's TAIL rows."""
    rng = np.random.default_rng(seed)
    p = case["p"]
    width = p // 30
    head = (np.arange(30, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (HEAD, 30))
    lens = tail_lengths(case["tail"])
    rows = []
    for r, n in enumerate(lens):
        if case["tail"] == "ties":
            c = np.sort(np.random.default_rng(1000 + r % 64).choice(p, n, replace=False))   # the same columns in rows r, r + 64, r + 128, r + 192
        else:
            c = np.sort(rng.choice(p, n, replace=False))
        if case["tail"] == "unsorted" and n >= 4:
            c = c[::-1].copy() if r % 3 == 0 else rng.permutation(c)   # descending, or no order at all ...
            c[n // 2] = c[1]                                            # ... and one column twice
        rows.append(c)
    col = np.concatenate([head.ravel()] + rows).astype(np.uint32)
    rp = np.zeros(HEAD + TAIL + 1, np.int64)
    rp[1:] = np.cumsum(np.concatenate([np.full(HEAD, 30, np.int64), lens]))
    val = rng.uniform(0.0, 1.0, len(col)).astype(np.float32) if case["values"] else np.ones(len(col), np.float32)
    y = np.where(rng.random(HEAD + TAIL) < 0.5, -1.0, 1.0).astype(np.float32)
    return rp, col, val, y


def test_the_cases_are_what_they_claim():
    """Without a GPU: every block of the cases that must fit does, the overflow case's tail blocks do not (its head tile does), and the mixed tail's
    longest row is too long for the host's shortcut (256 rows of that length would not fit)."""
    for case in CASES:
        rp, col, _, _ = problem(case, 1)
        assert col.max() < case["p"]
        for r0, n in [(0, HEAD)] + [(HEAD, t) for t in case["tails"]]:
            ends = np.minimum(np.arange(0, n, 256) + 256, n)
            most = int(np.max(rp[r0 + ends] - rp[r0 + np.arange(0, n, 256)]))
            assert (most <= STAGE) == bool(case["fits"] or r0 == 0), (case["name"], r0, n, most)
    lens = tail_lengths("mixed")
    assert set(lens[:256]) == {0, 1, 29, 30, 31, 64} and int(lens.max()) * 256 > STAGE


_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.test_gpu_rows_merged import problem, HEAD
cases, out = json.loads(sys.argv[1]), sys.argv[2]
def counter():
    a = (ctypes.c_int64 * 2)()
    L.check(L.lib().fmx_debug_rows_merged_launches(a))
    return np.array(list(a), np.int64)
def make(case, m, solver, seed):
    if case["wir"]:
        os.environ["FMX_W_IN_ROW"] = "1"   # read at engine creation
    try:
        l1 = 1e-3 if solver == L.SOLVER_FTRL else 0.0
        e = engine.Engine(case["p"], task=L.TASK_CLASSIFICATION, solver=solver, num_factor=case["k"], learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, l1_w1=l1, l1_v=l1,
                          mode=L.MODE_MINIBATCH, batch_rows=2 * HEAD, tile_rows=HEAD)
    finally:
        os.environ.pop("FMX_W_IN_ROW", None)
    assert bool(e.w_in_row()) == bool(case["wir"]), case["name"]
    e.init_normal(seed, 0.0, 0.05)
    return e
for i, case in enumerate(cases):
    rp, col, val, y = problem(case, 100 + i)
    m = engine.Matrix.from_csr(rp, col, val, case["p"], y)
    res = {}
    for t in case["tails"]:
        for name, solver in (("sgd", L.SOLVER_SGD), ("ftrl", L.SOLVER_FTRL)):
            e = make(case, m, solver, 3000 + i)
            c0 = counter()
            for _ in range(3):
                e.step(m, 0, HEAD + t)
            w0, w, v = e.get_params()
            assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, (case["name"], t, name)
            ck = os.path.join(out, "ck")
            e.save(ck)
            res[f"{name}_{t}_w0"], res[f"{name}_{t}_w"], res[f"{name}_{t}_v"] = np.float64(w0), w, v
            res[f"{name}_{t}_state"] = np.fromfile(ck, np.uint8)
            res[f"{name}_{t}_count"] = counter() - c0
            os.remove(ck)
            if name == "sgd":   # the exchange buffer of one more step's gradient sums, at the parameters three steps left
                c0 = counter()
                e.grad(m, 0, HEAD + t)
                e.sync()
                ptr, n = e.grad_buffer()
                res[f"grad_{t}"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
                res[f"grad_{t}_count"] = counter() - c0
            e.close()
    e = make(case, m, L.SOLVER_SGD, 3000 + i)
    e.step(m, 0, 0)   # w and w0 off zero
    for name, link in (("raw", L.LINK_NONE), ("logistic", L.LINK_LOGISTIC)):
        c0 = counter()
        res[f"predict_{name}"] = e.predict(m, link)
        res[f"predict_{name}_count"] = counter() - c0
    e.close()
    m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
print("DONE", len(cases))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs = {}
    for name, env in CHILDREN:
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        cases = CASES if name != "rule" else CASES[:1]
        r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(cases), str(d)], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and f"DONE {len(cases)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        dirs[name] = d
    return dirs


def _load(runs, child, case):
    with np.load(os.path.join(runs[child], case["name"] + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _keys(case):
    keys = [f"{s}_{t}_{q}" for t in case["tails"] for s in ("sgd", "ftrl") for q in ("w0", "w", "v", "state")]
    return keys + [f"grad_{t}" for t in case["tails"]] + ["predict_raw", "predict_logistic"]


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["merged"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_merged_form_gives_the_per_row_forms_bits(runs, case, child):
    a, b = _load(runs, child, case), _load(runs, "old", case)
    assert np.any(b[f"sgd_{case['tails'][-1]}_v"] != 0.0) and np.any(b["predict_raw"] != b["predict_raw"][0])
    for key in _keys(case):
        assert np.array_equal(a[key], b[key]), (case["name"], child, key)
    # which form ran.  A step or a gradient is two launches (the head tile, the tail tile), a prediction one launch over all the rows
    for t in case["tails"]:
        for key, steps in ((f"sgd_{t}_count", 3), (f"ftrl_{t}_count", 3), (f"grad_{t}_count", 1)):
            assert [int(x) for x in b[key]] == [0, 0], (case["name"], "old", key, b[key])
            want = [0, 0] if not case["form"] else ([2 * steps, 0] if case["fits"] else [steps, steps])   # overflow: the head tile fits, the tail does not
            assert [int(x) for x in a[key]] == want, (case["name"], child, key, a[key], want)
    for key in ("predict_raw_count", "predict_logistic_count"):
        assert [int(x) for x in b[key]] == [0, 0], (case["name"], "old", key, b[key])
        want = [0, 0] if not case["form"] else ([1, 0] if case["fits"] else [0, 1])
        assert [int(x) for x in a[key]] == want, (case["name"], child, key, a[key], want)


@pytest.mark.gpu
def test_the_launchers_rule_sends_no_small_launch_to_the_merged_form(runs):
    """No switch set: launches of 32 768 rows and fewer do not fill the device, nothing is counted -- not even as turned away by the stage -- and the
    bits are the per-row form's (they are its launches)."""
    case = CASES[0]
    a, b = _load(runs, "rule", case), _load(runs, "old", case)
    for key in _keys(case):
        assert np.array_equal(a[key], b[key]), key
    for key in a:
        if key.endswith("_count"):
            assert [int(x) for x in a[key]] == [0, 0], (key, a[key])
