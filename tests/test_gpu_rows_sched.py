"""The scheduled form of phase 1 (fm_rows_sched_k, fm_batch_kernels.hip: the merged form's walk along a table made once per matrix) gives the bits of the
per-row form (fm_rows_forward_k) under MERGE (DEAL: tests/test_gpu_rows_deal.py), and the device builder of the table (rows_sched_k, fm_ingest.hip) writes what its definition
(tests/rows_sched_model.py) says, word for word.

The switches are read once per process, hence child processes: MERGE under FMX_ROWS_SCHED=2 (wherever the data conditions hold and the rows have a
schedule, whatever the launch's size), compared with an FMX_ROWS_MERGE=0 child by np.array_equal on w0, w, V and the checkpoint after three mini-batch steps, the exchange buffer after
fmx_grad, and the predictions.  The shapes are tests/rows_sched_cases.py's: every matrix is a head tile of 32 768 ordinary rows and the tail under test
as a tile of its own.  fmx_debug_rows_sched_launches says which form ran: a tile takes the scheduled form exactly if every one of its blocks fits the
stage of 144 steps -- told for the tail tile from the model, for the head tile from the export hook (-1 steps: no schedule) -- and is counted as turned
away otherwise (the 37-entry rows); a matrix's schedule is built once.  With the id limit lowered below p nothing is built or run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_sched_model as M
from tests.rows_sched_cases import CASES, HEAD, P, problem, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHED_CHILDREN = [("merge", {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "merge"}, M.MERGE)]
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}, -1)] + SCHED_CHILDREN

_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.rows_sched_cases import CASES, HEAD, P, K, problem, seed_of
out, sched = sys.argv[1], int(sys.argv[2])
lib = L.lib()
def counter():
    a = (ctypes.c_int64 * 3)()
    L.check(lib.fmx_debug_rows_sched_launches(a))
    return np.array(list(a), np.int64)
def export(m, tile, block):
    buf = np.zeros(64 * 160, np.uint32)
    steps = ctypes.c_int64(0)
    info = (ctypes.c_int64 * 4)()
    L.check(lib.fmx_debug_rows_sched_export(m.h, ctypes.c_int64(tile), ctypes.c_int64(block), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(buf)),
                                            ctypes.byref(steps), info))
    return steps.value, buf[:64 * max(steps.value, 0)].reshape(-1, 64).copy(), list(info)
def make(case, solver, seed):
    if case["wir"]:
        os.environ["FMX_W_IN_ROW"] = "1"   # read at engine creation
    try:
        l1 = 1e-3 if solver == L.SOLVER_FTRL else 0.0
        e = engine.Engine(P, task=L.TASK_CLASSIFICATION, solver=solver, num_factor=K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, l1_w1=l1, l1_v=l1,
                          mode=L.MODE_MINIBATCH, batch_rows=2 * HEAD, tile_rows=HEAD)
    finally:
        os.environ.pop("FMX_W_IN_ROW", None)
    assert bool(e.w_in_row()) == bool(case["wir"]), case["name"]
    e.init_normal(seed, 0.0, 0.05)
    return e
for ci, case in enumerate(CASES):
    res = {}
    for t in case["tails"]:
        rp, col, val, y = problem(case, t, seed_of(ci, t))
        m = engine.Matrix.from_csr(rp, col, val, P, y)
        for name, solver in (("sgd", L.SOLVER_SGD), ("ftrl", L.SOLVER_FTRL)):
            if name == "ftrl" and t != case["tails"][-1]:
                continue
            e = make(case, solver, 3000 + ci)
            c0 = counter()
            for _ in range(3):
                e.step(m, 0, 0)
            w0, w, v = e.get_params()
            assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, (case["name"], t, name)
            ck = os.path.join(out, "ck")
            e.save(ck)
            res[f"{name}_{t}_w0"], res[f"{name}_{t}_w"], res[f"{name}_{t}_v"] = np.float64(w0), w, v
            res[f"{name}_{t}_state"] = np.fromfile(ck, np.uint8)
            res[f"{name}_{t}_count"] = counter() - c0
            os.remove(ck)
            if name == "sgd":   # the exchange buffer of one more step's gradient sums, at the parameters three steps left, and the predictions there
                c0 = counter()
                e.grad(m, 0, 0)
                e.sync()
                ptr, n = e.grad_buffer()
                res[f"grad_{t}"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
                res[f"grad_{t}_count"] = counter() - c0
                res[f"predict_{t}"] = e.predict(m, L.LINK_LOGISTIC)
            e.close()
        if sched:
            res[f"head_steps_{t}"], res[f"head_words_{t}"], _ = export(m, 0, 3)
            for b in range((t + 255) // 256):
                res[f"tail_steps_{t}_{b}"], res[f"tail_words_{t}_{b}"], info = export(m, 1, b)
            res[f"info_{t}"] = np.array(info, np.int64)
        m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
if sched:   # the id limit lowered below p: nothing is built, nothing runs in the form
    L.check(lib.fmx_debug_rows_sched_id_limit(ctypes.c_uint32(P - 1)))
    rp, col, val, y = problem(CASES[0], 257, 7)
    m = engine.Matrix.from_csr(rp, col, val, P, y)
    e = make(CASES[0], L.SOLVER_SGD, 1)
    c0 = counter()
    e.step(m, 0, 0)
    e.sync()
    steps, _, _ = export(m, 1, 0)
    np.savez(os.path.join(out, "refused.npz"), count=counter() - c0, steps=np.int64(steps))
    e.close()
    m.close()
    L.check(lib.fmx_debug_rows_sched_id_limit(ctypes.c_uint32(0)))
print("DONE", len(CASES))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs = {}
    for name, env, policy in CHILDREN:
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(d), "1" if policy >= 0 else "0"], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and f"DONE {len(CASES)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        dirs[name] = d
    return dirs


@pytest.fixture(scope="module")
def problems():
    return {(ci, t): problem(c, t, seed_of(ci, t)) for ci, c in enumerate(CASES) for t in c["tails"]}


def _load(runs, child, name):
    with np.load(os.path.join(runs[child], name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _keys(case):
    last = case["tails"][-1]
    keys = [f"sgd_{t}_{q}" for t in case["tails"] for q in ("w0", "w", "v", "state")] + [f"ftrl_{last}_{q}" for q in ("w0", "w", "v", "state")]
    return keys + [f"grad_{t}" for t in case["tails"]] + [f"predict_{t}" for t in case["tails"]]


@pytest.mark.gpu
@pytest.mark.parametrize("child", SCHED_CHILDREN, ids=[c[0] for c in SCHED_CHILDREN])
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_scheduled_form_gives_the_per_row_forms_bits(runs, problems, ci, child):
    name, _, policy = child
    case = CASES[ci]
    a, b = _load(runs, name, case["name"]), _load(runs, "old", case["name"])
    assert np.any(b[f"sgd_{case['tails'][-1]}_v"] != 0.0) and np.any(b[f"predict_{case['tails'][-1]}"] != b[f"predict_{case['tails'][-1]}"][0])
    for key in _keys(case):
        assert np.array_equal(a[key], b[key]), (case["name"], name, key)
    for key in b:
        if key.endswith("_count"):
            assert [int(x) for x in b[key]] == [0, 0, 0], (case["name"], "old", key, b[key])
    for t in case["tails"]:
        rp, col, _, _ = problems[(ci, t)]
        # the device builder against the model, word for word: every block of the tail tile and one of the head tile
        tail = [M.block_schedule(rp, col, HEAD, t, blk, P, policy, 0) for blk in range((t + 255) // 256)]
        tail_fits = all(s.shape[0] <= M.STAGE_STEPS for s in tail)
        for blk, want in enumerate(tail):
            if tail_fits:
                assert int(a[f"tail_steps_{t}_{blk}"]) == want.shape[0] and np.array_equal(a[f"tail_words_{t}_{blk}"], want), (case["name"], name, t, blk)
            else:
                assert int(a[f"tail_steps_{t}_{blk}"]) == -1, (case["name"], name, t, blk)
        head_fits = int(a[f"head_steps_{t}"]) >= 0
        if head_fits:
            assert np.array_equal(a[f"head_words_{t}"], M.block_schedule(rp, col, 0, HEAD, 3, P, policy, 0)), (case["name"], name, t)
        assert head_fits                                          # 120 steps, no bubble
        if case["tail"] == "over37":
            assert not tail_fits
        if case["tail"] == "full36":
            assert tail_fits
        # which form ran: a step or a gradient is two launches, the head tile and the tail tile; one build per matrix that has a tile with a schedule
        took, away = int(head_fits) + int(tail_fits), int(not head_fits) + int(not tail_fits)
        for key, steps in ((f"sgd_{t}_count", 3), (f"grad_{t}_count", 1)) + (((f"ftrl_{t}_count", 3),) if t == case["tails"][-1] else ()):
            builds = 1 if key.startswith("sgd") and took > 0 else 0
            assert [int(x) for x in a[key]] == [took * steps, away * steps, builds], (case["name"], name, key, a[key], took, away)
        if took > 0:
            info = a[f"info_{t}"]
            assert info[0] > 0 and info[2] == policy and info[3] == 0, (case["name"], name, info)


@pytest.mark.gpu
@pytest.mark.parametrize("child", [c[0] for c in SCHED_CHILDREN])
def test_lowered_id_limit_is_refused(runs, child):
    z = _load(runs, child, "refused")
    assert [int(x) for x in z["count"]] == [0, 0, 0] and int(z["steps"]) == -1
