"""Phase 1's scheduled form under the DEAL policy (fm_rows_sched_k<false, false, true>, fm_batch_kernels.hip; the builder rows_sched_k<WRITE, true>,
fm_ingest.hip) gives the bits of the per-row form, and the device writes the header and the words its definition (tests/rows_deal_model.py) says.

The switches are read once per process, hence two child processes: FMX_ROWS_SCHED=2 FMX_ROWS_SCHED_POLICY=deal (wherever the data conditions hold and the
rows have a schedule, whatever the launch's size) against FMX_ROWS_MERGE=0 (the per-row form), compared by np.array_equal on w0, w, V and the checkpoint
after three mini-batch steps and on the exchange buffer after fmx_grad.  The shapes are tests/rows_deal_cases.py's: tails of 1, 63, 64, 65, 255 and 257
rows with empty rows among them, unsorted rows with a column stored twice, rows of 0..37 entries and of 37 entries (a tile with a block of more than 144
steps is turned away and runs the merged form), and the p = 64 tie case.  fmx_debug_rows_sched_launches says which form ran -- a tile takes the scheduled
form exactly if the model says every one of its blocks fits -- and that the schedule is built in the first step and in no later one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_deal_model as D
from tests import rows_sched_model as M
from tests.rows_deal_cases import CASES, HEAD, problem, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}), ("deal", {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "deal"})]

_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.rows_deal_cases import CASES, HEAD, K, problem, seed_of
out, sched = sys.argv[1], int(sys.argv[2])
lib = L.lib()
def counter():
    a = (ctypes.c_int64 * 3)()
    L.check(lib.fmx_debug_rows_sched_launches(a))
    return np.array(list(a), np.int64)
def export(m, tile, block):
    buf = np.zeros(64 * 161, np.uint32)
    steps = ctypes.c_int64(0)
    info = (ctypes.c_int64 * 4)()
    L.check(lib.fmx_debug_rows_sched_export(m.h, ctypes.c_int64(tile), ctypes.c_int64(block), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(buf)),
                                            ctypes.byref(steps), info))
    return steps.value, buf[:64 * (steps.value + 1)].reshape(-1, 64).copy() if steps.value >= 0 else buf[:0].reshape(0, 64), list(info)
for ci, case in enumerate(CASES):
    res = {}
    for t in case["tails"]:
        rp, col, val, y = problem(case, t, seed_of(ci, t))
        m = engine.Matrix.from_csr(rp, col, val, case["p"], y)
        e = engine.Engine(case["p"], task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3,
                          mode=L.MODE_MINIBATCH, batch_rows=2 * HEAD, tile_rows=HEAD)
        e.init_normal(4000 + ci, 0.0, 0.05)
        c0 = counter()
        e.step(m, 0, 0)
        e.sync()
        res[f"first_{t}_count"] = counter() - c0
        for _ in range(2):
            e.step(m, 0, 0)
        w0, w, v = e.get_params()
        assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, (case["name"], t)
        ck = os.path.join(out, "ck")
        e.save(ck)
        res[f"sgd_{t}_w0"], res[f"sgd_{t}_w"], res[f"sgd_{t}_v"] = np.float64(w0), w, v
        res[f"sgd_{t}_state"] = np.fromfile(ck, np.uint8)
        res[f"sgd_{t}_count"] = counter() - c0
        os.remove(ck)
        c0 = counter()
        e.grad(m, 0, 0)
        e.sync()
        ptr, n = e.grad_buffer()
        res[f"grad_{t}"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
        res[f"grad_{t}_count"] = counter() - c0
        e.close()
        if sched:
            res[f"head_steps_{t}"], res[f"head_words_{t}"], _ = export(m, 0, 3)
            for b in range((t + 255) // 256):
                res[f"tail_steps_{t}_{b}"], res[f"tail_words_{t}_{b}"], info = export(m, 1, b)
            res[f"info_{t}"] = np.array(info, np.int64)
        m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
print("DONE", len(CASES))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs = {}
    for name, env in CHILDREN:
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        r = subprocess.run([sys.executable, "-c", _CHILD, str(d), "0" if name == "old" else "1"], env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"DONE {len(CASES)}" in r.stdout, (name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        dirs[name] = d
    return dirs


def _load(runs, child, name):
    with np.load(os.path.join(runs[child], name + ".npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_deal_gives_the_per_row_forms_bits_and_the_models_words(runs, ci):
    case = CASES[ci]
    p = case["p"]
    a, b = _load(runs, "deal", case["name"]), _load(runs, "old", case["name"])
    assert np.any(b[f"sgd_{case['tails'][-1]}_v"] != 0.0)
    for t in case["tails"]:
        for key in [f"sgd_{t}_{q}" for q in ("w0", "w", "v", "state")] + [f"grad_{t}"]:
            assert np.array_equal(a[key], b[key]), (case["name"], key)
        for key in (f"first_{t}_count", f"sgd_{t}_count", f"grad_{t}_count"):
            assert [int(x) for x in b[key]] == [0, 0, 0], (case["name"], "old", key, b[key])
        rp, col, _, _ = problem(case, t, seed_of(ci, t))
        # the device builder against the model, header and words: every block of the tail tile and one of the head tile
        tail = [D.block_schedule(rp, col, HEAD, t, blk, p) for blk in range((t + 255) // 256)]
        tail_fits = all(words.shape[0] <= M.STAGE_STEPS for _, words, _ in tail)
        for blk, (hdr, words, _) in enumerate(tail):
            if tail_fits:
                got = a[f"tail_words_{t}_{blk}"]
                assert int(a[f"tail_steps_{t}_{blk}"]) == words.shape[0] and got.shape[0] == words.shape[0] + 1, (case["name"], t, blk)
                assert np.array_equal(got[0], hdr) and np.array_equal(got[1:], words), (case["name"], t, blk)
            else:
                assert int(a[f"tail_steps_{t}_{blk}"]) == -1, (case["name"], t, blk)
        assert int(a[f"head_steps_{t}"]) == 120                                   # the head tile: 120 steps, no bubble, whatever the deal
        hdr, words, _ = D.block_schedule(rp, col, 0, HEAD, 3, p)
        assert np.array_equal(a[f"head_words_{t}"][0], hdr) and np.array_equal(a[f"head_words_{t}"][1:], words), (case["name"], t)
        if case["name"] == "over37":
            assert not tail_fits
        if case["name"] in ("mixed", "unsorted", "ties64"):
            assert tail_fits
        # which form ran: a step or a gradient is two launches, the head tile and the tail tile; the build happens in the first step and in no later one
        took, away = 1 + int(tail_fits), int(not tail_fits)
        assert [int(x) for x in a[f"first_{t}_count"]] == [took, away, 1], (case["name"], t, a[f"first_{t}_count"])
        assert [int(x) for x in a[f"sgd_{t}_count"]] == [3 * took, 3 * away, 1], (case["name"], t, a[f"sgd_{t}_count"])
        assert [int(x) for x in a[f"grad_{t}_count"]] == [took, away, 0], (case["name"], t, a[f"grad_{t}_count"])
        info = a[f"info_{t}"]
        assert info[0] > 0 and info[2] == D.DEAL and info[3] == 0, (case["name"], info)
