"""The specialised list-by-list phase-2 kernel (fm_cols_lean_k: row ids one round ahead, multiplier bits through DPP, launch flags
compiled in) gives the bits of the general kernel it replaces: the same seeded mini-batch training with FMX_COLS_LEAN unset and =0
(read once per process, hence child processes) must leave identical w0, w, V and optimizer tables.

The cases reach every branch of the new kernel: EMBED_BITS (k = 16), EMBED_PAD in a quad (k = 12) and in a pair (k = 6), no embedding
(k = 32); one-hot and real values; SGD, SGD with L1, FTRL, TDAP; every run ends in a truncated batch (rows_active below the tile);
Zipf columns (long lists beside short ones); dense directories (entries of a tile >= p: ids one round ahead) and sparse ones with the
first entry inline (Zipf, >= 2 entries per list) and without (uniform over a large p, one-entry lists: the parent's schedule).

Four runs of every case: the launcher's own rule, the ids never ahead (FMX_COLS_AHEAD_MIN=0: the plain loop's second and later rounds on
the dense cases), always ahead (=1: the look-ahead on one-entry lists and on lanes without a list) and the general kernel
(FMX_COLS_LEAN=0).  Each child reports, per case, which kernels its list-by-list launches went to (fmx_debug_cols_launches), so a case
that does not reach the kernel it is meant for fails instead of comparing the general kernel with itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from tests.step_cases import BATCH, CASES, N, TOTAL, Z   # the case list is shared with tests/test_gpu_step_forms.py, which holds the same cases to the oracle

_CHILD = r"""
import ctypes, json, os, sys
import numpy as np
from fmwr_amd import engine, _lib as L
cases, out = json.loads(sys.argv[1]), sys.argv[2]
N, Z, BATCH, TOTAL = (int(x) for x in sys.argv[3:7])
def launches():
    out = (ctypes.c_int64 * 3)()
    L.check(L.lib().fmx_debug_cols_launches(out))
    return np.array(list(out), np.int64)
for i, c in enumerate(cases):
    before = launches()
    m = engine.Matrix.synthetic_iid(N, c["p"], Z, 1000 + i, law=L.COLUMNS_ZIPF if c["law"] == "zipf" else L.COLUMNS_UNIFORM)
    if c["values"]:
        m.synthetic_values(2000 + i)
    l1 = 0.0 if c["solver"] == "sgd" else 1e-3
    solver = {"sgd": L.SOLVER_SGD, "sgd_l1": L.SOLVER_SGD, "ftrl": L.SOLVER_FTRL, "tdap": L.SOLVER_TDAP}[c["solver"]]
    e = engine.Engine(c["p"], task=L.TASK_CLASSIFICATION, solver=solver, num_factor=c["k"], learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, l1_w1=l1, l1_v=l1,
                      mode=L.MODE_MINIBATCH, batch_rows=BATCH)
    e.init_normal(3000 + i, 0.0, 0.05)
    done = e.train(m, TOTAL)
    assert done == TOTAL, (c["name"], done)
    w0, w, v = e.get_params()
    assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, c["name"]
    ck = os.path.join(out, c["name"] + ".ck")
    e.save(ck)
    np.savez(os.path.join(out, c["name"] + ".npz"), w0=np.float64(w0), w=w, v=v, state=np.fromfile(ck, np.uint8), launches=launches() - before)
    os.remove(ck)
print("DONE", len(cases))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs = {}
    for name, env in (("lean", {}), ("never_ahead", {"FMX_COLS_AHEAD_MIN": "0"}), ("always_ahead", {"FMX_COLS_AHEAD_MIN": "1"}), ("general", {"FMX_COLS_LEAN": "0"})):
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if k not in ("FMX_COLS_LEAN", "FMX_COLS_AHEAD_MIN", "FMX_BUF_GATHER", "FMX_EMBED_MULT", "FMX_EMBED_MAX_KP",
                                                                       "FMX_DIRECT_LISTS", "FMX_DIRECT_DENSE")}
        child_env.update(env)
        r = subprocess.run([sys.executable, "-c", _CHILD, json.dumps(CASES), str(d), str(N), str(Z), str(BATCH), str(TOTAL)],
                           env=child_env, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and f"DONE {len(CASES)}" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])
        dirs[name] = d
    return dirs


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_lean_kernel_gives_the_general_kernels_bits(runs, case):
    b = np.load(os.path.join(runs["general"], case["name"] + ".npz"))
    assert np.any(b["v"] != 0.0)
    lean_rows = case["k"] <= 16   # the specialised kernel is compiled for rows of up to 16 padded factors
    general, plain, ahead = (int(x) for x in b["launches"])
    assert general > 0 and plain == 0 and ahead == 0, (case["name"], b["launches"])
    for run in ("lean", "never_ahead", "always_ahead"):
        a = np.load(os.path.join(runs[run], case["name"] + ".npz"))
        for key in ("w0", "w", "v", "state"):   # state: the checkpoint, i.e. the scalars, the parameters and every optimizer table
            assert np.array_equal(a[key], b[key]), (case["name"], run, key)
        g, p, h = (int(x) for x in a["launches"])
        assert g + p + h == general, (case["name"], run, a["launches"])
        if not lean_rows:
            assert p == 0 and h == 0, (case["name"], run, a["launches"])
        elif run == "never_ahead":
            assert g == 0 and h == 0, (case["name"], run, a["launches"])
        elif run == "always_ahead":
            assert g == 0 and p == 0, (case["name"], run, a["launches"])
        else:   # the launcher's rule: dense directories here average 8 entries per list (ahead), uniform columns over 400 000 features one (not)
            assert g == 0, (case["name"], run, a["launches"])
            if case["name"].startswith("dense_"):
                assert p == 0, (case["name"], a["launches"])
            if case["name"].startswith("sparse_uniform"):
                assert h == 0, (case["name"], a["launches"])
