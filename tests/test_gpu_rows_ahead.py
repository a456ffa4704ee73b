"""Phase 1's look-ahead walk (fm_rows_sched_k<.., AHEAD>, FMX_ROWS_AHEAD; fm_batch_kernels.hip) changes no bit at any depth.

A walk of depth d requests step t + d - 1 before it takes step t's sums, so what can go wrong is at a block's two ends: the prologue of a block shorter than
the look-ahead, and the requests past the last step, which must be bubbles (no request, no sum) whatever the stage holds there.

The switches are read once per process, hence child processes, each under its own timeout.  Fifteen of them, in two rounds of at most eight -- so never
more than eight GPU processes at a time -- and not eight in all: the depth, the pace, the policy and the stamping instance are four process-wide switches,
four depths are built, and one process can vary only the planted target (a hook, not a switch); the per-row form, "DEAL and MERGE", "paced and unpaced"
and "once through the stamping instance" for each of four depths need three processes per depth.  What the three cover between them: DEAL and MERGE, the
paced and the unpaced product instance and the stamping one, and the planted targets far ahead and far behind (under DEAL, whose clock check is MERGE's:
the policy changes the words a block holds, not the walk).  Per depth d, all under FMX_ROWS_SCHED=2:
  deal    DEAL, FMX_ROWS_PACE=4: three engines -- no planted target, one far ahead (0xFFFFFFFF: every wave sleeps the longest length at every look at the clock)
          and one far behind (1: none ever sleeps)
  merge   MERGE, FMX_ROWS_PACE=4, through the stamping instance (FMX_ROWS_PACE_TRACE=1)
  deal0   DEAL, FMX_ROWS_PACE=0: the unpaced instance
twice more with FMX_ROWS_AHEAD unset (the compiled default, depth 2, paced or not), under FMX_ROWS_PACE=4 and =0;
and once the per-row form (FMX_ROWS_MERGE=0), to which every engine of every child is compared by np.array_equal on w0, w, V and the checkpoint after
three steps on the head tile and three on head and tail, and on the exchange buffer after fmx_grad.

Inputs: every case and tail of tests/rows_deal_cases.py (empty rows, lane groups of one to four rows, bubbles at the end of short lane groups, the 144-step
edge, the tile that is turned away), and a ladder of tail tiles of ONE block of exactly N steps, N = 0, 1, 2, AHEAD - 1, AHEAD, AHEAD + 1 over the built
depths (0 .. 5), 143 and 144.  How N follows from the models: under MERGE (tests/rows_sched_model.py) a lane group takes one entry per step and never
pauses, so T_b is the largest lane-group total; rows 64 s + g belong to lane group g.  N <= 5: sixteen rows of i mod (N + 1) ascending entries -- one row
per lane group, the longest N.  DEAL (tests/rows_deal_model.py) visits rows by descending key and gives the first 64 to 64 different lane groups; with so few
entries in the block every row that has one outranks every empty row, so again no lane group holds two.  144: 256 rows of 36.  143: the same with the rows
192 .. 255 (slot 3 under MERGE) one entry shorter, and every row on the same columns: rows of one length then have one key, the deal visits the 192 long
ones and the 64 short ones as two runs, a level of 64 holds rows of one length, and every lane group gets three long rows and a short one.
test_the_ladder_has_the_steps_it_names asserts all of it on the CPU, from the two models.

fmx_debug_rows_ahead_launches proves which instance ran: every scheduled-form launch of a child at the depth it was asked for, none at another, and none
at all for the tile that is turned away."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_deal_model as D
from tests import rows_sched_cases as C
from tests import rows_sched_model as M
from tests.rows_deal_cases import CASES, HEAD, problem, seed_of
from tests.test_gpu_rows_clock_pace import DEAL_ENV, FAR_AHEAD, FAR_BEHIND, _load, _tail_steps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS = [1, 2, 3, 4]          # the depths fm_rows_sched_k is built for (ROWS_AHEAD_MAX)
LADDER = sorted({0, 1, 2, 143, 144} | {d + o for d in DEPTHS for o in (-1, 0, 1)})
MERGE_ENV = {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "merge"}
# name, environment, depth (0: the per-row form), policy, the planted targets of its engines (-1: none)
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}, 0, None, [-1])]
for _d in DEPTHS:
    CHILDREN += [(f"deal_a{_d}", dict(DEAL_ENV, FMX_ROWS_PACE="4", FMX_ROWS_AHEAD=str(_d)), _d, "deal", [-1, FAR_AHEAD, FAR_BEHIND]),
                 (f"merge_a{_d}", dict(MERGE_ENV, FMX_ROWS_PACE="4", FMX_ROWS_PACE_TRACE="1", FMX_ROWS_AHEAD=str(_d)), _d, "merge", [-1]),
                 (f"deal0_a{_d}", dict(DEAL_ENV, FMX_ROWS_PACE="0", FMX_ROWS_AHEAD=str(_d)), _d, "deal", [-1])]
# FMX_ROWS_AHEAD unset: the compiled default, whether the launch is paced or not
DEFAULT_DEPTH = 2              # FMX_ROWS_AHEAD_DEFAULT (fm_batch_kernels.hip), copied by hand: no hook exposes it, so a changed default shows here as the counts of `deal_rule` failing
CHILDREN += [("deal_rule", dict(DEAL_ENV, FMX_ROWS_PACE="4"), DEFAULT_DEPTH, "deal", [-1]),
             ("deal0_rule", dict(DEAL_ENV, FMX_ROWS_PACE="0"), DEFAULT_DEPTH, "deal", [-1])]
AT_ONCE = 8


def ladder_lengths(n):
    if n == 0:
        return np.zeros(3, np.int64)
    if n <= 36:
        return np.arange(16, dtype=np.int64) % (n + 1)
    assert n in (143, 144)
    lens = np.full(256, 36, np.int64)
    if n == 143:
        lens[192:] = 35
    return lens


def ladder_problem(n):
    """CSR of rows_sched_cases' HEAD rows, then one block of exactly n steps: rows of 0 .. 36 ascending entries"""
    rp, col, _, y = C.problem(C.CASES[0], 0, 7000 + n)
    rng = np.random.default_rng(7100 + n)
    lens = ladder_lengths(n)
    rows = [np.sort(rng.choice(C.P, k, replace=False)) for k in lens]
    if n == 143:   # one column set for every row (a short row lacks its last): rows of one length then share one key, and a level of the deal holds rows of one length
        rows = [rows[0][:k] for k in lens]
    col = np.concatenate([col] + rows).astype(np.uint32)
    rp = np.concatenate([rp, rp[-1] + np.cumsum(lens)])
    y = np.concatenate([y, np.where(rng.random(len(lens)) < 0.5, -1.0, 1.0).astype(np.float32)])
    return rp, col, np.ones(len(col), np.float32), y


_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.rows_deal_cases import CASES, HEAD, K, problem, seed_of
from tests.rows_sched_cases import P
from tests.test_gpu_rows_ahead import LADDER, ladder_problem
out, poisons = sys.argv[1], [int(x) for x in sys.argv[2].split(",")]
lib = L.lib()
def launches():
    a, s, p = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 2)()
    L.check(lib.fmx_debug_rows_ahead_launches(a))
    L.check(lib.fmx_debug_rows_sched_launches(s))
    L.check(lib.fmx_debug_rows_pace_launches(p))
    return np.array(list(a) + [s[0]] + list(p), np.int64)   # by depth 1 .. 4; scheduled-form launches; of which paced, not paced
def run(res, tag, m, p, seed, t):
    for poison in poisons:
        e = engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, mode=L.MODE_MINIBATCH,
                          batch_rows=2 * HEAD, tile_rows=HEAD)
        if poison >= 0:
            L.check(lib.fmx_debug_rows_clock_poison(e.h, ctypes.c_uint32(poison)))
        e.init_normal(seed, 0.0, 0.05)
        key = f"{tag}_{poison}"
        c0 = launches()
        for _ in range(3):
            e.step(m, 0, HEAD)     # the head tile alone
        res[key + "_launches_head"] = launches() - c0
        c0 = launches()
        for _ in range(3):
            e.step(m, 0, 0)        # head and tail
        w0, w, v = e.get_params()
        assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, key
        ck = os.path.join(out, "ck")
        e.save(ck)
        res[key + "_w0"], res[key + "_w"], res[key + "_v"] = np.float64(w0), w, v
        res[key + "_state"] = np.fromfile(ck, np.uint8)
        os.remove(ck)
        e.grad(m, 0, 0)
        e.sync()
        ptr, n = e.grad_buffer()
        res[key + "_grad"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
        res[key + "_launches"] = launches() - c0    # three steps and the gradient
        e.close()
for ci, case in enumerate(CASES):
    res = {}
    for t in case["tails"]:
        rp, col, val, y = problem(case, t, seed_of(ci, t))
        m = engine.Matrix.from_csr(rp, col, val, case["p"], y)
        run(res, f"t{t}", m, case["p"], 4000 + ci, t)
        m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
res = {}
for n in LADDER:
    rp, col, val, y = ladder_problem(n)
    m = engine.Matrix.from_csr(rp, col, val, P, y)
    run(res, f"t{n}", m, P, 4300 + n, n)
    m.close()
np.savez(os.path.join(out, "ladder.npz"), **res)
print("DONE", len(CASES) + 1)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    dirs, failed = {}, []
    for lo in range(0, len(CHILDREN), AT_ONCE):
        procs = []
        for name, env, _, _, poisons in CHILDREN[lo:lo + AT_ONCE]:
            d = tmp_path_factory.mktemp(name)
            child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
            child_env.update(env)
            argv = [str(d), ",".join(str(p) for p in poisons)]
            procs.append((name, d, subprocess.Popen([sys.executable, "-c", _CHILD] + argv, env=child_env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                                    text=True)))
        for name, d, pr in procs:
            try:
                so, se = pr.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                pr.kill()
                so, se = pr.communicate()
            if pr.returncode != 0 or f"DONE {len(CASES) + 1}" not in so:
                failed.append((name, pr.returncode, so[-1000:], se[-3000:]))
            dirs[name] = d
        if failed:
            break     # a child that failed: no further round goes out
    assert not failed, failed
    return dirs


def _ladder_steps(n, policy):
    rp, col, _, _ = ladder_problem(n)
    t = len(ladder_lengths(n))
    assert t <= 256
    if policy == "deal":
        return D.block_schedule(rp, col, HEAD, t, 0, C.P)[1].shape[0]
    return M.block_schedule(rp, col, HEAD, t, 0, C.P, M.MERGE, 0).shape[0]


def test_the_ladder_has_the_steps_it_names():
    assert LADDER == [0, 1, 2, 3, 4, 5, 143, 144] and M.STAGE_STEPS == 144
    for n in LADDER:
        lens = ladder_lengths(n)
        assert lens.min() >= 0 and lens.max() <= 36 and (n == 0 or lens.max() == min(n, 36))
        rp, col, _, _ = ladder_problem(n)
        for r in range(HEAD, HEAD + len(lens)):
            assert np.all(np.diff(col[rp[r]:rp[r + 1]].astype(np.int64)) > 0)      # ascending
        # MERGE: the largest lane-group total, lane group g holding the rows 64 s + g
        padded = np.zeros(256, np.int64)
        padded[:len(lens)] = lens
        assert padded.reshape(4, 64).sum(axis=0).max() == n
        assert _ladder_steps(n, "merge") == n and _ladder_steps(n, "deal") == n, n


def _compare(a, old, tag, poisons, where):
    for poison in poisons:
        for q in ("w0", "w", "v", "state", "grad"):
            assert np.array_equal(a[f"{tag}_{poison}_{q}"], old[f"{tag}_-1_{q}"]), (where, tag, poison, q)


def _counts(a, tag, poisons, depth, took, paced, where):
    """every scheduled-form launch ran the instance of `depth`: 3 on the head tile alone, then 3 steps and a gradient of 1 + took launches each"""
    for poison in poisons:
        for key, n in ((f"{tag}_{poison}_launches_head", 3), (f"{tag}_{poison}_launches", 4 * (1 + took))):
            c = [int(x) for x in a[key]]
            want = [0, 0, 0, 0, n] + ([n, 0] if paced else [0, n])
            want[depth - 1] = n
            assert c == want, (where, key, c, want)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_no_depth_changes_a_bit(runs, ci, depth):
    case = CASES[ci]
    old = _load(runs, "old", case["name"])
    assert np.any(old[f"t{case['tails'][-1]}_-1_v"] != 0.0)
    for t in case["tails"]:
        assert not old[f"t{t}_-1_launches"].any() and not old[f"t{t}_-1_launches_head"].any()
    for name, env, d, policy, poisons in CHILDREN:
        if d != depth:
            continue
        a = _load(runs, name, case["name"])
        for t in case["tails"]:
            _compare(a, old, f"t{t}", poisons, (case["name"], name))
            fits = all(s <= M.STAGE_STEPS for s in _tail_steps(case, ci, t, policy))
            if policy == "deal":
                assert fits == (case["name"] != "over37")      # the tile that is turned away runs no instance at all
            _counts(a, f"t{t}", poisons, depth, int(fits), env["FMX_ROWS_PACE"] != "0", (case["name"], name))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", DEPTHS)
def test_no_depth_changes_a_bit_at_a_block_s_ends(runs, depth):
    old = _load(runs, "old", "ladder")
    assert np.any(old["t144_-1_v"] != 0.0)
    for name, env, d, policy, poisons in CHILDREN:
        if d != depth:
            continue
        a = _load(runs, name, "ladder")
        for n in LADDER:
            _compare(a, old, f"t{n}", poisons, ("ladder", name))
            _counts(a, f"t{n}", poisons, depth, 1, env["FMX_ROWS_PACE"] != "0", ("ladder", name))
