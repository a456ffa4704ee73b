"""Phase 1's pace (fm_rows_sched_k<.., PACE>, FMX_ROWS_PACE; fm_batch_kernels.hip) changes no bit, whatever its counters hold, and its counters hold what
tests/rows_pace_model.py says.

The switches are read once per process, hence child processes, started together: the per-row form (FMX_ROWS_MERGE=0); the scheduled form under DEAL with
FMX_ROWS_PACE=0 and =2 (2: wherever the scheduled form runs in one resident generation -- the small grids here qualify); MERGE with the pace; and DEAL with
the pace under fmx_debug_rows_pace_poison -- both sets filled with a value that EVERY check-in of every launch then returns, the check-ins adding 0 -- at 0
(every workgroup finds itself far ahead of a mean of nothing at every check-in, and its waves take the longest sleep each time) and at 0xFFFFFFFF (far
behind: none ever sleeps); the last two once more through the stamping instance (FMX_ROWS_PACE_TRACE=1), whose trace word says how often each wave slept
and at which level, so that the test SEES the sleeps taken and not taken; both sets must still hold the planted value after every launch.  Every child is compared with the per-row form by np.array_equal on w0, w, V and the checkpoint after three mini-batch steps and on
the exchange buffer after fmx_grad, on the shapes of tests/rows_deal_cases.py: tails of 1, 63, 64, 65, 255 and 257 rows with empty rows among them, unsorted
rows, the over-37 tile that is turned away, and the p = 64 tie case.  fmx_debug_rows_pace_launches says which launches were paced: every launch of the
scheduled form in the paced children -- a tile has one exactly if the model says its blocks fit -- and none elsewhere.  Three more steps on an engine of
their own (the head tile alone, twice, then head and tail) pin the check-in, the ping-pong of the two sets and the clearing: after a paced launch the set
it used holds the model's counts label by label and the other set is zero.  One case runs a two-replica engine: the same bits, and each replica's own
counters."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_deal_model as D
from tests import rows_pace_model as P
from tests import rows_sched_model as M
from tests.rows_deal_cases import CASES, HEAD, problem, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAL_ENV = {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "deal"}
# name, environment, the poison (-1: none), the policy whose steps the counters are held to (None: not a paced child)
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}, -1, None),
            ("deal0", dict(DEAL_ENV, FMX_ROWS_PACE="0"), -1, None),
            ("deal2", dict(DEAL_ENV, FMX_ROWS_PACE="2"), -1, "deal"),
            ("merge2", {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "merge", "FMX_ROWS_PACE": "2"}, -1, "merge"),
            ("ahead", dict(DEAL_ENV, FMX_ROWS_PACE="2"), 0, "deal"),
            ("behind", dict(DEAL_ENV, FMX_ROWS_PACE="2"), 0xFFFFFFFF, "deal"),
            # the same two through the stamping instance, whose trace word says how often every wave slept, and how long
            ("ahead_t", dict(DEAL_ENV, FMX_ROWS_PACE="2", FMX_ROWS_PACE_TRACE="1"), 0, "deal"),
            ("behind_t", dict(DEAL_ENV, FMX_ROWS_PACE="2", FMX_ROWS_PACE_TRACE="1"), 0xFFFFFFFF, "deal")]
GROUP_TAIL = 257   # the two-replica case: the `mixed` matrix with this tail, twice over, one copy per replica

_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.rows_deal_cases import CASES, HEAD, K, problem, seed_of
out, poison, group_tail = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
lib = L.lib()
def launches():
    a = (ctypes.c_int64 * 2)()
    L.check(lib.fmx_debug_rows_pace_launches(a))
    return np.array(list(a), np.int64)
def counters(e, replica=0):
    a = (ctypes.c_uint32 * 16)()
    L.check(lib.fmx_debug_rows_pace_counters_of(e.h, ctypes.c_int32(replica), a))
    return np.array(list(a), np.int64).reshape(2, 8)
def trace_words(e):
    n = ctypes.c_int64(0)
    L.check(lib.fmx_debug_rows_pace_trace(e.h, None, ctypes.c_int64(0), ctypes.byref(n)))
    buf = np.zeros(max(n.value, 1) * 16, np.uint64)
    L.check(lib.fmx_debug_rows_pace_trace(e.h, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(buf)), ctypes.byref(n)))
    return buf.reshape(-1, 16)[:n.value, 0].copy()
def make(p, **kw):
    e = engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, mode=L.MODE_MINIBATCH,
                      batch_rows=2 * HEAD, tile_rows=HEAD, **kw)
    if poison >= 0:
        L.check(lib.fmx_debug_rows_pace_poison(e.h, ctypes.c_uint32(poison)))
    return e
for ci, case in enumerate(CASES):
    res = {}
    for t in case["tails"]:
        rp, col, val, y = problem(case, t, seed_of(ci, t))
        m = engine.Matrix.from_csr(rp, col, val, case["p"], y)
        e = make(case["p"])
        e.init_normal(4000 + ci, 0.0, 0.05)
        c0 = launches()
        for _ in range(3):
            e.step(m, 0, 0)
        w0, w, v = e.get_params()
        assert np.isfinite(w0) and np.isfinite(w).all() and np.isfinite(v).all() and np.abs(w).max() > 0, (case["name"], t)
        ck = os.path.join(out, "ck")
        e.save(ck)
        res[f"sgd_{t}_w0"], res[f"sgd_{t}_w"], res[f"sgd_{t}_v"] = np.float64(w0), w, v
        res[f"sgd_{t}_state"] = np.fromfile(ck, np.uint8)
        res[f"sgd_{t}_launches"] = launches() - c0
        os.remove(ck)
        c0 = launches()
        e.grad(m, 0, 0)
        e.sync()
        ptr, n = e.grad_buffer()
        res[f"grad_{t}"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
        res[f"grad_{t}_launches"] = launches() - c0
        e.close()
        # the counters, on an engine of its own: the head tile alone (one launch), the head tile alone, then head and tail
        e = make(case["p"])
        e.init_normal(4000 + ci, 0.0, 0.05)
        for i, limit in enumerate((HEAD, HEAD, 0)):
            e.step(m, 0, limit)
            res[f"ctr_{t}_{i}"] = counters(e)
            if os.environ.get("FMX_ROWS_PACE_TRACE") == "1":
                res[f"trc_{t}_{i}"] = trace_words(e)   # word 0 of every wave of the step's last launch
        e.close()
        if case["name"] == "mixed" and t == group_tail:
            rp2 = np.concatenate([rp, rp[1:] + rp[-1]])
            m2 = engine.Matrix.from_csr(rp2, np.concatenate([col, col]), np.concatenate([val, val]), case["p"], np.concatenate([y, y]))
            g = make(case["p"], n_gpus=2, gpus_share_device=1)
            g.init_normal(4100, 0.0, 0.05)
            c0 = launches()
            done = g.train(m2, 2 * (HEAD + t))
            assert done == 2 * (HEAD + t), done
            gw0, gw, gv = g.get_params()
            res["group_w0"], res["group_w"], res["group_v"] = np.float64(gw0), gw, gv
            res["group_launches"] = launches() - c0
            res["group_ctr_0"], res["group_ctr_1"] = counters(g, 0), counters(g, 1)
            g.close()
            m2.close()
        m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
print("DONE", len(CASES))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    procs = []
    for name, env, poison, _ in CHILDREN:   # eight processes side by side: a few seconds in all
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        procs.append((name, d, subprocess.Popen([sys.executable, "-c", _CHILD, str(d), str(poison), str(GROUP_TAIL)], env=child_env, cwd=ROOT,
                                                stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)))
    dirs, failed = {}, []
    for name, d, pr in procs:
        try:
            so, se = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            pr.kill()
            so, se = pr.communicate()
        if pr.returncode != 0 or f"DONE {len(CASES)}" not in so:
            failed.append((name, pr.returncode, so[-1000:], se[-3000:]))
        dirs[name] = d
    assert not failed, failed
    return dirs


def _load(runs, child, name):
    with np.load(os.path.join(runs[child], name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def _tail_steps(case, ci, t, policy):
    """T_b of every block of the tail tile under `policy`"""
    rp, col, _, _ = problem(case, t, seed_of(ci, t))
    blocks = range((t + 255) // 256)
    if policy == "deal":
        return [D.block_schedule(rp, col, HEAD, t, b, case["p"])[1].shape[0] for b in blocks]
    return [M.block_schedule(rp, col, HEAD, t, b, case["p"], M.MERGE, 0).shape[0] for b in blocks]


HEAD_STEPS = [120] * (HEAD // 256)   # the head tile: every lane group holds four rows of 30 entries, no bubble, under MERGE and under any deal


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_the_pace_changes_no_bit_and_counts_its_check_ins(runs, ci):
    case = CASES[ci]
    old = _load(runs, "old", case["name"])
    assert np.any(old[f"sgd_{case['tails'][-1]}_v"] != 0.0)
    head = P.launch_counters(HEAD_STEPS)
    assert head.sum() == 4 * (HEAD // 256)   # steps 24, 48, 72 and 96 of 120
    for name, _, poison, policy in CHILDREN[1:]:
        a = _load(runs, name, case["name"])
        for t in case["tails"]:
            for key in [f"sgd_{t}_{q}" for q in ("w0", "w", "v", "state")] + [f"grad_{t}"]:
                assert np.array_equal(a[key], old[key]), (case["name"], name, key)
            steps = _tail_steps(case, ci, t, policy or "deal")
            fits = all(s <= M.STAGE_STEPS for s in steps)
            if (policy or "deal") == "deal":
                assert fits == (case["name"] != "over37")
            took = 1 + int(fits)   # scheduled-form launches of a step or a gradient: the head tile, and the tail tile if its blocks fit the stage
            want = [took, 0] if policy else [0, took]
            assert [int(x) for x in a[f"sgd_{t}_launches"]] == [3 * x for x in want], (case["name"], name, t, a[f"sgd_{t}_launches"])
            assert [int(x) for x in a[f"grad_{t}_launches"]] == want, (case["name"], name, t, a[f"grad_{t}_launches"])
            assert [int(x) for x in old[f"sgd_{t}_launches"]] == [0, 0] and [int(x) for x in old[f"grad_{t}_launches"]] == [0, 0]
            c = [a[f"ctr_{t}_{i}"] for i in range(3)]
            if policy is None:
                assert not any(x.any() for x in c), (case["name"], name, t)   # an engine that never paces leaves its counters as they were allocated
            elif poison < 0:
                zero = np.zeros(8, np.int64)
                # paced launch 0: the head tile into set 0; launch 1: the head tile into set 1, set 0 cleared; then launch 2 (head, set 0) and, if the
                # tail has a schedule, launch 3 (tail, set 1), each clearing the other set
                assert np.array_equal(c[0][0], head) and np.array_equal(c[0][1], zero), (case["name"], name, t, c[0])
                assert np.array_equal(c[1][1], head) and np.array_equal(c[1][0], zero), (case["name"], name, t, c[1])
                if fits:
                    assert np.array_equal(c[2][1], P.launch_counters(steps)) and np.array_equal(c[2][0], zero), (case["name"], name, t, c[2], steps)
                else:
                    assert np.array_equal(c[2][0], head) and np.array_equal(c[2][1], zero), (case["name"], name, t, c[2])
            else:
                # poisoned: the check-ins add nothing and no launch clears, so both sets hold the planted value after every launch ...
                for x in c:
                    assert np.array_equal(x, np.full((2, 8), poison, np.int64)), (case["name"], name, t, x)
                if name.endswith("_t"):
                    # ... and every check-in returned it.  The first step ran the head tile alone: 512 waves of 120 steps, 4 check-ins each.  Planted 0:
                    # the workgroup is 24 k - 11.5 steps ahead of a mean of nothing at check-in k, beyond three times the lead, so every sleep is the
                    # longest one (level 3); a wave that passes before its workgroup's first word is written -- the add holds the checking wave up -- misses that one sleep and no other.
                    # Planted 0xFFFFFFFF: far behind at every check-in, not one sleep in the launch.
                    w0 = a[f"trc_{t}_0"].astype(np.uint64)
                    assert len(w0) == 4 * len(HEAD_STEPS) and np.all(((w0 >> np.uint64(8)) & np.uint64(0xFFFF)) == 120), (case["name"], name, t)
                    slept = ((w0 >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
                    levels = (w0 >> np.uint64(48)).astype(np.int64)
                    if poison == 0:
                        n = P.block_checkins(120)
                        # (the wave that makes the first check-in, wave 1 of its workgroup, writes the word before it reads it: it misses none)
                        assert np.all((slept == n) | (slept == n - 1)) and np.all(slept[1::4] == n), (case["name"], name, t, np.bincount(slept))
                        assert np.array_equal(levels, 3 * slept), (case["name"], name, t)
                    else:
                        assert not slept.any() and not levels.any(), (case["name"], name, t, np.bincount(slept))


@pytest.mark.gpu
def test_every_replica_of_a_group_has_counters_of_its_own(runs):
    ci, case = 0, CASES[0]
    assert case["name"] == "mixed" and GROUP_TAIL in case["tails"]
    old = _load(runs, "old", "mixed")
    for name, _, poison, policy in CHILDREN[1:]:
        tail = P.launch_counters(_tail_steps(case, ci, GROUP_TAIL, policy or "deal"))
        assert tail.sum() > 0
        a = _load(runs, name, "mixed")
        for key in ("group_w0", "group_w", "group_v"):
            assert np.array_equal(a[key], old[key]), (name, key)
        # one global step: every replica runs its copy's head tile and tail tile
        assert [int(x) for x in a["group_launches"]] == ([4, 0] if policy else [0, 4]), (name, a["group_launches"])
        if policy and poison < 0:
            for r in (0, 1):   # each replica: launch 0 the head into its set 0, launch 1 the tail into its set 1
                c = a[f"group_ctr_{r}"]
                assert np.array_equal(c[1], tail) and not c[0].any(), (name, r, c)
