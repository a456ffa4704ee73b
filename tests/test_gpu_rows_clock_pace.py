"""Phase 1's clock pace (fm_rows_sched_k<.., PACED = true>, FMX_ROWS_PACE=3 and 4; fm_batch_kernels.hip) changes no bit, whatever its targets are, and its
records hold what the schedules say.

The switches are read once per process, hence child processes, started together: the per-row form (FMX_ROWS_MERGE=0); the scheduled form under DEAL and under
MERGE with FMX_ROWS_PACE=4 (the clock pace wherever the scheduled form runs in one resident generation -- the small grids here qualify); DEAL under
fmx_debug_rows_clock_poison, which plants one target for every label before every launch, at 0xFFFFFFFF (16.7 M ticks a step: every wave finds itself far
ahead at every check and takes the longest sleep) and at 1 (far behind: none ever sleeps); those two once more through the stamping instance
(FMX_ROWS_PACE_TRACE=1), whose trace word counts the sleeps a wave took and their levels; DEAL with FMX_ROWS_PACE=0, the unpaced walk, none of whose launches
may count as paced; and FMX_ROWS_PACE=3 on one tile of 1 025 blocks, more than the 1 024
workgroups an MI355X holds at once, which must go out unpaced.  Every child is compared with the per-row form by np.array_equal on w0, w, V and the checkpoint
after three steps on the head tile alone (the second and third launch read the targets the one before left: fmx_debug_rows_clock_launches says so) and three
on head and tail, and on the exchange buffer after fmx_grad, on the shapes of tests/rows_deal_cases.py.

Without a bit comparison, on an engine of its own: after clock-paced launch n set n % 3 holds, label by label, the sum of T_b over the label's blocks
(tests/rows_deal_model.py, tests/rows_sched_model.py) and a positive tick count, set (n + 1) % 3 is zero, through three rotations and then one launch of the
tail; the first launch on a second matrix has no target and the second has one; and each replica of a two-replica engine keeps records of its own."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_deal_model as D
from tests import rows_sched_model as M
from tests.rows_deal_cases import CASES, HEAD, problem, seed_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEAL_ENV = {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "deal"}
EVERY = 24           # FMX_ROWS_PACE_CLOCK_EVERY: a wave looks at the clock behind steps 24, 48, ... < T_b
FAR_AHEAD, FAR_BEHIND = 0xFFFFFFFF, 1
BIG_ROWS = 1024 * 256 + 1   # 1 025 blocks: one more than 4 workgroups x 256 CUs
# name, environment, the planted target (-1: none), the policy whose steps the records are held to (None: not a clock-paced child), runs the big tile
CHILDREN = [("old", {"FMX_ROWS_MERGE": "0"}, -1, None, True),
            ("deal4", dict(DEAL_ENV, FMX_ROWS_PACE="4"), -1, "deal", False),
            ("merge4", {"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "merge", "FMX_ROWS_PACE": "4"}, -1, "merge", False),
            ("ahead", dict(DEAL_ENV, FMX_ROWS_PACE="4"), FAR_AHEAD, "deal", False),
            ("behind", dict(DEAL_ENV, FMX_ROWS_PACE="4"), FAR_BEHIND, "deal", False),
            ("ahead_t", dict(DEAL_ENV, FMX_ROWS_PACE="4", FMX_ROWS_PACE_TRACE="1"), FAR_AHEAD, "deal", False),
            ("behind_t", dict(DEAL_ENV, FMX_ROWS_PACE="4", FMX_ROWS_PACE_TRACE="1"), FAR_BEHIND, "deal", False),
            ("deal0", dict(DEAL_ENV, FMX_ROWS_PACE="0"), -1, None, False),
            ("big3", dict(DEAL_ENV, FMX_ROWS_PACE="3"), -1, None, True)]
GROUP_TAIL = 257   # the two-replica case: the `mixed` matrix with this tail, twice over, one copy per replica

_CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from fmwr_amd import engine, _lib as L
from tests import util
from tests.rows_deal_cases import CASES, HEAD, K, problem, seed_of
out, poison, group_tail, big_rows, only_big = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
lib = L.lib()
def launches():
    a, b = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
    L.check(lib.fmx_debug_rows_pace_launches(a))
    L.check(lib.fmx_debug_rows_clock_launches(b))
    return np.array(list(a) + list(b), np.int64)   # scheduled-form launches paced, not paced; clock-paced with a target, without one
def records(e, replica=0):
    a = (ctypes.c_uint64 * 48)()
    L.check(lib.fmx_debug_rows_clock_records_of(e.h, ctypes.c_int32(replica), a))
    return np.array(list(a), np.uint64).reshape(3, 8, 2)
def trace_words(e):
    n = ctypes.c_int64(0)
    L.check(lib.fmx_debug_rows_pace_trace(e.h, None, ctypes.c_int64(0), ctypes.byref(n)))
    buf = np.zeros(max(n.value, 1) * 16, np.uint64)
    L.check(lib.fmx_debug_rows_pace_trace(e.h, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(buf)), ctypes.byref(n)))
    return buf.reshape(-1, 16)[:n.value, 0].copy()
def make(p, batch_rows=2 * HEAD, tile_rows=HEAD, **kw):
    e = engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, mode=L.MODE_MINIBATCH,
                      batch_rows=batch_rows, tile_rows=tile_rows, **kw)
    if poison >= 0:
        L.check(lib.fmx_debug_rows_clock_poison(e.h, ctypes.c_uint32(poison)))
    return e
traced = os.environ.get("FMX_ROWS_PACE_TRACE") == "1"
if big_rows:   # one tile of more blocks than the device holds at once: every row 30 ascending columns
    p = CASES[0]["p"]
    rng = np.random.default_rng(77)
    width = p // 30
    col = ((np.arange(30, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (big_rows, 30))).astype(np.uint32).ravel()
    rp = np.arange(big_rows + 1, dtype=np.int64) * 30
    y = np.where(rng.random(big_rows) < 0.5, -1.0, 1.0).astype(np.float32)
    m = engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), p, y)
    e = make(p, batch_rows=big_rows, tile_rows=big_rows)
    e.init_normal(4200, 0.0, 0.05)
    c0 = launches()
    for _ in range(2):
        e.step(m, 0, 0)
    w0, w, v = e.get_params()
    np.savez(os.path.join(out, "big.npz"), w0=np.float64(w0), w=w, v=v, launches=launches() - c0)
    e.close()
    m.close()
for ci, case in enumerate([] if only_big else CASES):
    res = {}
    for t in case["tails"]:
        rp, col, val, y = problem(case, t, seed_of(ci, t))
        m = engine.Matrix.from_csr(rp, col, val, case["p"], y)
        e = make(case["p"])
        e.init_normal(4000 + ci, 0.0, 0.05)
        c0 = launches()
        for _ in range(3):
            e.step(m, 0, HEAD)     # the head tile alone: launches two and three read a target
        res[f"sgd_{t}_launches_head"] = launches() - c0
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
        if traced:
            res[f"trc_{t}_tail"] = trace_words(e)   # word 0 of every wave of the last launch: the tail tile's if its blocks fit, else the head's
        os.remove(ck)
        c0 = launches()
        e.grad(m, 0, 0)
        e.sync()
        ptr, n = e.grad_buffer()
        res[f"grad_{t}"] = util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)
        res[f"grad_{t}_launches"] = launches() - c0
        e.close()
        # the records, on an engine of its own: the head tile alone three times (every set written once), then head and tail
        e = make(case["p"])
        e.init_normal(4000 + ci, 0.0, 0.05)
        for i, limit in enumerate((HEAD, HEAD, HEAD, 0)):
            e.step(m, 0, limit)
            res[f"rec_{t}_{i}"] = records(e)
            if traced and i == 0:
                res[f"trc_{t}_head"] = trace_words(e)
        if ci == 0 and t == group_tail:
            # a second matrix of another shape: its first launch has no target although the engine's last launch was clock-paced, its second has one
            rp_b, col_b, val_b, y_b = problem(CASES[3], 257, seed_of(3, 257))
            mb = engine.Matrix.from_csr(rp_b, col_b, val_b, CASES[3]["p"], y_b)
            e.step(m, 0, HEAD)
            c0 = launches()
            e.step(mb, 0, HEAD)
            res["other_first"] = launches() - c0
            c0 = launches()
            e.step(mb, 0, HEAD)
            res["other_second"] = launches() - c0
            mb.close()
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
            res["group_rec_0"], res["group_rec_1"] = records(g, 0), records(g, 1)
            g.close()
            m2.close()
        m.close()
    np.savez(os.path.join(out, case["name"] + ".npz"), **res)
print("DONE", len(CASES))
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    procs = []
    for name, env, poison, _, big in CHILDREN:   # nine processes side by side: a few seconds in all
        d = tmp_path_factory.mktemp(name)
        child_env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
        child_env.update(env)
        argv = [str(d), str(poison), str(GROUP_TAIL), str(BIG_ROWS if big else 0), str(int(name == "big3"))]
        procs.append((name, d, subprocess.Popen([sys.executable, "-c", _CHILD] + argv, env=child_env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                                text=True)))
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
TICK_MASK = np.uint64((1 << 40) - 1)


def _label_steps(steps):
    out = np.zeros(8, np.int64)
    for b, s in enumerate(steps):
        out[b % 8] += s
    return out


def _steps_of(rec):
    return (rec[:, 0] >> np.uint64(40)).astype(np.int64)


def _ticks_of(rec):
    return (rec[:, 0] & TICK_MASK).astype(np.int64)


def _holds(rec, steps, planted):
    """set `rec` ([label][sums, planted]) is what a launch of blocks with `steps` steps leaves: the steps by label, ticks wherever a label has a block"""
    want = _label_steps(steps)
    blocks = np.bincount(np.arange(len(steps)) % 8, minlength=8)
    return np.array_equal(_steps_of(rec), want) and np.all((_ticks_of(rec) > 0) == (blocks > 0)) and np.all(rec[:, 1] == np.uint64(planted))


def _blank(rec, planted):
    return not rec[:, 0].any() and np.all(rec[:, 1] == np.uint64(planted))


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(CASES)), ids=[c["name"] for c in CASES])
def test_the_clock_pace_changes_no_bit_and_records_its_steps(runs, ci):
    case = CASES[ci]
    old = _load(runs, "old", case["name"])
    assert np.any(old[f"sgd_{case['tails'][-1]}_v"] != 0.0)
    for name, _, poison, policy, _ in CHILDREN[1:-1]:
        a = _load(runs, name, case["name"])
        planted = max(poison, 0)
        for t in case["tails"]:
            for key in [f"sgd_{t}_{q}" for q in ("w0", "w", "v", "state")] + [f"grad_{t}"]:
                assert np.array_equal(a[key], old[key]), (case["name"], name, key)
            steps = _tail_steps(case, ci, t, policy or "deal")
            fits = all(s <= M.STAGE_STEPS for s in steps)
            if (policy or "deal") == "deal":
                assert fits == (case["name"] != "over37")
            took = 1 + int(fits)   # scheduled-form launches of a full step or a gradient: the head tile, and the tail tile if its blocks fit the stage
            assert not old[f"sgd_{t}_launches"].any() and not old[f"sgd_{t}_launches_head"].any() and not old[f"grad_{t}_launches"].any()
            if policy is None:   # FMX_ROWS_PACE=0: every launch of the scheduled form unpaced, and an engine that never paces leaves its records as they were allocated
                assert [int(x) for x in a[f"sgd_{t}_launches_head"]] == [0, 3, 0, 0], (case["name"], name, t)
                assert [int(x) for x in a[f"sgd_{t}_launches"]] == [0, 3 * took, 0, 0], (case["name"], name, t, a[f"sgd_{t}_launches"])
                assert [int(x) for x in a[f"grad_{t}_launches"]] == [0, took, 0, 0], (case["name"], name, t, a[f"grad_{t}_launches"])
                assert not any(a[f"rec_{t}_{i}"].any() for i in range(4)), (case["name"], name, t)
                continue
            # the head tile alone, three times: the first launch of the engine has no target, the next two have the one before's
            assert [int(x) for x in a[f"sgd_{t}_launches_head"]] == ([3, 0, 3, 0] if poison >= 0 else [3, 0, 2, 1]), (case["name"], name, t)
            # head and tail, three times: only the first head launch follows a launch of its own row count (a tail turned away is another launch in between)
            n = 3 * took
            assert [int(x) for x in a[f"sgd_{t}_launches"]] == ([n, 0, n, 0] if poison >= 0 else [n, 0, 1, n - 1]), (case["name"], name, t, a[f"sgd_{t}_launches"])
            assert [int(x) for x in a[f"grad_{t}_launches"]] == ([took, 0, took, 0] if poison >= 0 else [took, 0, 0, took]), (case["name"], name, t)
            r = [a[f"rec_{t}_{i}"] for i in range(4)]
            if poison < 0:
                # clock-paced launch n: set n % 3 written, set (n + 1) % 3 cleared, set (n + 2) % 3 as launch n - 1 left it
                assert _holds(r[0][0], HEAD_STEPS, 0) and _blank(r[0][1], 0) and _blank(r[0][2], 0), (case["name"], name, t, r[0])
                assert _holds(r[1][1], HEAD_STEPS, 0) and _blank(r[1][2], 0) and np.array_equal(r[1][0], r[0][0]), (case["name"], name, t, r[1])
                assert _holds(r[2][2], HEAD_STEPS, 0) and _blank(r[2][0], 0) and np.array_equal(r[2][1], r[1][1]), (case["name"], name, t, r[2])
                if fits:   # launch 3 the head into set 0, launch 4 the tail into set 1, which clears set 2
                    assert _holds(r[3][1], steps, 0) and _blank(r[3][2], 0) and _holds(r[3][0], HEAD_STEPS, 0), (case["name"], name, t, r[3], steps)
                else:      # launch 3 the head into set 0, and the tail goes elsewhere
                    assert _holds(r[3][0], HEAD_STEPS, 0) and _blank(r[3][1], 0) and np.array_equal(r[3][2], r[2][2]), (case["name"], name, t, r[3])
            else:
                # planted: every record holds the target, the set the last launch wrote its sums, and the other two nothing (the plant clears the sums)
                for i, x in enumerate(r):
                    last, last_steps = (i % 3, HEAD_STEPS) if i < 3 else ((1, steps) if fits else (0, HEAD_STEPS))
                    for s in range(3):
                        ok = _holds(x[s], last_steps, planted) if s == last else _blank(x[s], planted)
                        assert ok, (case["name"], name, t, i, s, x[s])
                if name.endswith("_t"):
                    # a wave of a T-step block looks at the clock behind steps 24, 48, ... < T: (T - 1) // 24 times.  Far ahead: a sleep of the longest length
                    # (level 3) at every look of every wave; far behind: not one
                    for key, blocks in ((f"trc_{t}_head", HEAD_STEPS), (f"trc_{t}_tail", steps if fits else HEAD_STEPS)):
                        w0 = a[key].astype(np.uint64)
                        walked = ((w0 >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.int64)
                        assert np.array_equal(walked, np.repeat(np.array(blocks, np.int64), 4)), (case["name"], name, t, key)
                        slept = ((w0 >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
                        levels = (w0 >> np.uint64(48)).astype(np.int64)
                        if poison == FAR_AHEAD:
                            assert np.array_equal(slept, np.maximum(0, (walked - 1) // EVERY)) and np.array_equal(levels, 3 * slept), (case["name"], name, t, key)
                        else:
                            assert not slept.any() and not levels.any(), (case["name"], name, t, key, np.bincount(slept))


@pytest.mark.gpu
def test_another_matrix_starts_without_a_target(runs):
    for name, _, poison, policy, _ in CHILDREN[1:3]:
        a = _load(runs, name, "mixed")
        assert [int(x) for x in a["other_first"]] == [1, 0, 0, 1], (name, a["other_first"])
        assert [int(x) for x in a["other_second"]] == [1, 0, 1, 0], (name, a["other_second"])


@pytest.mark.gpu
def test_every_replica_of_a_group_has_records_of_its_own(runs):
    ci, case = 0, CASES[0]
    assert case["name"] == "mixed" and GROUP_TAIL in case["tails"]
    old = _load(runs, "old", "mixed")
    for name, _, poison, policy, _ in CHILDREN[1:-1]:
        a = _load(runs, name, "mixed")
        for key in ("group_w0", "group_w", "group_v"):
            assert np.array_equal(a[key], old[key]), (name, key)
        # one global step: every replica runs its copy's head tile and tail tile
        if policy is None:
            assert [int(x) for x in a["group_launches"]] == [0, 4, 0, 0], (name, a["group_launches"])
            continue
        assert [int(x) for x in a["group_launches"][:2]] == [4, 0], (name, a["group_launches"])
        assert [int(x) for x in a["group_launches"][2:]] == ([4, 0] if poison >= 0 else [0, 4]), (name, a["group_launches"])
        if poison < 0:
            tail = _tail_steps(case, ci, GROUP_TAIL, policy)
            for r in (0, 1):   # each replica: launch 0 the head into its set 0, launch 1 the tail into its set 1, which clears its set 2
                c = a[f"group_rec_{r}"]
                assert _holds(c[0], HEAD_STEPS, 0) and _holds(c[1], tail, 0) and _blank(c[2], 0), (name, r, c)


@pytest.mark.gpu
def test_mode_3_leaves_a_grid_of_two_generations_unpaced(runs):
    old, a = _load(runs, "old", "big"), _load(runs, "big3", "big")
    for key in ("w0", "w", "v"):
        assert np.array_equal(a[key], old[key]), key
    assert np.any(old["v"] != 0.0)
    assert [int(x) for x in a["launches"]] == [0, 2, 0, 0], a["launches"]   # two scheduled-form launches, neither paced
    assert not old["launches"].any()
