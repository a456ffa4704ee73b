"""The drift of phase 1's waves, seen: the stamps of the diagnostic instance of fm_rows_sched_k (FMX_ROWS_PACE_TRACE=1; fmx_debug_rows_pace_trace) on
headline launches (1 M features, 30 per row, k = 16, SGD, 262 144-row tiles: 1 024 workgroups, one resident generation), reduced to what DESIGN.md 6.12
and profiles/rows_pace.txt quote.

    python profiles/rows_pace_trace.py [--pace 0|3|4] [--ahead 1..4] [--clock-tune every,lead,sleep,gain] [--launches 5] [--json FILE]

Lane 0 of every wave stores s_memrealtime (100 MHz) at step 0, 16, 32, ... and behind its last step, and HW_REG_XCC_ID.  Per launch:
  * labels: blockIdx.x % 8 against the XCC id the waves read -- each label must sit on one XCD;
  * drift(s): per XCD, the standard deviation over its waves of the time at which step s is reached, in steps (divided by the launch's mean step
    time), and the mean of that over the XCDs, for s = 0, 16, ...;  a random walk makes the VARIANCE grow linearly in s, a drift fixed from the start
    keeps it flat: the least-squares line var(s) = a + b s is printed;
  * steps(t): per XCD, the standard deviation over waves of the step reached at time t (stamps interpolated), at five times across the launch;
  * inside a workgroup against between workgroups: the variance of the four waves' times about their workgroup's mean, and of the workgroups' means
    about the XCD's, at the middle and at the end of the walk.
  * the launch's two ends (words 15 and 14: the stamps at kernel entry and behind the epilogue's last store): entry to step 0 -- the schedule stage, loaded
    while no gather is in flight -- and last step to exit -- the epilogue -- per wave, median and range, and the launch from its first entry to its last exit.
The switches are read once per process: --pace, --ahead and --clock-tune are put into the environment before the library loads."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORDS = 16


def reduce_launch(tr):
    """tr: uint64 [waves, 16]"""
    waves = tr.shape[0]
    xcc = (tr[:, 0] & 15).astype(np.int64)
    steps = ((tr[:, 0] >> 8) & 0xFFFF).astype(np.int64)
    slept = ((tr[:, 0] >> 32) & 0xFFFF).astype(np.int64)
    label = (np.arange(waves) // 4) % 8
    labels_ok = all(len(np.unique(xcc[label == lb])) == 1 for lb in range(8)) and len(np.unique(xcc)) == 8
    n = int(steps.min())
    assert n == int(steps.max()) and n >= 32, "the headline's blocks hold the same number of steps"
    at = list(range(0, n, 16))
    stamps = tr[:, 1:1 + len(at) + 1].astype(np.int64)       # the stamps of steps `at`, then the end
    t0 = stamps[:, 0].min()
    tm = (stamps - t0).astype(np.float64) * 0.01             # microseconds
    pos = np.array(at + [n], np.float64)
    step_us = float(np.mean((tm[:, -1] - tm[:, 0]) / n))
    out = {"waves": waves, "steps": n, "labels_are_xcds": bool(labels_ok), "launch_us": float(tm[:, -1].max()), "first_step_spread_us": float(tm[:, 0].max()),
           "step_us": step_us, "sleeps": int(slept.sum()), "waves_that_slept": int((slept > 0).sum())}
    if tr[:, 15].all() and tr[:, 14].all():   # a library that stamps the two ends
        entry, leave = (tr[:, 15].astype(np.int64) - t0) * 0.01, (tr[:, 14].astype(np.int64) - t0) * 0.01
        head, tail = tm[:, 0] - entry, leave - tm[:, -1]
        out["entry_to_step0_us"] = {"median": float(np.median(head)), "min": float(head.min()), "max": float(head.max())}
        out["last_step_to_exit_us"] = {"median": float(np.median(tail)), "min": float(tail.min()), "max": float(tail.max())}
        out["entry_spread_us"] = float(entry.max() - entry.min())
        out["first_entry_to_last_exit_us"] = float(leave.max() - entry.min())
        out["first_entry_to_first_step0_us"] = float(tm[:, 0].min() - entry.min())
        out["last_walk_end_to_last_exit_us"] = float(leave.max() - tm[:, -1].max())
    drift = np.zeros((8, len(pos)))
    for x in range(8):
        sel = tm[label == x]
        drift[x] = sel.std(axis=0) / step_us
    out["drift_steps_by_step"] = {str(int(s)): float(v) for s, v in zip(pos, drift.mean(axis=0))}
    out["drift_steps_by_step_per_xcd_end"] = [float(v) for v in drift[:, -1]]
    b, a = np.polyfit(pos, (drift ** 2).mean(axis=0), 1)
    out["variance_fit"] = {"at_step_0": float(a), "per_step": float(b), "fixed_share_at_end": float(a / max(a + b * n, 1e-12))}
    frac = [0.1, 0.25, 0.5, 0.75, 0.9]
    lo, hi = float(np.median(tm[:, 0])), float(np.median(tm[:, -1]))
    reached = {}
    for f in frac:
        t = lo + f * (hi - lo)
        sd = []
        for x in range(8):
            sel = tm[label == x]
            sd.append(float(np.std([np.interp(t, w, pos) for w in sel])))
        reached[str(f)] = float(np.mean(sd))
    out["sd_of_step_reached_at_time"] = reached
    for name, j in (("middle", len(pos) // 2), ("end", len(pos) - 1)):
        inside, between = [], []
        for x in range(8):
            sel = tm[label == x][:, j].reshape(-1, 4)
            inside.append(float(np.mean(sel.var(axis=1))))
            between.append(float(sel.mean(axis=1).var()))
        out[f"sd_inside_workgroup_steps_{name}"] = float(np.sqrt(np.mean(inside)) / step_us)
        out[f"sd_between_workgroups_steps_{name}"] = float(np.sqrt(np.mean(between)) / step_us)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pace", default="0", choices=["0", "3", "4"])
    ap.add_argument("--ahead", default=None, choices=["1", "2", "3", "4"], help="FMX_ROWS_AHEAD (unset: the library's default)")
    ap.add_argument("--clock-tune", default=None, help="FMX_ROWS_PACE_CLOCK_TUNE")
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--json", default=None)
    ap.add_argument("--raw", default=None, help="save the last launch's stamps as .npy")
    a = ap.parse_args()
    os.environ["FMX_ROWS_PACE_TRACE"] = "1"
    os.environ["FMX_ROWS_PACE"] = a.pace
    if a.ahead:
        os.environ["FMX_ROWS_AHEAD"] = a.ahead
    if a.clock_tune:
        os.environ["FMX_ROWS_PACE_CLOCK_TUNE"] = a.clock_tune
    from fmwr_amd import _lib as L
    from fmwr_amd import engine
    lib = L.lib()
    p, z, k, B = 1_000_000, 30, 16, a.rows
    m = engine.Matrix.synthetic_iid(2 * B, p, z, 20240001, law=L.COLUMNS_UNIFORM)
    e = engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=k, learn_rate=0.01, l2_w1=1e-4, l2_v=1e-4, mode=L.MODE_MINIBATCH, batch_rows=B)
    e.init_normal(1, 0.0, 0.01)
    for i in range(40):   # the engine settles its request schedule, the clocks ramp
        e.step(m, i % 2)
    e.sync()
    per = []
    for i in range(a.launches):
        e.step(m, i % 2)
        e.sync()
        waves = ctypes.c_int64(0)
        L.check(lib.fmx_debug_rows_pace_trace(e.h, None, ctypes.c_int64(0), ctypes.byref(waves)))
        if waves.value == 0:
            raise SystemExit("no traced launch: the step did not take the scheduled form")
        buf = np.zeros(waves.value * WORDS, np.uint64)
        L.check(lib.fmx_debug_rows_pace_trace(e.h, buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(buf)), ctypes.byref(waves)))
        per.append(reduce_launch(buf.reshape(-1, WORDS)))
        if a.raw and i == a.launches - 1:
            np.save(a.raw, buf.reshape(-1, WORDS))
    pl, cl = (ctypes.c_int64 * 2)(), (ctypes.c_int64 * 2)()
    L.check(lib.fmx_debug_rows_pace_launches(pl))
    L.check(lib.fmx_debug_rows_clock_launches(cl))
    keys = ["launch_us", "step_us", "first_step_spread_us", "sleeps", "waves_that_slept", "sd_inside_workgroup_steps_middle", "sd_between_workgroups_steps_middle",
            "sd_inside_workgroup_steps_end", "sd_between_workgroups_steps_end"]
    med = {q: float(np.median([r[q] for r in per])) for q in keys}
    med["drift_steps_by_step"] = {s: float(np.median([r["drift_steps_by_step"][s] for r in per])) for s in per[0]["drift_steps_by_step"]}
    med["sd_of_step_reached_at_time"] = {s: float(np.median([r["sd_of_step_reached_at_time"][s] for r in per])) for s in per[0]["sd_of_step_reached_at_time"]}
    if "entry_to_step0_us" in per[0]:
        for q in ("entry_to_step0_us", "last_step_to_exit_us"):
            med[q] = {s: float(np.median([r[q][s] for r in per])) for s in ("median", "min", "max")}
        for q in ("entry_spread_us", "first_entry_to_last_exit_us", "first_entry_to_first_step0_us", "last_walk_end_to_last_exit_us"):
            med[q] = float(np.median([r[q] for r in per]))
    med["variance_fit"] = {s: float(np.median([r["variance_fit"][s] for r in per])) for s in per[0]["variance_fit"]}
    out = {"pace": a.pace, "ahead": a.ahead, "tune": a.clock_tune, "paced_launches": int(pl[0]), "unpaced_launches": int(pl[1]),
           "clock_launches_with_target": int(cl[0]), "clock_launches_without": int(cl[1]), "labels_are_xcds": all(r["labels_are_xcds"] for r in per),
           "median": med, "launches": per}
    print(json.dumps({q: out[q] for q in ("pace", "ahead", "tune", "paced_launches", "unpaced_launches", "clock_launches_with_target", "clock_launches_without", "labels_are_xcds", "median")}, indent=1))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    e.close()
    m.close()


if __name__ == "__main__":
    main()
