"""CPU model of the V and w lines phase 1's DEAL walk fetches per tile when the workgroups drift as the trace says they do, with and without the pace
(profiles/rows_clock_pace.txt).  numpy only:  python profiles/rows_pace_sim.py [--rate 0.08] [--every 8 --lead 2 --sleep 10 --gain 1.0] [--seed 1]

profiles/rows_deal_sim.py gave every wave an offset against the common clock that is FIXED for the walk (N(0, d) steps; d = 4 fitted).  The stamps of
profiles/rows_pace_trace.py show something else: the spread of an XCD's waves is 0.7 steps at step 0 and grows in proportion to the step -- 2.2, 3.5, 4.7,
5.9, 6.9, 8.0 steps at step 16, 32, ... 96 -- so the VARIANCE grows with the square of the step: neither a fixed offset nor a random walk but a pace of
its own per workgroup (between workgroups 6.7 steps at the end, between the four waves of one 0.7).  Here workgroup g reaches step t at
    o_g + t (1 + r_g),   o_g ~ N(0, start),   r_g ~ N(0, rate)      (rate 0.08: 8 steps of spread at step 96)
and its four waves within N(0, inside) of that.  The same streams, LRU and line sizes as rows_deal_sim.py (imported).

The pace: the lead is taken against a target -- at steps E, 2 E, ... a workgroup that has done s + 1 steps in less than (s + 1 - lead) x target (2 x, 3 x
the lead: the longer lengths) is held for sleep x 64 cycles (one step = 0.78 us = 1 870 cycles at 2.4 GHz), the target being gain x the
mean time per step of the XCD's workgroups in the launch BEFORE (the model runs the launch `--clock-launches` times, the first one without a target, each
with the same paces, and prices the last).  The look at the clock is free, as on the device.  Used only to choose the sweep's grid: not evidence."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rows_deal_sim as S   # noqa: E402

STEP_CYCLES = 1870.0
N_STEPS = S.SLOTS * S.NNZ


def arrival_times(rng, rate, start, inside):
    """[BLOCKS * 4, N_STEPS]: when each wave of each workgroup of the XCD reaches each step of an unpaced walk, in steps"""
    o = rng.normal(0.0, start, S.BLOCKS)
    r = rng.normal(0.0, rate, S.BLOCKS)
    t = np.arange(N_STEPS, dtype=np.float64)
    wg = o[:, None] + t[None, :] * (1.0 + r[:, None])
    return np.repeat(wg, 4, axis=0) + rng.normal(0.0, inside, S.BLOCKS * 4)[:, None]


def arrival_times_clock(rng, rate, start, inside, clock, launches):
    """the same under the pace; clock = (every, lead, sleep, gain).  Returns the last launch's waves, its sleeps and the targets launch by launch"""
    every, lead, sleep, gain = clock
    o = rng.normal(0.0, start, S.BLOCKS)
    r = rng.normal(0.0, rate, S.BLOCKS)
    jitter = rng.normal(0.0, inside, S.BLOCKS * 4)
    t = np.arange(N_STEPS, dtype=np.float64)
    target, targets = 0.0, []
    for _ in range(launches):
        held = np.zeros((S.BLOCKS, N_STEPS))
        delay = np.zeros(S.BLOCKS)
        slept = 0
        if target > 0.0:
            for k in range(1, (N_STEPS - 1) // every + 1):
                s = k * every
                gone = (s + 1) * (1.0 + r) + delay          # time since the workgroup's own step 0, behind step s
                level = sum(((s + 1 - m * lead) * target > gone).astype(int) for m in (1, 2, 3))
                slept += int((level > 0).sum())
                delay = delay + level * sleep * 64.0 / STEP_CYCLES
                held[:, s + 1:] = delay[:, None]
        targets.append(target)
        target = gain * float(np.sum(N_STEPS * (1.0 + r) + delay) / (S.BLOCKS * N_STEPS))   # what the launch leaves in its record
    wg = o[:, None] + t[None, :] * (1.0 + r[:, None]) + held
    waves = np.repeat(wg, 4, axis=0) + jitter[:, None]
    return waves, slept, targets


def lines_fetched(cols, when_wave):
    """(V lines, w lines): rows_deal_sim's LRU over the accesses in the order `when_wave` gives them (a wave = 16 lane-group streams)"""
    when = np.repeat(when_wave, 16, axis=0).ravel()
    order = np.argsort(when, kind="stable")
    flat = cols.ravel()[order]
    v_line, w_line = (flat >> 1).tolist(), ((flat >> 5) + S.W_BASE).tolist()
    lru, miss_v, miss_w = {}, 0, 0
    for v, w in zip(v_line, w_line):
        for key in (v, w):
            if key in lru:
                del lru[key]
            else:
                if key >= S.W_BASE:
                    miss_w += 1
                else:
                    miss_v += 1
                if len(lru) >= S.LRU_LINES:
                    del lru[next(iter(lru))]
            lru[key] = None
    return miss_v, miss_w


def spread(when_wave):
    return {s: float(when_wave[:, s].std()) for s in (0, 32, 64, 96, N_STEPS - 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rate", type=float, nargs="*", default=[0.0, 0.04, 0.08])
    ap.add_argument("--start", type=float, default=0.7)
    ap.add_argument("--inside", type=float, default=0.7)
    ap.add_argument("--every", type=int, default=8)
    ap.add_argument("--lead", type=float, nargs="*", default=[1.0, 2.0, 4.0])
    ap.add_argument("--sleep", type=int, nargs="*", default=[10, 20])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gain", type=float, nargs="*", default=[1.0, 0.97, 0.94])
    ap.add_argument("--clock-launches", type=int, default=6)
    a = ap.parse_args()
    t0 = time.time()
    cols = S.streams(np.random.default_rng(a.seed), "deal")
    print(f"DEAL streams made in {time.time() - t0:.1f} s")
    print("M lines per tile (8 XCDs); spread = sd over the XCD's waves of the time a step is reached, in steps")
    for rate in a.rate:
        w = arrival_times(np.random.default_rng(a.seed + 1000), rate, a.start, a.inside)
        v, wl = lines_fetched(cols, w)
        sp = spread(w)
        print(f"rate {rate:.2f}  no pace              V {S.XCDS * v / 1e6:5.2f}  w {S.XCDS * wl / 1e6:4.2f}  spread " + " ".join(f"{s}:{x:.1f}" for s, x in sp.items()), flush=True)
        if rate == 0.0:
            continue
        for lead in a.lead:
            for sleep in a.sleep:
                for gain in a.gain:
                    w, slept, targets = arrival_times_clock(np.random.default_rng(a.seed + 1000), rate, a.start, a.inside, (a.every, lead, sleep, gain), a.clock_launches)
                    v, wl = lines_fetched(cols, w)
                    sp = spread(w)
                    print(f"rate {rate:.2f}  clock every {a.every} lead {lead:.0f} sleep {sleep:2d} gain {gain:.2f}  V {S.XCDS * v / 1e6:5.2f}  w {S.XCDS * wl / 1e6:4.2f}  spread " +
                          " ".join(f"{s}:{x:.1f}" for s, x in sp.items()) + f"  sleeps {slept}  end {w.max() - w.min():.1f} steps  target {targets[-1]:.4f}", flush=True)
    print(f"{time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
