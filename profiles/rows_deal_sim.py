"""CPU model of the V lines phase 1's scheduled form fetches per tile, under three assignments of a block's rows to its lane groups (profiles/rows_deal.txt;
DESIGN.md 6.11).  numpy only, a few seconds per case:  python profiles/rows_deal_sim.py [--drift 0 2 4 8] [--ahead 1 2 3 4] [--seed 1]

What is modelled: one XCD's share of a tile on the headline shape -- 128 resident 256-row blocks (32 CUs x 4 workgroups: one generation) of i.i.d. rows of
30 sorted columns over p = 1 M, that is 8 192 lane-group streams of 120 entries, each walked in column order, one entry per step.  Every entry touches its V
line (64-byte rows: two per 128-byte line) and its w line (32 words per line); both kinds share one LRU of 32 768 lines (the XCD's 4 MiB L2).  The waves
(16 lane groups each) do not run in lockstep: wave j is offset against the common clock by N(0, d) steps, fixed for the walk.  A tile is eight such shares.

The assignments:  identity (MERGE: lane group g owns rows 64 s + g),  DEAL (tests/rows_deal_model.py: the rule the device builder implements),  and
perfectly even streams (entry t of every stream drawn inside the t-th of 120 equal column bands: the floor for any assignment at that drift).

The drift d is not known from first principles: it is calibrated so that the identity reproduces the V-line count measured for MERGE on the device
(fabric reads per launch minus the schedule's own lines and the w lines).  With that one number fixed, the model predicts DEAL's count.

--ahead (the look-ahead walk, fm_rows_sched_k<.., AHEAD>; profiles/rows_ahead.txt): every wave issues the requests of step t when it stands
at step t - (AHEAD - 1) -- the first AHEAD - 1 steps' all at once, at its start; the LRU is unchanged.  A look-ahead that every wave has alike shifts all
request streams by the same amount, so the model can only see the start of the walk change: it prints DEAL's lines per depth and drift to say so in numbers."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import rows_deal_model as D   # noqa: E402  (the definition of the rule)

P, NNZ, BLOCKS, NG, SLOTS, LRU_LINES, XCDS = 1_000_000, 30, 128, 64, 4, 32768, 8
W_BASE = 1 << 40   # w lines live in another address range than V lines


def streams(rng, kind):
    """[BLOCKS * NG, 120] columns, every stream ascending"""
    if kind == "even":
        n = SLOTS * NNZ
        band = np.arange(n, dtype=np.float64) * P / n
        return (band[None, :] + rng.random((BLOCKS * NG, n)) * P / n).astype(np.int64)
    out = np.empty((BLOCKS * NG, SLOTS * NNZ), np.int64)
    for b in range(BLOCKS):
        rows = np.sort(rng.integers(0, P, (256, NNZ)), axis=1)
        if kind == "deal":
            m = D.deal_map([[int(c) for c in r] for r in rows], P)
        else:
            m = D.identity_map()
        for g in range(NG):
            out[b * NG + g] = np.sort(np.concatenate([rows[m[s][g]] for s in range(SLOTS)]))
    return out


def excursion(cols):
    n = cols.shape[1]
    ramp = (np.arange(n) + 0.5) * P / n
    return float(np.mean(np.max(np.abs(cols - ramp[None, :]), axis=1)) / P)


def lines_fetched(cols, drift, rng, ahead=1):
    """(V lines, w lines) this XCD fetches: an LRU over the accesses in time order; step t's access is issued at the wave's step max(t - (ahead - 1), 0)"""
    n_streams, n = cols.shape
    offset = np.repeat(rng.normal(0.0, drift, n_streams // 16) if drift > 0 else np.zeros(n_streams // 16), 16)
    issued = np.maximum(np.arange(n, dtype=np.float64) - (ahead - 1), 0.0)
    when = (issued[None, :] + offset[:, None]).ravel()
    order = np.argsort(when, kind="stable")
    flat = cols.ravel()[order]
    v_line, w_line = (flat >> 1).tolist(), ((flat >> 5) + W_BASE).tolist()
    lru, miss_v, miss_w = {}, 0, 0
    for v, w in zip(v_line, w_line):
        for key in (v, w):
            if key in lru:
                del lru[key]
            else:
                if key >= W_BASE:
                    miss_w += 1
                else:
                    miss_v += 1
                if len(lru) >= LRU_LINES:
                    del lru[next(iter(lru))]
            lru[key] = None
    return miss_v, miss_w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--drift", type=float, nargs="*", default=[0.0, 2.0, 4.0, 8.0], help="sd of a wave's offset against the common clock, in steps")
    ap.add_argument("--ahead", type=int, nargs="*", default=[], help="look-ahead depths to price under DEAL (1: the walk that requests and consumes step by step)")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    t0 = time.time()
    sets = {}
    for kind in ("identity", "deal", "even"):
        sets[kind] = streams(np.random.default_rng(a.seed), kind)   # identity and deal see the same rows
    print(f"streams made in {time.time() - t0:.1f} s; mean largest excursion from the ramp, fraction of p: " + ", ".join(f"{k} {excursion(v):.4f}" for k, v in sets.items()))
    distinct = len(np.unique(sets["identity"] >> 1))
    print(f"distinct V lines one XCD touches: {distinct} ({XCDS * distinct / 1e6:.2f} M per tile: perfect re-use)")
    print("M lines per tile (8 XCDs):   drift   identity V / w      DEAL V / w      even V / w")
    for d in a.drift:
        row = []
        for kind in ("identity", "deal", "even"):
            v, w = lines_fetched(sets[kind], d, np.random.default_rng(a.seed + 1000))   # the same offsets for all three
            row.append(f"{XCDS * v / 1e6:6.2f} / {XCDS * w / 1e6:4.2f}")
        print(f"                             {d:5.1f}   " + "   ".join(row), flush=True)
    if a.ahead:
        print("DEAL, M lines per tile (8 XCDs), V + w, by look-ahead depth:   drift   " + "   ".join(f"AHEAD {d}" for d in a.ahead))
        for d in a.drift:
            row = []
            for depth in a.ahead:
                v, w = lines_fetched(sets["deal"], d, np.random.default_rng(a.seed + 1000), depth)
                row.append(f"{XCDS * (v + w) / 1e6:7.3f}")
            print(f"                                                               {d:5.1f}   " + "   ".join(row), flush=True)
    print(f"{time.time() - t0:.1f} s")


if __name__ == "__main__":
    main()
