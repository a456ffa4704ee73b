"""The check-ins of phase 1's pace (fm_rows_sched_k<.., PACE>, fm_batch_kernels.hip), as a definition: what a paced launch leaves in the engine's counters.

A block of T_b steps (tests/rows_sched_model.py, tests/rows_deal_model.py: the steps of its schedule, the DEAL header not counted) is walked by one
workgroup, and the WORKGROUP checks in -- one lane of one of its waves (the four take turns) adds 1 to the counter of the block's label, blockIdx.x mod 8 -- behind the sums of
the steps t = E, 2 E, 3 E, ... < T_b, E = EVERY steps apart: never at step 0, where nobody leads, so

    a block checks in   max(0, (T_b - 1) // E)   times,

and a launch of blocks 0 .. B - 1 leaves  the sum over the blocks b with b mod 8 == l of that number  in counter l of the set it used (paced launch n of
an engine: set n & 1) and zeros in the other set, which it clears for the launch after it."""
import numpy as np

EVERY = 24
LABELS = 8


def block_checkins(t_b, every=EVERY):
    return max(0, (int(t_b) - 1) // every)


def launch_counters(steps, every=EVERY):
    """int64 [8]: counter l after a paced launch whose block b has steps[b] steps"""
    out = np.zeros(LABELS, np.int64)
    for b, t in enumerate(steps):
        out[b % LABELS] += block_checkins(t, every)
    return out
