"""The shapes tests/test_rows_sched_cpu.py (the model's invariants) and tests/test_gpu_rows_sched.py (the device builder and fm_rows_sched_k) share.

The scheduled form exists on the large-step path only (256-thread workgroups: steps of at least 32 768 four-lane rows), and a schedule is used for exactly
a tile's rows, so every matrix is two tiles: HEAD ordinary rows of 30 sorted entries, then the tail under test as a tile of its own -- 1, 63, 64, 65, 255,
256, 257 or 1 000 rows: a last workgroup that is partly filled, lane groups with one to four rows, slots without a row.  The tails:
  mixed     rows of 0, 1, 30 and 36 entries next to each other
  full36    every row 36 entries: 4 x 36 = 144 steps under MERGE, 144 x 256 B = the stage exactly
  over37    every row 37 entries: more than 144 steps; the launch must be turned away
  unsorted  rows whose entries are not ascending, with a column stored twice: the row's own order must still be kept
  ragged    the four rows of lane group 5 hold 32 entries each, every other row 8: one lane group with four times the entries of the others"""
import numpy as np

HEAD = 32768
P = 5000
K = 16
ALL_TAILS = [1, 63, 64, 65, 255, 256, 257, 1000]
CASES = [dict(name="mixed", tail="mixed", wir=0, tails=ALL_TAILS),
         dict(name="mixed_wir", tail="mixed", wir=1, tails=[65, 1000]),
         dict(name="full36", tail="full36", wir=0, tails=[256, 1000]),
         dict(name="over37", tail="over37", wir=0, tails=[256]),
         dict(name="unsorted", tail="unsorted", wir=0, tails=[257]),
         dict(name="ragged", tail="ragged", wir=1, tails=[256, 1000])]
# (name, the model's policy, its rho in 1024ths); only MERGE has a device form, FRONT and ROUND exist in the model alone (tests/rows_sched_model.py)
POLICIES = [("merge", 0, 0), ("front", 1, 922), ("round", 2, 0), ("round_front", 2, 922)]


def tail_lengths(kind, n):
    if kind == "mixed":
        return np.resize(np.array([0, 1, 30, 36, 30, 0, 36, 1, 30, 30, 36], np.int64), n)
    if kind == "full36":
        return np.full(n, 36, np.int64)
    if kind == "over37":
        return np.full(n, 37, np.int64)
    if kind == "ragged":
        return np.where(np.arange(n) % 64 == 5, 32, 8).astype(np.int64)
    return np.full(n, 30, np.int64)


def problem(case, n_tail, seed):
    """CSR of HEAD rows of 30 ascending columns (one per stratum of the features), then n_tail rows of the case's kind; unit values"""
    rng = np.random.default_rng(seed)
    width = P // 30
    head = (np.arange(30, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (HEAD, 30))
    lens = tail_lengths(case["tail"], n_tail)
    rows = []
    for r, n in enumerate(lens):
        c = np.sort(rng.choice(P, n, replace=False))
        if case["tail"] == "unsorted" and n >= 4:
            c = c[::-1].copy() if r % 3 == 0 else rng.permutation(c)   # descending, or no order at all ...
            c[n // 2] = c[1]                                            # ... and one column twice
        rows.append(c)
    col = np.concatenate([head.ravel()] + rows).astype(np.uint32)
    rp = np.zeros(HEAD + n_tail + 1, np.int64)
    rp[1:] = np.cumsum(np.concatenate([np.full(HEAD, 30, np.int64), lens]))
    y = np.where(rng.random(HEAD + n_tail) < 0.5, -1.0, 1.0).astype(np.float32)
    return rp, col, np.ones(len(col), np.float32), y


def seed_of(ci, t):
    return 100 + 17 * ci + t
