"""The shapes tests/test_rows_deal_cpu.py (the DEAL rule's invariants) and tests/test_gpu_rows_deal.py (the device builder and the kernel under DEAL) share.

As in tests/rows_sched_cases.py every matrix is two tiles: HEAD ordinary rows of 30 ascending entries, then the tail under test as a tile of its own.  The
first three cases are that file's own (imported, not copied): mixed (rows of 0, 1, 30 and 36 entries: empty rows, tails that leave lane groups with one to
four rows and slots without one), unsorted (rows in no order, a column stored twice) and over37 (every lane group needs 148 steps whatever it is dealt: the
tile is turned away and runs the merged form).  Two are new:
  upto37   row r of the tail holds r mod 38 entries: 0..37, where it is the deal that decides whether a block fits the 144 steps
  ties64   p = 64 and every tail row is one of four patterns on multiples of four -- the cuts themselves -- so that most keys and most costs are equal and
           the tie rules (the lower row, the lowest lane group, the lowest slot) decide"""
import numpy as np

from tests import rows_sched_cases as C

HEAD = C.HEAD
K = C.K
P_TIES = 64
# name, p, the tails; `base` is the case of rows_sched_cases whose problem() makes the matrix, None for the two made here
CASES = [dict(name="mixed", p=C.P, base=C.CASES[0], tails=[1, 63, 64, 65, 255, 257]),
         dict(name="unsorted", p=C.P, base=C.CASES[4], tails=[257]),
         dict(name="over37", p=C.P, base=C.CASES[3], tails=[256]),
         dict(name="upto37", p=C.P, base=None, tails=[257]),
         dict(name="ties64", p=P_TIES, base=None, tails=[257])]
TIE_PATTERNS = [list(range(0, 64, 4)), list(range(0, 32, 4)) * 2, list(range(32, 64, 4)) * 2, [0, 4, 8, 60, 60, 4, 0, 32]]


def seed_of(ci, t):
    return 900 + 31 * ci + t


def problem(case, n_tail, seed):
    """CSR (row_ptr, col, val, y) of HEAD rows of 30 ascending columns, then n_tail rows of the case's kind; unit values"""
    if case["base"] is not None:
        return C.problem(case["base"], n_tail, seed)
    rng = np.random.default_rng(seed)
    p = case["p"]
    if case["name"] == "ties64":
        head = np.sort(np.argsort(rng.random((HEAD, p)), axis=1)[:, :30], axis=1)      # 30 of the 64 columns, ascending
        rows = [np.array(TIE_PATTERNS[(r * 7 // 3) % 4], np.int64) for r in range(n_tail)]
    else:
        width = p // 30
        head = (np.arange(30, dtype=np.int64) * width)[None, :] + rng.integers(0, width, (HEAD, 30))
        rows = [np.sort(rng.choice(p, r % 38, replace=False)) for r in range(n_tail)]
    lens = np.array([len(r) for r in rows], np.int64)
    col = np.concatenate([head.ravel()] + rows).astype(np.uint32)
    rp = np.zeros(HEAD + n_tail + 1, np.int64)
    rp[1:] = np.cumsum(np.concatenate([np.full(HEAD, 30, np.int64), lens]))
    y = np.where(rng.random(HEAD + n_tail) < 0.5, -1.0, 1.0).astype(np.float32)
    return rp, col, np.ones(len(col), np.float32), y
