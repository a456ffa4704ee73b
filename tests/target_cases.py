"""The sources the target-encoding tests share (tests/test_target_cpu.py, tests/test_gpu_target.py): made once from fixed seeds, never changed."""
import numpy as np

# the ragged source: seven segments over 41 columns
#   0 [0, 1)   a dense column of width 1     1 [1, 6) and 2 [6, 10)  a few entries a row     3 [10, 30)  a bag: most of a row's entries, columns twice
#   4 [30, 34) at most one entry a row       5 [34, 34)  empty                               6 [34, 41)  no row stores it
RAGGED_BASE = np.array([0, 1, 6, 10, 30, 34, 34, 41], np.uint32)
RAGGED_P = 41
RAGGED_LENS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1025)
RAGGED_TERMS = np.array([0, 1, 3, 5, 6], np.uint32)      # the dense column, a field, the bag, the empty segment, the segment no row stores
NO_PART = 0xFFFFFFFF


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def bits64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def ragged(seed=5, per_len=3):
    """(row_ptr, col, val, y): rows of every length of RAGGED_LENS, per_len of each, shuffled; unsorted rows, real values, columns stored twice;
    labels in {-1, +1} with a few real ones"""
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.repeat(RAGGED_LENS, per_len))
    cols = []
    for n in lens:
        c = rng.integers(1, 30, int(n))
        if n >= 2:
            c[1] = c[0]                                    # a column stored twice in the row
        if n >= 3 and rng.random() < 0.6:
            c[2] = 0                                       # the dense column, somewhere in the row
        if n >= 1 and rng.random() < 0.7:
            c[rng.integers(0, n)] = rng.integers(30, 34)   # at most one entry of segment 4
        cols.append(c)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    y = np.where(rng.random(len(lens)) < 0.5, 1.0, -1.0).astype(np.float32)
    y[::5] = rng.normal(0, 3, len(y[::5])).astype(np.float32)
    return rp, col, val, y


def ragged_parts(n, n_parts, seed=3):
    """a part per row: mostly valid, some >= n_parts, some 0xFFFFFFFF"""
    rng = np.random.default_rng(seed)
    part = rng.integers(0, n_parts, n).astype(np.uint32)
    part[rng.random(n) < 0.15] = n_parts
    part[rng.random(n) < 0.1] = NO_PART
    part[rng.random(n) < 0.05] = n_parts + 7
    part[3], part[7], part[11] = NO_PART, n_parts, n_parts + 7
    return part


# the tall source: one entry a row, column j in a block of TALL_ROWS[j] rows -- the cells of 1 023, 1 024, 1 025 and 2 049 rows at the chunk edges of the sum
TALL_ROWS = (1023, 1024, 1025, 2049, 1)
TALL_BASE = np.array([0, 5], np.uint32)
TALL_P = 5


def tall(seed=7):
    """(row_ptr, col, val, y): labels of mixed sign over 38 decimal orders of magnitude, so the order of the sum shows; column 0 holds a -0, column 1
    a +inf, column 3 a NaN with a payload, +inf and -inf, column 4 is one row with label -0"""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(len(TALL_ROWS)), TALL_ROWS).astype(np.uint32)
    n = len(col)
    with np.errstate(over="ignore"):
        y = (rng.normal(0, 1, n) * 10.0 ** rng.integers(-8, 31, n)).astype(np.float32)
    y[np.isinf(y)] = np.float32(3e38)
    y[5] = np.float32(-0.0)
    y[1023 + 17] = np.float32(np.inf)
    at = 1023 + 1024 + 1025
    y[at + 3] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    y[at + 900] = np.float32(np.inf)
    y[at + 1500] = np.float32(-np.inf)
    y[n - 1] = np.float32(-0.0)
    return np.arange(n + 1, dtype=np.int64), col, np.ones(n, np.float32), y


FIELD_VOCAB = [3, 1, 17, 300, 70000]


def field_base(dense):
    return np.concatenate([np.arange(dense), dense + np.concatenate([[0], np.cumsum(FIELD_VOCAB)])]).astype(np.uint32)
