"""The sources the cross tests share (tests/test_cross_cpu.py, tests/test_gpu_cross.py): made once from fixed seeds, never changed."""
import numpy as np

# the ragged source: six segments over 40 columns
#   0 [0, 5) and 1 [5, 9)   several entries a row        2 [9, 29)   a bag: most of a row's entries
#   3 [29, 33)              at most one entry a row      4 [33, 33)  empty         5 [33, 40)  no row stores it
RAGGED_BASE = np.array([0, 5, 9, 29, 33, 33, 40], np.uint32)
RAGGED_P = 40
RAGGED_LENS = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 257)
# (0, 1) exact; (1, 3) hashed into 7 buckets: collisions are certain; the bag with itself, exact and hashed; a self-cross that emits nothing; a
# term on the empty segment (width 0); a term on the segment no row stores
RAGGED_TERMS = [(0, 1), (1, 3, 7), (2, 2), (2, 2, 11), (3, 3), (2, 4), (0, 5, 5)]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def ragged(seed=5, per_len=3):
    """(row_ptr, col, val, y): rows of every length of RAGGED_LENS, per_len of each, shuffled; unsorted rows, real values, columns stored twice"""
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.repeat(RAGGED_LENS, per_len))
    cols = []
    for n in lens:
        c = rng.integers(0, 29, int(n))
        if n >= 2:
            c[1] = c[0]                                    # a column stored twice in the row
        if n >= 1 and rng.random() < 0.7:
            c[rng.integers(0, n)] = rng.integers(29, 33)   # at most one entry of segment 3
        cols.append(c)
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    y = np.where(rng.random(len(lens)) < 0.5, 1.0, -1.0).astype(np.float32)
    return rp, col, val, y


def small(seed=9):
    """a few short rows of the ragged shape, for the Python triple loop"""
    rp, col, val, y = ragged(seed, 1)
    keep = np.flatnonzero(np.diff(rp) <= 17)
    lens = np.diff(rp)[keep]
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in keep]) if len(keep) else np.zeros(0, np.int64)
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), col[idx], val[idx], y[keep]


# the value cases: rows (0: x, 1: y, 2 + r % 3: 1.0) -- a dense prefix of two and one field, so every form applies -- whose product x * y
F = lambda b: np.array([b], np.uint32).view(np.float32)[0]
VALUE_PAIRS = [
    (np.float32(1.1), np.float32(1.3)),                    # rounds
    (np.float32(16777217.0), np.float32(3.0000002)),       # rounds, many bits
    (np.float32(3e38), np.float32(10.0)),                  # overflows to +inf
    (np.float32(-3e38), np.float32(10.0)),                 # ... and to -inf
    (np.float32(1e-20), np.float32(1e-20)),                # lands in the subnormals
    (np.float32(1.5e-23), np.float32(1e-22)),              # ... at the bottom of them (rounds to the smallest ones)
    (F(0x00000001), np.float32(0.5)),                      # starts from a subnormal: a tie, to even (0)
    (F(0x00000003), np.float32(0.5)),                      # ... a tie, to even (2)
    (F(0x00400000), np.float32(1e10)),                     # a subnormal times a normal: a normal
    (F(0x00012345), F(0x00054321)),                        # subnormal times subnormal: 0
    (np.float32(-1.0), np.float32(0.0)),                   # -0
    (np.float32(-0.0), np.float32(-0.0)),                  # +0
    (np.float32(np.inf), np.float32(0.0)),                 # inf * 0: NaN
    (np.float32(-np.inf), np.float32(np.inf)),             # -inf
    (F(0x7FC12345), np.float32(2.0)),                      # a NaN payload in
    (F(0xFFC00001), np.float32(1.0)),                      # ... with the sign set
    (F(0x7F800001), F(0xFF800001)),                        # signalling NaNs
    (np.float32(1.0), np.float32(1.0)),
]
VALUE_BASE = np.array([0, 1, 2, 5], np.uint32)
VALUE_TERMS = [(0, 1), (0, 2), (1, 2, 3), (0, 1, 4)]


def values():
    """(row_ptr, col, val, y, p)"""
    n = len(VALUE_PAIRS)
    col = np.stack([np.zeros(n), np.ones(n), 2 + np.arange(n) % 3], axis=1).astype(np.uint32).ravel()
    val = np.stack([bits(np.array([a for a, _ in VALUE_PAIRS], np.float32)), bits(np.array([b for _, b in VALUE_PAIRS], np.float32)),
                    np.full(n, 0x3F800000, np.uint32)], axis=1).ravel().view(np.float32)
    return np.arange(n + 1, dtype=np.int64) * 3, col, val, None, 5
