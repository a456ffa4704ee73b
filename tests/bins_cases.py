"""The matrices of the value-binning tests (tests/test_bins_cpu.py, tests/test_gpu_bins.py): small CSR arrays whose columns hold the values at
which a binning can go wrong."""
import numpy as np

P = 12
EDGE_VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 1e-45, 3.0, np.inf], np.float32)
NANS = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)   # quiet and signalling, both signs
COUNTS = (0, 1, 2, 3, 63, 64, 65, 1023, 1024, 1025)


def mixed(seed=1, n=200):
    """200 ragged rows over a dozen columns: 0 normal values, 1 half-integer ties, 2 the edge values {-inf, -1, -0, +0, 1e-45, 3, +inf}, 3 all
    equal, 4 never stored, 5 normal values and NaNs of both signs, 6 NaNs alone, 7 subnormals, 8 - 11 normal values; a column stored twice in
    some rows.  Returns (row_ptr, col, val, y)."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([[0, 1, 2, 0, 40, 1], rng.integers(0, 14, n - 6)])
    nnz = int(lens.sum())
    col = rng.integers(0, P, nnz)
    col[col == 4] = 0
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for r in (4, 9, 20, 33):                    # a column stored twice in a row
        if rp[r + 1] - rp[r] >= 2:
            col[rp[r] + 1] = col[rp[r]]
    val = rng.normal(0, 1, nnz).astype(np.float32)
    at = col == 1
    val[at] = np.round(val[at] * 2) / 2
    at = col == 2
    val[at] = EDGE_VALUES[rng.integers(0, len(EDGE_VALUES), int(at.sum()))]
    val[col == 3] = np.float32(2.5)
    at = np.flatnonzero(col == 5)
    pick = at[rng.random(len(at)) < 0.3]
    val[pick] = NANS[rng.integers(0, len(NANS), len(pick))]
    at = col == 6
    val[at] = NANS[rng.integers(0, len(NANS), int(at.sum()))]
    at = col == 7
    val[at] = (rng.integers(-40, 40, int(at.sum())).astype(np.float64) * 1.4e-45).astype(np.float32)
    y = np.where(rng.random(n) < 0.4, 1.0, -1.0).astype(np.float32)
    return rp, col.astype(np.uint32), val, y


def counted(seed=2):
    """Column j of 10 holds exactly COUNTS[j] stored entries (normal values, some tied), interleaved in ragged rows; column 5 is stored twice in one
    row.  Returns (row_ptr, col, val, y, p)."""
    rng = np.random.default_rng(seed)
    col = np.repeat(np.arange(len(COUNTS)), COUNTS)
    rng.shuffle(col)
    nnz = len(col)
    cuts = np.sort(rng.integers(0, nnz + 1, 299))
    rp = np.concatenate([[0], cuts, [nnz]]).astype(np.int64)
    lens = np.diff(rp)
    r = int(np.flatnonzero(lens >= 2)[0])
    a = int(rp[r])
    for want, at in ((5, a), (5, a + 1)):       # swap so that the counts stay what they are
        if col[at] != want:
            other = np.flatnonzero(col == want)
            other = other[(other != a) & (other != a + 1)][0]
            col[other], col[at] = col[at], want
    val = rng.normal(0, 3, nnz).astype(np.float32)
    tie = rng.random(nnz) < 0.2
    val[tie] = np.round(val[tie])
    y = rng.normal(0, 1, len(rp) - 1).astype(np.float32)
    return rp, col.astype(np.uint32), val, y, len(COUNTS)


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x
