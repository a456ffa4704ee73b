"""The case table of the flag detector's tests (tests/test_flags_cpu.py, tests/test_gpu_flags.py): small matrices that each change ONE thing about a
base matrix, placed on the seams of the detector's decomposition -- 64 lanes per atomic, 256 threads and 4 096 entries per block of the entry scan,
256 rows per block of the row scan, 256 counter slots.  A case is a dict: rp, col, val, p, plus what it promises about itself (`t`: the planted
entry, `row`: the planted row, `expect`: flags that must differ from the clean twin `clean`), which the CPU test checks, so that a case that no
longer sits on its seam fails without a GPU.

build(name) makes a case (deterministic, cached); NAMES lists them by section."""
import zlib

import numpy as np

P = 1000
N_BASE = 700
BLOCK = 4096                     # entries per block of the entry scan (256 threads x 16)
SLOTS = 256
WRAP_NNZ = 257 * BLOCK + 1       # block 256 shares counter slot 0 with block 0
F32 = np.float32
ODD_VALUES = {"up": np.uint32(0x3F800001).view(F32), "down": np.uint32(0x3F7FFFFF).view(F32), "neg": F32(-1.0), "zero": F32(0.0),
              "nan": F32(np.nan), "inf": F32(np.inf)}     # 1 + 2^-23, 1 - 2^-24, ...
T_PAIRS = [0, 62, 63, 64, 254, 255, 256, 4094, 4095, 4096, "nnz-2"]
T_VALUES = [0, 63, 64, 255, 256, 4095, 4096, "nnz-1"]
SEAM_ROWS = [0, 62, 63, 64, 254, 255, 256, "n-2"]
LEN_ROWS = [0, 63, 64, 255, 256, "n-1"]
_cache = {}


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _rows(rng, lens, p=P, lo=0):
    """strictly ascending rows of the given lengths, columns in [lo, p)"""
    if len(lens) == 0 or int(np.sum(lens)) == 0:
        return np.zeros(0, np.uint32)
    return np.concatenate([np.sort(rng.choice(p - lo, int(k), replace=False)) + lo for k in lens if k > 0]).astype(np.uint32)


def _case(lens, col, val=None, p=P, **promise):
    rp = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))]).astype(np.int64)
    col = np.ascontiguousarray(col, np.uint32)
    val = np.ones(len(col), F32) if val is None else np.ascontiguousarray(val, F32)
    assert len(col) == len(val) == rp[-1]
    return dict(rp=rp, col=col, val=val, p=p, **promise)


def _spread(rng, lens, target, keep=()):
    """move `lens` (each 0 .. 20) to the sum `target`, rows in `keep` stay at least 1"""
    lens = np.asarray(lens, np.int64).copy()
    for r in keep:
        lens[r] = max(lens[r], 1)
    diff = int(target - lens.sum())
    for r in rng.permutation(len(lens)):
        if diff == 0:
            break
        step = min(20 - lens[r], diff) if diff > 0 else -min(lens[r] - (1 if r in keep else 0), -diff)
        lens[r] += step
        diff -= step
    assert diff == 0, "the rows cannot hold this many entries"
    return lens


def base_lens(seed=0):
    """700 rows of 0 .. 20 entries, nnz between 4 200 and 9 000"""
    lens = _rng("base", seed).integers(0, 21, N_BASE)
    assert 4200 <= lens.sum() <= 9000
    return lens


def _together(lens, t):
    """the base's row cuts, moved so that entries t and t + 1 share a row (row lengths stay within 0 .. 20)"""
    lens = lens.copy()
    rp = np.concatenate([[0], np.cumsum(lens)])
    ra, rb = int(np.searchsorted(rp, t, "right")) - 1, int(np.searchsorted(rp, t + 1, "right")) - 1   # rows of t and t + 1
    if ra != rb:
        if lens[ra] < 20:
            lens[ra] += 1; lens[rb] -= 1       # t + 1 joins t's row
        else:
            assert lens[rb] < 20
            lens[ra] -= 1; lens[rb] += 1       # t joins t + 1's row
    return lens


def _resolve(t, nnz, n=None):
    if isinstance(t, str):
        what, off = t.split("-")
        return (nnz if what == "nnz" else n) - int(off)
    return t


# ---------------------------------------------------------------------------------------------------------------- section: order inside rows and at seams
def clean():
    lens = base_lens()
    return _case(lens, _rows(_rng("clean"), lens))


def in_row(t, kind):
    """one descent (the pair swapped) or one tie (the second made equal to the first) between entries t and t + 1 of one row"""
    lens0 = base_lens()
    t = _resolve(t, int(lens0.sum()))
    lens = _together(lens0, t)
    col = _rows(_rng("in_row", t), lens)
    twin = _case(lens, col.copy())
    if kind == "descent":
        col[t], col[t + 1] = col[t + 1], col[t]
    else:
        col[t + 1] = col[t]
    return _case(lens, col, t=t, pair="in_row", twin=twin, expect=dict(rows_sorted=0))


def seam(t, row, gap, kind):
    """entry t is the last of row `row`, then `gap` empty rows, then t + 1 opens the next row with col[t] >= col[t + 1] ('down': smaller, 'tie': equal);
    `row` None: a row that fits t.  Every row ascends strictly: rows_sorted stays 1."""
    n, total = N_BASE, 7000
    rng = _rng("seam", t, row, gap, kind)
    last_pair = t == "nnz-2"
    t = _resolve(t, total)
    row = _resolve(row, None, n) if row is not None else (t + 1) // 12
    assert row + gap + 1 <= n - 1, "no room for the rows after the seam"
    head = _spread(rng, rng.integers(0, 21, row + 1), t + 1, keep=(row,))
    n_tail = n - (row + gap + 1)
    if last_pair:
        tail = np.zeros(n_tail, np.int64); tail[0] = 1       # (t + 1 is the last entry: trailing empty rows after it)
    else:
        tail = _spread(rng, rng.integers(0, 21, n_tail), min(total - (t + 1), 20 * n_tail), keep=(0,))
    lens = np.concatenate([head, np.zeros(gap, np.int64), tail])
    col = _rows(rng, lens)
    a, b = int(lens[row]), int(lens[row + gap + 1])
    col[t + 1 - a:t + 1] = _rows(rng, [a], p=500, lo=1)      # the row that ends in t: columns 1 .. 499
    col[t + 1:t + 1 + b] = _rows(rng, [b], lo=500)           # the row that t + 1 opens: 500 .. 999, then its first entry is planted below them
    col[t + 1] = col[t] if kind == "tie" else col[t] - 1
    return _case(lens, col, t=t, row=row, gap=gap, pair="seam")


def many_seams(which):
    rng = _rng("many", which)
    if which == "every_row":        # every row draws from the same 40 columns: nearly every seam descends; empty rows in between and at the end
        lens = rng.integers(0, 21, N_BASE); lens[rng.random(N_BASE) < 0.2] = 0; lens[-9:] = 0
        return _case(lens, _rows(rng, lens, p=40), p=40, pair="many")
    if which == "empty_rows_only":
        return _case(np.zeros(N_BASE, np.int64), np.zeros(0, np.uint32), pair="many")
    if which == "one_row":
        return _case([5], _rows(rng, [5]), pair="many")
    if which == "one_entry":
        return _case([0, 1, 0], [7], pair="many")
    if which == "no_rows":
        return _case([], np.zeros(0, np.uint32), pair="many")
    raise KeyError(which)


def wrap(which):
    """nnz = 257 x 4 096 + 1: single-entry rows (every adjacent pair is a seam, about half of them descending), the planted pair in block 256, whose
    counts land in the slot of block 0"""
    rng = _rng("wrap")
    col = rng.integers(0, P, WRAP_NNZ).astype(np.uint32)
    lens = np.ones(WRAP_NNZ, np.int64)
    t256, t0 = 256 * BLOCK + 100, 1000
    planted = []

    def two_entry_row(t, descend):
        nonlocal lens
        rp = np.concatenate([[0], np.cumsum(lens)])
        r = int(np.searchsorted(rp, t, "right")) - 1
        lens = np.concatenate([lens[:r], [2], lens[r + 2:]])
        a, b = 100, 900
        col[t], col[t + 1] = (b, a) if descend else (a, b)
        planted.append(t)

    if which == "in_row_256":
        two_entry_row(t256, True)
    elif which == "seam_256":
        col[t256], col[t256 + 1] = 900, 100
        planted.append(t256)
    elif which == "both":
        two_entry_row(t256, True)
        two_entry_row(t0, True)
    elif which == "ascending_rows_256":      # the twin of in_row_256: the same two-entry row, ascending
        two_entry_row(t256, False)
    else:
        raise KeyError(which)
    return _case(lens, col, planted=planted, pair="wrap")


# ---------------------------------------------------------------------------------------------------------------- section: values
def odd_value(t, name):
    c = clean()
    t = _resolve(t, len(c["col"]))
    val = c["val"].copy()
    val[t] = ODD_VALUES[name]
    return dict(c, val=val, t=t, twin=c, expect=dict(unit_values=0))


# ---------------------------------------------------------------------------------------------------------------- section: row lengths
def all_rows(z):
    lens = np.full(300, z)
    return _case(lens, _rows(_rng("all_rows", z), lens))


def one_row_differs(row, how, z=5, n=300):
    row = _resolve(row, None, n)
    lens = np.full(n, z); lens[row] = {"shorter": z - 1, "longer": z + 1, "empty": 0}[how]
    return _case(lens, _rows(_rng("one_row", row, how), lens), row=row, z=z, how=how)


def longest_row(row):
    lens = base_lens()
    row = _resolve(row, None, len(lens))
    lens[row] = 25
    return _case(lens, _rows(_rng("longest", row), lens), row=row, longest=25)


# ---------------------------------------------------------------------------------------------------------------- section: field layouts
def fields(n=300, z=30, d=0, dense="real", vocab=None, seed=0, gapped=True):
    """rows of [columns 0 .. d-1 | one id of each of z - d fields]; returns the case and the vocabularies' bases (wider than the ids that occur when
    `gapped`: the first and last id of every vocabulary are never drawn)"""
    rng = _rng("fields", n, z, d, dense, seed)
    C = z - d
    vocab = rng.integers(5, 12, C) if vocab is None else np.asarray(vocab)
    base = d + np.concatenate([[0], np.cumsum(vocab)])
    ids = np.stack([base[c] + rng.integers(1 if gapped else 0, vocab[c] - (1 if gapped else 0), n) for c in range(C)], axis=1)
    col = np.concatenate([np.tile(np.arange(d), (n, 1)), ids], axis=1).astype(np.uint32)
    val = np.ones((n, z), F32)
    if dense == "real":
        val[:, :d] = rng.normal(0, 1, (n, d)).astype(F32)
        val[:, :d][val[:, :d] == 1.0] = 0.5
    c = _case(np.full(n, z), col.ravel(), val.ravel(), p=int(base[-1]), d=d, vocab_base=[int(b) for b in base])
    return c


def fields_case(which):
    if which.startswith("clean"):                  # clean_z30_d3
        _, z, d = which.split("_")
        return fields(z=int(z[1:]), d=int(d[1:]))
    if which.startswith("unit_dense"):             # unit_dense_d3: the dense values all 1 -> d = 0, every position a field
        return fields(z=30, d=int(which[-1]), dense="ones")
    if which.startswith("z"):                      # z1, z2, z64, z65 (z64: FMX_MAX_FIELDS fields; z65: one more, and a row too long for the rule)
        return fields(z=int(which[1:]), d=0)
    c = fields(z=39 if which == "last_row_extremes" else 30, d=3)
    n, z, d = len(c["rp"]) - 1, int(c["rp"][1]), 3
    col, val, vb = c["col"].reshape(n, z).copy(), c["val"].reshape(n, z).copy(), c["vocab_base"]
    f = 7                                           # a field in the middle; its position in the row
    pos = d + f
    if which == "touch":                            # hi[f - 1] + 1 == lo[f]: still disjoint
        col[5, pos - 1] = vb[f] - 1; col[7, pos] = vb[f]
        c["touch"] = (int(vb[f]) - 1, int(vb[f]))
    elif which == "meet":                           # lo[f] == hi[f - 1] = X, in two different rows; both rows still ascend
        X = vb[f]
        col[5, pos - 1] = X; col[7, pos] = X
        assert col[5, pos] > X and col[7, pos - 1] < X
        c["meet"] = int(X)
    elif which in ("odd_value_last", "odd_value_4096"):
        t = n * z - 1 if which == "odd_value_last" else BLOCK
        assert t % z >= d
        val.ravel()[t] = ODD_VALUES["up"]
        c["t"] = t
    elif which == "last_row_extremes":              # field 4's smallest id and field 9's largest id occur in the last row alone
        col[n - 1, d + 4] = vb[4]; col[n - 1, d + 9] = vb[10] - 1
        c["extremes"] = (d + 4, int(vb[4]), d + 9, int(vb[10]) - 1)
    else:
        raise KeyError(which)
    return dict(c, col=col.ravel(), val=val.ravel())


def set_fields_case(row):
    """a qualifying matrix of 300 rows (d = 1, four fields) in which `row` ALONE holds the smallest id that occurs of field 2: the bases the detector
    finds hold every row; the same bases with base[2] one higher are violated by that row only"""
    c = fields(z=5, d=1, seed=11)
    n = 300
    row = _resolve(row, None, n)
    col = c["col"].reshape(n, 5).copy()
    lo = int(col[:, 3].min())
    col[:, 3] = np.maximum(col[:, 3], lo + 1)
    col[row, 3] = lo
    assert lo + 1 < c["vocab_base"][3]
    return dict(c, col=col.ravel(), row=row, lowest=lo)


# ---------------------------------------------------------------------------------------------------------------- section: in-place changes
def all_twos(kind):
    """stored values all 2: normalize(mean 0, std 2) makes every one exactly 1 -- on field rows (the layout must appear) and on ragged rows"""
    c = fields(z=6, d=0, seed=5) if kind == "fields" else clean()
    return dict(c, val=np.full(len(c["col"]), 2.0, F32))


def normalized(val, col, mean, std):
    """normalize_apply_k, restated: (float)(((double)val - mean[col]) / std[col]) where std[col] != 0"""
    m, s = np.asarray(mean, np.float64)[col], np.asarray(std, np.float64)[col]
    out = np.asarray(val, F32).copy()
    nz = s != 0
    out[nz] = ((out[nz].astype(np.float64) - m[nz]) / s[nz]).astype(F32)
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
GAPS = [0, 1, 70]
SECTIONS = {
    "in_row": [("in_row", (t, k)) for t in T_PAIRS for k in ("descent", "tie")],
    "seam": [("seam", (t, None, g, "down")) for t in T_PAIRS for g in GAPS]
            + [("seam", (7 * (N_BASE - 2 if r == "n-2" else r) + 3, r, g, "tie")) for r in SEAM_ROWS for g in GAPS if not (r == "n-2" and g > 0)],
    "many": [("many_seams", (w,)) for w in ("every_row", "empty_rows_only", "one_row", "one_entry", "no_rows")],
    "wrap": [("wrap", (w,)) for w in ("in_row_256", "seam_256", "both", "ascending_rows_256")],
    "value": [("odd_value", (t, v)) for t in T_VALUES for v in ODD_VALUES],
    "lengths": [("all_rows", (z,)) for z in (1, 2, 30, 64, 65)]
               + [("one_row_differs", (r, h)) for r in LEN_ROWS for h in ("shorter", "longer", "empty")]
               + [("longest_row", (r,)) for r in LEN_ROWS],
    "fields": [("fields_case", (w,)) for w in ("clean_z30_d0", "clean_z30_d1", "clean_z30_d3", "clean_z39_d0", "clean_z39_d1", "clean_z39_d3",
                                               "unit_dense_d1", "unit_dense_d3", "touch", "meet", "odd_value_last", "odd_value_4096",
                                               "last_row_extremes", "z1", "z2", "z64", "z65")],
    "set_fields": [("set_fields_case", (r,)) for r in (0, 255, 256, "n-1")],
}


def name_of(fn, args):
    return fn + "(" + ",".join(str(a) for a in args) + ")"


NAMES = {s: [name_of(f, a) for f, a in v] for s, v in SECTIONS.items()}
_BY_NAME = {name_of(f, a): (f, a) for v in SECTIONS.values() for f, a in v}


def build(name):
    if name not in _cache:
        f, a = _BY_NAME[name]
        if f == "wrap":          # (4 MB each: not kept)
            return globals()[f](*a)
        _cache[name] = globals()[f](*a)
    return _cache[name]
