"""The definition of the flags an fmx_matrix carries about its rows -- rows_sorted, unit_values, fixed_row_len, max_row_len and the field layout
(dense_prefix, field_base) -- restated from the exported CSR alone, in numpy.  Every kernel trusts these flags (a one-hot matrix's values are never
read, sorted rows open the merged forms, a fixed row length turns "row of an entry" into a division, a layout selects the per-field plan builder),
so the tests hold the library to THIS file, not to the flags of a second upload.

truth(...)  what the detector must find on these rows (fm_ingest.hip: check_rows_sorted, detect_fields' documented rule).
sound(...)  the weaker question for flags a producer claims without looking at the rows: is every claim true of the rows?

tests/test_flags_cpu.py holds truth to a brute-force loop; tests/test_gpu_flags.py holds the library to truth and sound."""
import numpy as np

MAX_FIELDS = 64             # FMX_MAX_FIELDS (fmx_internal.h)
ONE_BITS = 0x3F800000       # 1.0f
FLAG_KEYS = ("rows_sorted", "unit_values", "fixed_row_len", "max_row_len")


def _arrays(row_ptr, col, val):
    rp = np.asarray(row_ptr, np.int64)
    col = np.asarray(col).astype(np.int64)
    bits = np.ascontiguousarray(val, np.float32).view(np.uint32)
    assert rp[0] == 0 and len(col) == len(bits) == int(rp[-1])
    return rp, col, bits


def no_layout():
    return dict(dense_prefix=0, field_base=[])


def truth(row_ptr, col, val, p):
    """(flags, layout): flags a dict over FLAG_KEYS, layout dict(dense_prefix, field_base) with field_base [] where the rule finds none"""
    rp, col, bits = _arrays(row_ptr, col, val)
    n, nnz = len(rp) - 1, len(col)
    lens = np.diff(rp)
    # strictly ascending inside every row: an adjacent pair that does not ascend and does not straddle a row start
    starts = np.zeros(nnz + 1, bool)
    starts[rp[:-1]] = True          # (an empty row marks the start of the next stored entry, or position nnz)
    bad = (col[:-1] >= col[1:]) & ~starts[1:nnz] if nnz > 1 else np.zeros(0, bool)
    flags = dict(rows_sorted=int(not bad.any()),
                 unit_values=int(bool(np.all(bits == ONE_BITS))),
                 max_row_len=int(lens.max()) if n > 0 else 0,
                 fixed_row_len=0)
    if n > 0 and lens[0] > 0 and np.all(lens == lens[0]):
        flags["fixed_row_len"] = int(lens[0])
    return flags, _layout_rule(flags, col, bits, n, nnz, p)


def _layout_rule(flags, col, bits, n, nnz, p):
    z = flags["fixed_row_len"]
    if not (flags["rows_sorted"] and 1 <= z <= 64 and nnz > 0):
        return no_layout()
    c2 = col.reshape(n, z)
    lo, hi = c2.min(axis=0), c2.max(axis=0)
    d = 0
    while d < z and lo[d] == d and hi[d] == d:
        d += 1
    if flags["unit_values"]:
        d = 0
    C = z - d
    if not 1 <= C <= MAX_FIELDS:
        return no_layout()
    if np.any(bits.reshape(n, z)[:, d:] != ONE_BITS):
        return no_layout()
    if np.any(lo[d + 1:] <= hi[d:z - 1]):
        return no_layout()
    base = [d] + [int(lo[d + c]) for c in range(1, C)] + [int(p)]
    return dict(dense_prefix=d, field_base=base)


def sound(flags, layout, row_ptr, col, val, p):
    """the claims of (flags, layout) that the rows contradict, as a list of strings: [] is sound"""
    rp, col, bits = _arrays(row_ptr, col, val)
    n = len(rp) - 1
    lens = np.diff(rp)
    t, _ = truth(row_ptr, col, val, p)
    wrong = []
    if flags["rows_sorted"] and not t["rows_sorted"]:
        wrong.append("rows_sorted claimed, some row does not ascend strictly")
    if flags["unit_values"] and not t["unit_values"]:
        wrong.append("unit_values claimed, some value is not 1.0f")
    z = flags["fixed_row_len"]
    if z < 0 or (z > 0 and not np.all(lens == z)):
        wrong.append(f"fixed_row_len {z} claimed, row lengths {sorted(set(lens.tolist()))[:5]}")
    if flags["max_row_len"] < t["max_row_len"]:
        wrong.append(f"max_row_len {flags['max_row_len']} claimed, the longest row holds {t['max_row_len']}")
    base = [int(b) for b in layout["field_base"]]
    d = int(layout["dense_prefix"])
    if not base:
        if d != 0:
            wrong.append(f"dense_prefix {d} without a layout")
        return wrong
    C = len(base) - 1
    if not (1 <= C <= MAX_FIELDS and base[0] == d and base[C] == p and all(base[c] < base[c + 1] for c in range(C))):
        wrong.append(f"layout d={d} base={base} is not d = base[0] < ... < base[C] = p ({p})")
        return wrong
    if z != d + C:
        wrong.append(f"layout of d={d} + {C} fields on fixed_row_len {z}")
        return wrong
    if not np.all(lens == z):
        return wrong    # (already reported above)
    c2, b2 = col.reshape(n, z), bits.reshape(n, z)
    if np.any(c2[:, :d] != np.arange(d)[None, :]):
        wrong.append("a row does not start with columns 0 .. d-1")
    b = np.asarray(base, np.int64)
    if np.any(c2[:, d:] < b[None, :C]) or np.any(c2[:, d:] >= b[None, 1:]):
        wrong.append("a field id lies outside its range")
    if np.any(b2[:, d:] != ONE_BITS):
        wrong.append("a field entry's value is not 1.0f")
    return wrong
