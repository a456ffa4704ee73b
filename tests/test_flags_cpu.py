"""tests/flags_model.py (the definition of a matrix's flags) against a brute-force loop over lists, against the detector's own formulation (descents over
all adjacent entries minus descents at row seams, empty rows skipped), and the promises of the case table (tests/flags_cases.py): the planted entry
sits where the case says, nnz crosses the seam it names.  No GPU."""
import numpy as np
import pytest

from tests import flags_cases as fc
from tests import flags_model as fm

ALL = [n for s in fc.NAMES.values() for n in s]


def _host(c):
    return c["rp"], c["col"], c["val"], c["p"]


def brute(rp, col, val, p):
    """the definition once more, with lists, sorted() and integer compares"""
    rp, col = np.asarray(rp).tolist(), np.asarray(col).tolist()     # (Python ints from here on)
    bits = np.ascontiguousarray(val, np.float32).view(np.uint32).tolist()
    n = len(rp) - 1
    rows = [col[rp[r]:rp[r + 1]] for r in range(n)]
    lens = [len(r) for r in rows]
    flags = dict(rows_sorted=int(all(len(r) < 2 or r == sorted(set(r)) for r in rows)), unit_values=int(all(b == 0x3F800000 for b in bits)),
                 max_row_len=max(lens, default=0), fixed_row_len=lens[0] if n > 0 and lens[0] > 0 and len(set(lens)) == 1 else 0)
    z = flags["fixed_row_len"]
    none = dict(dense_prefix=0, field_base=[])
    if not flags["rows_sorted"] or not 1 <= z <= 64 or not col:
        return flags, none
    at = [[r[i] for r in rows] for i in range(z)]
    d = 0
    while d < z and set(at[d]) == {d}:
        d += 1
    if flags["unit_values"]:
        d = 0
    C = z - d
    if C < 1 or C > 64:
        return flags, none
    for r in range(n):
        if any(b != 0x3F800000 for b in bits[rp[r] + d:rp[r + 1]]):
            return flags, none
    for i in range(d + 1, z):
        if min(at[i]) <= max(at[i - 1]):
            return flags, none
    return flags, dict(dense_prefix=d, field_base=[d] + [min(at[d + c]) for c in range(1, C)] + [p])


def detector_rows_sorted(rp, col):
    """check_rows_sorted's count: every adjacent pair that does not ascend, minus those where a non-empty row's last entry meets the next stored entry"""
    col = np.asarray(col).tolist()
    nnz = len(col)
    descents = sum(col[t] >= col[t + 1] for t in range(nnz - 1))
    seams = sum(1 for a, b in zip(rp[:-1].tolist(), rp[1:].tolist()) if b > a and b < nnz and col[b - 1] >= col[b])
    return int(descents == seams)


@pytest.mark.parametrize("name", ALL)
def test_truth_is_the_brute_force_definition_and_the_detectors_count(name):
    c = fc.build(name)
    flags, layout = fm.truth(*_host(c))
    bf, bl = brute(*_host(c))
    assert flags == bf and layout == bl
    assert detector_rows_sorted(c["rp"], c["col"]) == flags["rows_sorted"]
    assert fm.sound(flags, layout, *_host(c)) == []


def _same_row(c, t):
    rp = c["rp"]
    r = int(np.searchsorted(rp, t, "right")) - 1
    return rp[r] <= t and t + 1 < rp[r + 1]


@pytest.mark.parametrize("name", fc.NAMES["in_row"])
def test_in_row_cases_plant_one_pair_inside_a_row(name):
    c = fc.build(name)
    t, twin = c["t"], c["twin"]
    nnz = len(c["col"])
    assert 4200 <= nnz <= 9000 and len(c["rp"]) - 1 == fc.N_BASE and np.diff(c["rp"]).max() <= 20
    assert _same_row(c, t) and c["col"][t] >= c["col"][t + 1]
    assert ("tie" in name) == bool(c["col"][t] == c["col"][t + 1])
    col = c["col"].astype(np.int64)
    assert int(np.sum(col[:-1] >= col[1:])) - int(np.sum(twin["col"][:-1].astype(np.int64) >= twin["col"][1:])) == 1   # one pair, nothing else
    tf, tl = fm.truth(*_host(twin))
    f, l = fm.truth(*_host(c))
    assert tf["rows_sorted"] == 1 and tf["unit_values"] == 1 and f == dict(tf, rows_sorted=0) and l == fm.no_layout()


def test_in_row_positions_cover_the_lane_wave_and_block_seams():
    ts = sorted(fc.build(n)["t"] for n in fc.NAMES["in_row"] if "descent" in n)
    nnz = len(fc.clean()["col"])
    assert ts == [0, 62, 63, 64, 254, 255, 256, 4094, 4095, 4096, nnz - 2] and nnz > fc.BLOCK + 2


@pytest.mark.parametrize("name", fc.NAMES["seam"])
def test_seam_cases_descend_between_rows_only(name):
    c = fc.build(name)
    rp, col, t, row, gap = c["rp"], c["col"], c["t"], c["row"], c["gap"]
    assert 4200 <= len(col) <= 9000 and len(rp) - 1 == fc.N_BASE and np.diff(rp).max() <= 20
    assert rp[row] <= t and rp[row + 1] == t + 1                                  # t closes row `row`
    assert np.all(rp[row + 1:row + gap + 2] == t + 1) and rp[row + gap + 2] > t + 1  # `gap` empty rows, then t + 1 opens one
    assert col[t] >= col[t + 1] and ("tie" in name) == bool(col[t] == col[t + 1])
    flags, _ = fm.truth(*_host(c))
    assert flags["rows_sorted"] == 1 and flags["unit_values"] == 1


def test_seam_cases_cover_the_named_entries_and_rows():
    cs = [fc.build(n) for n in fc.NAMES["seam"]]
    nnz = 7000
    for g in fc.GAPS:
        assert {c["t"] for c in cs if c["gap"] == g} >= {0, 62, 63, 64, 254, 255, 256, 4094, 4095, 4096, nnz - 2}
        assert {c["row"] for c in cs if c["gap"] == g} >= {0, 62, 63, 64, 254, 255, 256}
    assert fc.N_BASE - 2 in {c["row"] for c in cs if c["gap"] == 0}
    last = [c for c in cs if c["t"] == nnz - 2]
    assert last and all(len(c["col"]) == nnz for c in last)


def test_many_seams_descend_at_many_rows_and_never_inside_one():
    c = fc.build("many_seams(every_row)")
    rp, col = c["rp"], c["col"].astype(np.int64)
    assert int(np.sum(col[:-1] >= col[1:])) > 300 and fm.truth(*_host(c))[0]["rows_sorted"] == 1
    assert np.all(np.diff(rp)[-9:] == 0) and np.sum(np.diff(rp) == 0) > 50
    assert len(fc.build("many_seams(empty_rows_only)")["col"]) == 0 and len(fc.build("many_seams(one_entry)")["col"]) == 1
    assert len(fc.build("many_seams(one_row)")["rp"]) == 2 and len(fc.build("many_seams(no_rows)")["rp"]) == 1


@pytest.mark.parametrize("name", fc.NAMES["wrap"])
def test_wrap_cases_reach_block_256(name):
    c = fc.build(name)
    nnz = len(c["col"])
    assert nnz == 257 * 4096 + 1 and (nnz - 1) // fc.BLOCK > 256 and 256 % fc.SLOTS == 0      # block 256 is there, and full
    blocks = sorted(t // fc.BLOCK for t in c["planted"])
    assert blocks == ([0, 256] if "both" in name else [256])
    lens = np.diff(c["rp"])
    assert np.sum(lens == 2) == (0 if "seam" in name else len(blocks)) and np.sum(lens == 1) == len(lens) - np.sum(lens == 2)
    for t in c["planted"]:
        assert _same_row(c, t) == ("seam" not in name)
        assert (c["col"][t] > c["col"][t + 1]) == ("ascending" not in name)
    assert fm.truth(*_host(c))[0]["rows_sorted"] == int("seam" in name or "ascending" in name)


@pytest.mark.parametrize("name", fc.NAMES["value"])
def test_value_cases_change_one_value(name):
    c = fc.build(name)
    t, twin = c["t"], c["twin"]
    bits, tb = c["val"].view(np.uint32), twin["val"].view(np.uint32)
    assert np.all(tb == fm.ONE_BITS) and np.flatnonzero(bits != tb).tolist() == [t] and np.array_equal(c["col"], twin["col"])
    f, l = fm.truth(*_host(c))
    tf, _ = fm.truth(*_host(twin))
    assert f == dict(tf, unit_values=0) and l == fm.no_layout()


def test_value_cases_cover_the_named_entries_and_values():
    nnz = len(fc.clean()["col"])
    assert sorted({fc.build(n)["t"] for n in fc.NAMES["value"]}) == [0, 63, 64, 255, 256, 4095, 4096, nnz - 1]
    b = {k: int(np.float32(v).view(np.uint32)) for k, v in fc.ODD_VALUES.items()}
    assert b["up"] == 0x3F800001 and b["down"] == 0x3F7FFFFF and b["neg"] == 0xBF800000 and b["zero"] == 0 and b["inf"] == 0x7F800000
    assert np.isnan(fc.ODD_VALUES["nan"]) and float(fc.ODD_VALUES["up"]) == 1 + 2.0 ** -23 and float(fc.ODD_VALUES["down"]) == 1 - 2.0 ** -24


def test_length_cases():
    for z in (1, 2, 30, 64, 65):
        f, _ = fm.truth(*_host(fc.build(f"all_rows({z})")))
        assert f["fixed_row_len"] == z == f["max_row_len"] and f["rows_sorted"] == 1
    rows = set()
    for n in fc.NAMES["lengths"]:
        c = fc.build(n)
        f, l = fm.truth(*_host(c))
        if n.startswith("one_row_differs"):
            lens = np.diff(c["rp"])
            assert np.flatnonzero(lens != c["z"]).tolist() == [c["row"]]
            assert f["fixed_row_len"] == 0 and f["max_row_len"] == (c["z"] + 1 if c["how"] == "longer" else c["z"]) and l == fm.no_layout()
            rows.add(c["row"])
        if n.startswith("longest_row"):
            lens = np.diff(c["rp"])
            assert int(np.argmax(lens)) == c["row"] and np.sum(lens == 25) == 1 and f["max_row_len"] == 25
    assert rows == {0, 63, 64, 255, 256, 299}


def test_field_cases_keep_their_promises():
    for n in fc.NAMES["fields"]:
        c = fc.build(n)
        z = int(c["rp"][1])
        nnz = len(c["col"])
        f, l = fm.truth(*_host(c))
        assert f["rows_sorted"] == 1 and f["fixed_row_len"] == z, n
        w = n[len("fields_case("):-1]
        if w.startswith("clean"):
            assert nnz > fc.BLOCK and fc.BLOCK % z != 0 and l["dense_prefix"] == c["d"] and len(l["field_base"]) - 1 == z - c["d"], n
            assert l["field_base"][0] == c["d"] and l["field_base"][-1] == c["p"]
            assert all(a >= b for a, b in zip(l["field_base"][1:-1], c["vocab_base"][1:-1]))      # found bases: the smallest ids that occur
        elif w.startswith("unit_dense"):
            assert f["unit_values"] == 1 and l["dense_prefix"] == 0 and len(l["field_base"]) - 1 == z and l["field_base"][:c["d"]] == list(range(c["d"]))
        elif w == "touch":
            a, b = c["touch"]
            c2 = c["col"].reshape(-1, z)
            assert c2[:, 3 + 6].max() == a and c2[:, 3 + 7].min() == b == a + 1 and l["field_base"][7] == b
        elif w == "meet":
            c2 = c["col"].reshape(-1, z)
            assert c2[:, 3 + 6].max() == c["meet"] == c2[:, 3 + 7].min() and l == fm.no_layout()
            assert int(np.argmax(c2[:, 3 + 6])) != int(np.argmin(c2[:, 3 + 7]))
        elif w.startswith("odd_value"):
            assert c["t"] == (nnz - 1 if w.endswith("last") else fc.BLOCK) and c["t"] % z >= 3 and l == fm.no_layout() and f["unit_values"] == 0
            assert np.flatnonzero(c["val"].reshape(-1, z)[:, 3:].ravel().view(np.uint32) != fm.ONE_BITS).size == 1
        elif w == "last_row_extremes":
            p4, lo4, p9, hi9 = c["extremes"]
            c2 = c["col"].reshape(-1, z)
            assert np.flatnonzero(c2[:, p4] == lo4).tolist() == [len(c2) - 1] == np.flatnonzero(c2[:, p9] == hi9).tolist()
            assert c2[:, p4].min() == lo4 and c2[:, p9].max() == hi9 and l["field_base"][4] == lo4 and l["dense_prefix"] == 3
            assert (nnz - 1) // fc.BLOCK == (nnz - z) // fc.BLOCK and nnz % fc.BLOCK != 0      # the last row lies in the partial last block
        elif w in ("z1", "z2", "z64"):
            assert l["dense_prefix"] == 0 and len(l["field_base"]) - 1 == z
        elif w == "z65":
            assert l == fm.no_layout()
        else:
            raise AssertionError(n)


def test_set_fields_cases_are_violated_by_one_row():
    rows = []
    for n in fc.NAMES["set_fields"]:
        c = fc.build(n)
        f, l = fm.truth(*_host(c))
        assert l["dense_prefix"] == 1 and len(l["field_base"]) == 5 and l["field_base"][2] == c["lowest"]
        assert fm.sound(f, l, *_host(c)) == []
        assert fm.sound(f, dict(l, field_base=c["vocab_base"]), *_host(c)) == []            # the vocabularies' bases are wider and hold every row
        assert c["vocab_base"] != l["field_base"]
        bad = list(l["field_base"]); bad[2] += 1
        assert fm.sound(f, dict(l, field_base=bad), *_host(c)) == ["a field id lies outside its range"]
        c2 = c["col"].reshape(-1, 5)
        assert np.flatnonzero(c2[:, 3] < bad[2]).tolist() == [c["row"]]
        rows.append(c["row"])
    assert rows == [0, 255, 256, 299]


def test_all_twos_normalize_to_exactly_one():
    for kind in ("fields", "ragged"):
        c = fc.all_twos(kind)
        p = c["p"]
        f, l = fm.truth(*_host(c))
        assert f["unit_values"] == 0 and l == fm.no_layout()
        out = fc.normalized(c["val"], c["col"], np.zeros(p), np.full(p, 2.0))
        assert np.all(out.view(np.uint32) == fm.ONE_BITS)
        f1, l1 = fm.truth(c["rp"], c["col"], out, p)
        assert f1["unit_values"] == 1 and bool(l1["field_base"]) == (kind == "fields")


def test_sound_notices_every_false_claim():
    c = fc.build("in_row(63,descent)")
    f, l = fm.truth(*_host(c))
    assert fm.sound(dict(f, rows_sorted=1), l, *_host(c)) != []
    assert fm.sound(dict(f, max_row_len=f["max_row_len"] - 1), l, *_host(c)) != [] and fm.sound(dict(f, max_row_len=64), l, *_host(c)) == []
    assert fm.sound(dict(f, fixed_row_len=3), l, *_host(c)) != []
    v = fc.build("odd_value(64,up)")
    fv, lv = fm.truth(*_host(v))
    assert fm.sound(dict(fv, unit_values=1), lv, *_host(v)) != [] and fm.sound(dict(fv, rows_sorted=0), lv, *_host(v)) == []
    m = fc.build("fields_case(meet)")
    fmm, _ = fm.truth(*_host(m))
    assert fm.sound(fmm, dict(dense_prefix=3, field_base=m["vocab_base"]), *_host(m)) != []
    o = fc.build("fields_case(odd_value_4096)")
    fo, _ = fm.truth(*_host(o))
    assert fm.sound(fo, dict(dense_prefix=3, field_base=o["vocab_base"]), *_host(o)) == ["a field entry's value is not 1.0f"]
