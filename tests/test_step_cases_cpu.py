"""CPU self-checks of tests/step_cases.py: the hand-made matrices of tests/test_gpu_step_forms.py have the lists they claim to have, the case
selection covers what it says, and the oracle side runs without a GPU."""
import numpy as np
import pytest

import oracle
from tests import step_cases as sc


@pytest.mark.parametrize("values", [False, True], ids=["onehot", "val"])
@pytest.mark.parametrize("regime", list(sc.REGIMES))
def test_ladder_lists_have_their_lengths_and_the_truncated_step_its_ghosts(regime, values):
    prob = sc.ladder_problem(regime, values, 7)
    p, rp, col, val = prob["p"], prob["rp"], prob["col"], prob["val"]
    assert len(rp) == 3 * sc.STEP + 1 and rp[-1] == len(col) == len(val)
    row_of = np.repeat(np.arange(prob["n"]), np.diff(rp))
    assert np.all((np.diff(col.astype(np.int64)) > 0) | (np.diff(row_of) > 0)), "columns ascend inside every row"
    assert np.all(val == 1.0) != values
    ids, virgin = sc.ladder_ids(p)
    cut = 0
    for s in range(3):
        feat, cnt = sc.step_lists(prob, s)
        length = dict(zip(feat.tolist(), cnt.tolist()))
        assert [length[int(j)] for j in ids] == list(sc.LADDER), s   # exactly L entries in step 0 (and in the two others)
        assert (virgin in length) == (s == 2)
        entries = int(rp[(s + 1) * sc.STEP] - rp[s * sc.STEP])
        lists = len(feat)
        if regime == "dense":
            assert entries >= p
        elif regime == "inline":
            assert entries < p and 2 * lists <= entries < 16 * lists
        else:
            assert entries < p and entries < 2 * lists
        assert cnt.max() >= sc.LADDER[-1] and np.sum(cnt > sc.LONG_MIN) >= 4   # 65, 1023.. and 2049 are long lists in every regime
    # the truncated third step: rows [2 STEP, 2 STEP + LIMIT) are active
    third = (row_of >= 2 * sc.STEP)
    active = third & (row_of < 2 * sc.STEP + sc.LIMIT)
    for j, length in zip(ids, sc.LADDER):
        a, t = int(np.sum(active & (col == j))), int(np.sum(third & (col == j)))
        assert t == length
        if length in sc.GHOSTS:
            assert a == 0 and int(j) in prob["ghosts"]
        cut += 0 < a < t
    assert cut >= 8, "rows_limit must cut through the middle of several ladder lists"
    assert np.sum(third & (col == virgin)) == 2 and np.sum(active & (col == virgin)) == 0 and np.sum(col == virgin) == 2
    assert prob["oracle_steps"][-1] == (2 * sc.STEP, 2 * sc.STEP + sc.LIMIT) and prob["engine_steps"][-1] == (2, sc.LIMIT)


def test_ladder_selection_covers_every_k_with_every_solver_value_kind_and_directory():
    cases = sc.LADDER_CASES
    assert 30 <= len(cases) <= 40 and len({c["name"] for c in cases}) == len(cases)
    assert len({(c["k"], c["solver"], c["regime"], c["values"]) for c in cases}) == len(cases)
    for k in (16, 12, 6, 8, 32):
        mine = [c for c in cases if c["k"] == k]
        assert {c["solver"] for c in mine} == set(sc.SOLVERS)
        assert {c["values"] for c in mine} == {False, True}
        assert {c["regime"] for c in mine} == set(sc.REGIMES)


def test_side_stream_tile_carries_enough_long_list_segments():
    prob = sc.side_problem(True, 900)
    for s in range(2):
        feat, cnt = sc.step_lists(prob, s)
        long_lists = cnt[cnt > sc.LONG_MIN]
        assert np.all(long_lists <= 1024)                                   # one segment each
        assert len(long_lists) >= sc.SIDE_MIN_SEG + 64, len(long_lists)     # the side stream's threshold, with room
        entries = int(cnt.sum())
        assert entries < prob["p"] and 2 * len(feat) <= entries < 16 * len(feat)   # a sparse tile in the list-by-list form


def test_schedule_is_the_wrap_around_one():
    assert sc.schedule(sc.N, sc.BATCH, sc.TOTAL) == [(0, 2048), (2048, 4096), (0, 2048), (2048, 2053)]
    steps = sc.schedule(1200, 257, 1805)   # a last batch shorter than the others, then the wrap
    assert steps[4] == (1028, 1200) and steps[5] == (0, 257) and sum(b - a for a, b in steps) == 1805


@pytest.mark.parametrize("solver", sc.SOLVERS)
def test_oracle_leaves_the_ghost_features_alone_in_the_truncated_step(solver):
    """The oracle side of a ladder case end to end (no GPU): the features whose third-step entries are all inactive keep parameters and optimizer
    state through that step, the never-active feature keeps its start values, everything else that occurs moves."""
    case = dict(name="cpu", part="B", k=6, solver=solver, regime="dense", values=True, seed=3)
    prob = sc.ladder_problem("dense", True, 3)
    w0, w, v = sc.start_params(prob["p"], 6, 3)
    ref = sc.oracle_run(case, prob["rp"], prob["col"], prob["val"], prob["y"], prob["p"], w0, w, v, prob["oracle_steps"], prob["ghosts"])
    assert ref["ghost_still"]
    virgin = prob["virgin"]
    assert np.array_equal(ref["v"][:, virgin], v[:, virgin]) and ref["w"][virgin] == w[virgin]
    ids = prob["ids"]
    assert np.all(np.any(ref["v"][:, ids] != v[:, ids], axis=0))
    assert np.isfinite(ref["v"]).all() and np.isfinite(ref["w"]).all()
    assert oracle.CLASSIFICATION == sc.oracle_params(case).task
