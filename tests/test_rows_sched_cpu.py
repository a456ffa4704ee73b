"""The invariants of phase 1's plan-time schedule, on its definition (tests/rows_sched_model.py) and on the grid of shapes the GPU test runs
(tests/rows_sched_cases.py): every entry exactly once and in its row's stored order, nothing taken above the front, the bound on a block's steps, MERGE
equal to a plain 4-way merge, ROUND serving slot t mod 4 only -- for every tail block of every case under every policy of the
model (MERGE is the one the device builds; FRONT and ROUND exist in the model only), and for one block of the head tile."""
import numpy as np
import pytest

from tests import rows_sched_model as M
from tests.rows_sched_cases import ALL_TAILS, CASES, HEAD, P, POLICIES, problem, seed_of, tail_lengths

GRID = [(ci, t) for ci, c in enumerate(CASES) for t in c["tails"]]


@pytest.fixture(scope="module")
def problems():
    return {(ci, t): problem(CASES[ci], t, seed_of(ci, t)) for ci, t in GRID}


def test_the_cases_are_what_they_claim(problems):
    assert CASES[0]["tails"] == ALL_TAILS and set(tail_lengths("mixed", 256)) == {0, 1, 30, 36}
    for (ci, t), (rp, col, _, _) in problems.items():
        assert col.max() < P <= M.MAX_P and len(rp) == HEAD + t + 1
    rp, col, _, _ = problems[(4, 257)]
    rows = [col[rp[HEAD + r]:rp[HEAD + r + 1]] for r in range(257)]
    assert any(np.any(np.diff(r.astype(np.int64)) < 0) for r in rows) and any(len(set(r.tolist())) < len(r) for r in rows)
    rows = M.block_rows(*problems[(5, 256)][:2], HEAD, 256, 0)
    per_group = [sum(len(rows[s][g]) for s in range(4)) for g in range(64)]
    assert per_group[5] == 4 * per_group[0] == 128


@pytest.mark.parametrize("pol", POLICIES, ids=[p[0] for p in POLICIES])
@pytest.mark.parametrize("ci,t", GRID, ids=[f"{CASES[ci]['name']}_{t}" for ci, t in GRID])
def test_invariants_of_every_tail_block(problems, ci, t, pol):
    rp, col, _, _ = problems[(ci, t)]
    _, policy, rho_q = pol
    for b in range((t + 255) // 256):
        rows = M.block_rows(rp, col, HEAD, t, b)
        sched = M.block_schedule(rp, col, HEAD, t, b, P, policy, rho_q)
        assert sched.dtype == np.uint32 and sched.shape[1] == 64
        M.check_block(sched, rows, policy, rho_q, P)
        if CASES[ci]["tail"] == "over37" and b == 0:
            assert sched.shape[0] > M.STAGE_STEPS
        if CASES[ci]["tail"] == "full36" and policy == M.MERGE and (b + 1) * 256 <= t:
            assert sched.shape[0] == M.STAGE_STEPS          # the stage exactly


@pytest.mark.parametrize("pol", POLICIES, ids=[p[0] for p in POLICIES])
def test_invariants_of_a_head_block(problems, pol):
    rp, col, _, _ = problems[(0, 1)]
    _, policy, rho_q = pol
    sched = M.block_schedule(rp, col, 0, HEAD, 3, P, policy, rho_q)
    M.check_block(sched, M.block_rows(rp, col, 0, HEAD, 3), policy, rho_q, P)
    if policy == M.MERGE:
        assert sched.shape[0] == 120 and not np.any(sched == M.BUBBLE)


def test_front_formula():
    assert M.ramp_steps(120, 0) == 0 and M.front(0, P, 0) == M.ALL
    assert M.ramp_steps(120, 1024) == 120 and M.ramp_steps(120, 922) == 134 and M.ramp_steps(0, 922) == 0
    r = M.ramp_steps(120, 922)
    f = [M.front(t, P, r) for t in range(r + 2)]
    assert f[0] == P // r and all(a <= b for a, b in zip(f, f[1:])) and f[r - 2] < P and f[r - 1] == M.ALL and f[r] == M.ALL
    big = M.front(10 ** 6, M.MAX_P, 2 * 10 ** 6)      # no 32-bit wrap in (t + 1) p
    assert big == (10 ** 6 + 1) * M.MAX_P // (2 * 10 ** 6)
