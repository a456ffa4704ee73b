"""Phase 1's plan-time schedule, in numpy: THE DEFINITION (the device builder is rows_sched_k, fm_ingest.hip; the kernel that walks it fm_rows_sched_k,
fm_batch_kernels.hip).

A tile's rows are cut into blocks of 256.  Lane group g (0..63) of block b owns the rows 64 s + g of the block, slots s = 0..3, and walks their entries as
one stream.  The block's schedule is T_b steps of 64 words, step-major: word g of step t names what lane group g takes at step t -- `col | slot << 30` -- or
is a bubble, 0xFFFFFFFF.  Every row's entries appear exactly once and in the row's stored order, whatever that order is.

  MERGE       the lane group takes the smallest head column of its four rows, ties to the lowest slot (a 4-way merge of the heads); no bubbles before its end
  FRONT(rho)  the same choice, taken only if that column is at most front(t), else a bubble
  ROUND(rho)  step t serves slot t mod 4 only: the head of that row if it has one and its column is at most front(t), else a bubble

front(t) = floor((t + 1) p / R) while t + 1 < R, and everything from then on; R = ceil(1024 E_b / rho_q) steps, E_b the most entries any lane group of the
block holds, rho_q = rho in 1024ths (an integer, 1..1024); rho_q = 0 means no front at all.  T_b is one past the last step at which any lane group takes an
entry, rounded up to a multiple of four under ROUND; shorter lane groups end in bubbles.

The device builds and walks MERGE (and DEAL, tests/rows_deal_model.py, which is this MERGE walk on rows dealt to other places of the block).  FRONT and ROUND
have no device form: they are defined here and checked on the CPU only (tests/test_rows_sched_cpu.py)."""
import numpy as np

MERGE, FRONT, ROUND = 0, 1, 2
BUBBLE = 0xFFFFFFFF
NG, SLOTS, RPW = 64, 4, 256
STAGE_STEPS = 144            # steps a workgroup of the kernel stages (36 KiB)
MAX_P = (1 << 30) - 1
ALL = 0xFFFFFFFF


def ramp_steps(e_b, rho_q):
    return 0 if rho_q == 0 else (int(e_b) * 1024 + rho_q - 1) // rho_q


def front(t, p, ramp):
    return ALL if ramp == 0 or t + 1 >= ramp else ((t + 1) * int(p)) // ramp


def block_rows(rp, col, r0, nrows, b):
    """rows[s][g]: the column ids of row 64 s + g of block b of rows [r0, r0 + nrows), as Python ints (a row beyond the range is empty)"""
    rows = [[[] for _ in range(NG)] for _ in range(SLOTS)]
    for s in range(SLOTS):
        for g in range(NG):
            r = b * RPW + s * NG + g
            if r < nrows:
                rows[s][g] = [int(c) for c in col[rp[r0 + r]:rp[r0 + r + 1]]]
    return rows


def lane_group_words(lists, policy, ramp, p):
    """the words of one lane group up to its last entry"""
    pos = [0] * SLOTS
    left = sum(len(x) for x in lists)
    out = []
    t = 0
    while left > 0:
        f = front(t, p, ramp)
        if policy == ROUND:
            s = t % SLOTS
            sel = s if pos[s] < len(lists[s]) else -1
        else:
            sel = -1
            for s in range(SLOTS):
                if pos[s] < len(lists[s]) and (sel < 0 or lists[s][pos[s]] < lists[sel][pos[sel]]):
                    sel = s
        if sel >= 0 and lists[sel][pos[sel]] <= f:
            out.append(lists[sel][pos[sel]] | (sel << 30))
            pos[sel] += 1
            left -= 1
        else:
            out.append(BUBBLE)
        t += 1
    return out


def block_schedule(rp, col, r0, nrows, b, p, policy, rho_q):
    """uint32 [T_b, 64]"""
    if policy == MERGE:
        rho_q = 0
    rows = block_rows(rp, col, r0, nrows, b)
    e_b = max(sum(len(rows[s][g]) for s in range(SLOTS)) for g in range(NG))
    ramp = ramp_steps(e_b, rho_q)
    words = [lane_group_words([rows[s][g] for s in range(SLOTS)], policy, ramp, p) for g in range(NG)]
    steps = max(len(w) for w in words)
    if policy == ROUND:
        steps = (steps + 3) // 4 * 4
    out = np.full((steps, NG), BUBBLE, np.uint32)
    for g, w in enumerate(words):
        out[:len(w), g] = w
    return out


def steps_bound(rows, policy, rho_q):
    """what T_b cannot exceed: the ramp, then one entry per step and lane group (MERGE, FRONT) or one per four steps and row (ROUND)"""
    e_b = max(sum(len(rows[s][g]) for s in range(SLOTS)) for g in range(NG))
    longest = max(len(rows[s][g]) for s in range(SLOTS) for g in range(NG))
    if policy == MERGE:
        return e_b
    ramp = ramp_steps(e_b, rho_q)
    return max(ramp - 1, 0) + e_b if policy == FRONT else (max(ramp - 1, 0) + 4 * longest + 3) // 4 * 4


def plain_merge(lists):
    """a 4-way merge of the heads, smallest first, ties to the lowest slot: (col, slot) pairs"""
    pos = [0] * SLOTS
    out = []
    while True:
        live = [s for s in range(SLOTS) if pos[s] < len(lists[s])]
        if not live:
            return out
        s = min(live, key=lambda j: (lists[j][pos[j]], j))
        out.append((lists[s][pos[s]], s))
        pos[s] += 1


def check_block(sched, rows, policy, rho_q, p):
    """the invariants of one block's schedule; raises AssertionError"""
    if policy == MERGE:
        rho_q = 0
    steps = sched.shape[0]
    e_b = max(sum(len(rows[s][g]) for s in range(SLOTS)) for g in range(NG))
    ramp = ramp_steps(e_b, rho_q)
    assert steps <= steps_bound(rows, policy, rho_q), (steps, steps_bound(rows, policy, rho_q))
    any_last = False
    for g in range(NG):
        seen = [[] for _ in range(SLOTS)]
        for t in range(steps):
            w = int(sched[t, g])
            if w == BUBBLE:
                continue
            c, s = w & MAX_P, w >> 30
            seen[s].append(c)
            assert c <= front(t, p, ramp), (g, t, c)                      # nothing taken above the front
            assert policy != ROUND or s == t % SLOTS, (g, t, s)
        for s in range(SLOTS):
            assert seen[s] == rows[s][g], (g, s)                            # every entry once, row order kept
        if steps and (int(sched[steps - 1, g]) != BUBBLE or (policy == ROUND and any(int(x) != BUBBLE for x in sched[steps - 4:, g]))):
            any_last = True
        if policy == MERGE:
            lists = [rows[s][g] for s in range(SLOTS)]
            want = [c | (s << 30) for c, s in plain_merge(lists)]
            assert [int(x) for x in sched[:len(want), g]] == want and all(int(x) == BUBBLE for x in sched[len(want):, g]), g
    assert steps == 0 or any_last                                           # no trailing step (round of four) of bubbles alone
