"""Phase 1's DEAL schedule, in numpy and Python integers: THE DEFINITION (the device builder is rows_sched_k<WRITE, true>, fm_ingest.hip; the kernel that
walks it fm_rows_sched_k<DEAL = true>, fm_batch_kernels.hip).

DEAL is the MERGE walk (tests/rows_sched_model.py) on rows that a plan-time rule has dealt to (slot, lane group) places inside each 256-row block: MERGE
gives lane group g the rows 64 s + g of the block; DEAL gives it the rows m[s][g], chosen so that every lane group's merged stream stays close to an even
ramp over the columns.  Nothing in the results depends on which lane group walks a row: a row's sums are its own.

Block b's rows are i = 0..255 (a row past the range is empty), n_i their entries, N_b the block's entries.  Cuts q_k = floor(k p / 16), k = 1..15;
c_i[k] = the row's stored entries with column < q_k (whatever their order), c_i[16] = n_i; a_i[k] = 4096 c_i[k] - k N_b, k = 1..16 -- 4096 times the row's
excess over its 1/256 share of an even ramp; key_i = max_k |a_i[k]|.

The rows are visited by descending key, ties to the lower i.  Per lane group A_g[k] = 0 and cnt_g = 0.  The j-th visited row (j = 0..255) goes to level
j // 64; the candidates are the lane groups with cnt_g == level; it takes the g that minimises max_k |A_g[k] + a_i[k]|, ties to the lowest g, and becomes
that lane group's slot `level`: m[level][g] = i, A_g += a_i, cnt_g += 1.  m is a permutation of 0..255.

A DEAL block's schedule is 64 header words -- word g = m[0][g] | m[1][g] << 8 | m[2][g] << 16 | m[3][g] << 24 -- followed by T_b steps of 64 words:
lane group g's words are MERGE's over the lists [row m[s][g] for s in 0..3], ties to the lowest slot; T_b is the largest lane group total."""
import numpy as np

from tests.rows_sched_model import BUBBLE, MERGE, NG, RPW, SLOTS, lane_group_words

DEAL = 3
CUTS = 16
SCALE = 4096


def block_lists(rp, col, r0, nrows, b):
    """the column ids of rows 0..255 of block b of rows [r0, r0 + nrows), as lists of Python ints (a row beyond the range is empty)"""
    out = []
    for i in range(RPW):
        r = b * RPW + i
        out.append([int(c) for c in col[rp[r0 + r]:rp[r0 + r + 1]]] if r < nrows else [])
    return out


def excess(lists, p):
    """a[i][k - 1] = 4096 c_i[k] - k N_b, k = 1..16, as Python ints"""
    n_b = sum(len(x) for x in lists)
    cuts = [(k * int(p)) // CUTS for k in range(1, CUTS)]
    a = []
    for x in lists:
        c = [sum(1 for v in x if v < q) for q in cuts] + [len(x)]
        a.append([SCALE * c[k - 1] - k * n_b for k in range(1, CUTS + 1)])
    return a


def deal_map(lists, p):
    """m[s][g]: the row of the block that lane group g walks as its slot s"""
    a = np.array(excess(lists, p), np.int64)          # exact: every value is far below 2^63
    key = np.abs(a).max(axis=1)
    order = sorted(range(RPW), key=lambda i: (-int(key[i]), i))
    acc = np.zeros((NG, CUTS), np.int64)
    cnt = np.zeros(NG, np.int64)
    m = [[-1] * NG for _ in range(SLOTS)]
    for j, i in enumerate(order):
        level = j // NG
        cost = np.abs(acc + a[i]).max(axis=1)
        cost[cnt != level] = np.iinfo(np.int64).max
        g = int(np.argmin(cost))                      # the first of the smallest: ties to the lowest g
        m[level][g] = i
        acc[g] += a[i]
        cnt[g] += 1
    return m


def header(m):
    return np.array([m[0][g] | m[1][g] << 8 | m[2][g] << 16 | m[3][g] << 24 for g in range(NG)], np.uint32)


def block_schedule_lists(lists, p):
    """(header uint32 [64], words uint32 [T_b, 64], the map) of a block given as its 256 lists"""
    m = deal_map(lists, p)
    words = [lane_group_words([lists[m[s][g]] for s in range(SLOTS)], MERGE, 0, p) for g in range(NG)]
    steps = max(len(w) for w in words)
    out = np.full((steps, NG), BUBBLE, np.uint32)
    for g, w in enumerate(words):
        out[:len(w), g] = w
    return header(m), out, m


def block_schedule(rp, col, r0, nrows, b, p):
    return block_schedule_lists(block_lists(rp, col, r0, nrows, b), p)


def identity_map():
    return [[s * NG + g for g in range(NG)] for s in range(SLOTS)]


def largest_excursion(lists, m, p):
    """the mean over the lane groups that hold entries of the largest distance, as a fraction of p, between a lane group's merged stream and the even ramp
    from 0 to p over its own steps: max_t |col_t - (t + 1/2) p / n| / p"""
    worst = []
    for g in range(NG):
        cols = sorted(c for s in range(SLOTS) for c in lists[m[s][g]])
        n = len(cols)
        if n:
            worst.append(max(abs(c - (t + 0.5) * p / n) for t, c in enumerate(cols)) / p)
    return float(np.mean(worst)) if worst else 0.0
