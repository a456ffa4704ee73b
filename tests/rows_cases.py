"""Cases, matrix builder, the fp64 reference and the child process shared by tests/test_gpu_rows_forms.py and tests/test_rows_cases_cpu.py.

The mini-batch step's FIRST half (fm_rows_forward_k / _dyn_k / _flat_k, fm_batch_kernels.hip) leaves per row the factor sums and the gradient
multiplier, per workgroup the w0 partial sums.  What it computed is observable without any update: fmx_grad publishes the per-feature gradient sums
GV[F][kp] | GW[F] | CNT[F] (| QV | QW) and the tail {sum M, sum M^2, rows / 4096, rows % 4096} in the exchange buffer, and oracle.batch_sums computes
exactly those in fp64.  A child holds every ELEMENT of that buffer to the reference at the parameters the engine holds, relative to the element's
own un-cancelled absolute sum, for every form of phase 1 the launcher can select -- and reports which form ran (fmx_debug_rows_launches).

Everything above `child_main` runs without a GPU: the launcher's rule restated (`static_form`), the case table with the form every step of every
case must take, the hand-shaped matrices and `sums_reference`, the vectorised restatement of fmo_batch_sums.  `child_main` is what a fresh child
process executes per set of process-wide switches: `python -m tests.rows_cases <job.json>`.  A child asserts nothing about the numerics; it
writes one figure per quantity and the parent's tests hold them to their bars."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEARN_RATE, L2 = 0.05, 1e-3
MIN_P = 6000                     # the longest row holds 5 000 distinct columns
NARROW_CHUNK, WIDE_CHUNK = 512, 2048   # entries a workgroup stages at a time: one-wave workgroups, 256-thread workgroups (STAGE_ENTRIES)
LONG_ROW = 5000
LATE_ROWS = 8                    # the last rows of every step: the only rows that hold the `late` features, and inactive in every truncated step
TAIL_ROWS = 37                   # every step's row count is a multiple of 64 plus this: the last workgroup of every form is partly filled

# the counter's slots (fmx_test_hooks.h: fmx_debug_rows_launches)
NARROW4, NARROW1, WIDE_SERIAL, WIDE_PIPELINED, PULL, FLAT = range(6)
FORM_NAMES = ("narrow4", "narrow1", "wide_serial", "wide_pipelined", "pull", "flat")

# name -> environment of the child (switches read once per process)
CHILDREN = [("default", {}),
            ("serial", {"FMX_ROWS_SERIAL": "1"}),
            ("pipelined", {"FMX_ROWS_SERIAL": "0"}),
            ("side_table", {"FMX_EMBED_MULT": "0"}),        # the multiplier in the side table only: S rows keep all their bits
            ("embed_wide", {"FMX_EMBED_MAX_KP": "64"})]     # the 1-bit embedding at kp = 32 and 64, the padding slot at k = 24 and 48


# --------------------------------------------------------------------------------------------------------------------- the launcher's rule, restated
def padded(k, fp64):
    kp = 2 if fp64 else 4
    while kp < k:
        kp *= 2
    return kp


def lanes(k, fp64):
    """lanes per row: 16 bytes of the padded row each (mb_lpr)"""
    return padded(k, fp64) // (2 if fp64 else 4)


def static_form(rows, lpr):
    """rows_wg_threads / rows_split / launch_rows_w on a pointwise step of `rows` rows: NARROW4, NARROW1 or "wide"."""
    if rows * lpr >= 512 * 256:
        return "wide"
    return NARROW4 if (lpr <= 16 and rows * lpr < 1024 * 64) else NARROW1


def expected_form(rows, lpr, child, variant="plain"):
    """The counter slot a step of `rows` rows must land in, in child `child`, with FMX_ROWS_PULL (variant "pull") or FMX_ROWS_FLAT ("flat") set.
    The two opt-in kernels exist for wide launches only; below 65 536 rows an engine that is not pinned never measures and stays serial."""
    f = static_form(rows, lpr)
    if f != "wide":
        return f
    if variant == "pull":
        return PULL
    if variant == "flat":
        return FLAT
    assert child in ("serial", "pipelined") or rows < 65536, "an unpinned step this large would be timed: its schedule is not predictable"
    return WIDE_PIPELINED if child == "pipelined" else WIDE_SERIAL


def embed_mode(k, fp64, child):
    """fm_batch_kernels.hip: embed_mode -- "none", "pad" or "bits"."""
    kp = padded(k, fp64)
    if fp64 or child == "side_table" or kp > (64 if child == "embed_wide" else 16):
        return "none"
    return "pad" if k < kp else ("bits" if kp >= 16 else "none")


# --------------------------------------------------------------------------------------------------------------------- cases
def _case(name, k, fp64, rows, values, children=("default",), **opts):
    limit = opts.pop("limit", None)
    if limit is None:
        # the truncated third step: about 5/8 of a step, an odd count (the last workgroup of every form with more than one row per workgroup is
        # partly filled) -- except that a wide step stays wide where it can: 21 rows above the threshold (the issue's wide steps sit just above it)
        lpr = lanes(k, fp64)
        edge = -(-512 * 256 // lpr) + 21
        limit = edge if static_form(rows, lpr) == "wide" and edge < rows else (rows * 5 // 8) | 1
    assert limit <= rows - LATE_ROWS
    c = dict(name=name, k=k, fp64=bool(fp64), rows=rows, values=bool(values), children=list(children), limit=limit, task="classification", keep_w0=1, keep_w1=1,
             solver="sgd", w_in_row=0, tile_rows=0, chunks=1, p=MIN_P + 257)
    c.update(opts)
    return c


def _both(name, k, fp64, rows, children=("default",), **opts):
    return [_case(f"{name}_{'val' if v else 'onehot'}", k, fp64, rows, v, children, **opts) for v in (True, False)]


def _cases():
    out = []
    small = 960 + TAIL_ROWS
    # narrow4: steps of about 1 000 rows; fp32 k spans EMBED_PAD (3, 6, 12), none (8; 32 and 64 by default) and EMBED_BITS (16) and lanes 1 .. 16
    for k in (3, 6, 8, 12, 16, 32, 64):
        ch = ["default"] + (["side_table"] if k in (12, 16) else []) + (["embed_wide"] if k in (32, 64) else [])
        out += _both(f"narrow4_f32_k{k}", k, False, small, ch)
    for k in (24, 48):   # EMBED_PAD on rows of 128 and 256 bytes
        out += _both(f"narrow4_f32_k{k}", k, False, small, ["embed_wide"])
    for k in (2, 16, 32):
        out += _both(f"narrow4_f64_k{k}", k, True, small)
    # narrow1 by width: more than 16 lanes per row
    # (the engine takes at most 128 factors: fp32 rows reach 32 lanes, fp64 rows 64 -- the 64-lane fp32 instances are compiled and unreachable)
    for k, fp64 in ((64, True), (128, True), (128, False)):
        out += _both(f"narrow1_{'f64' if fp64 else 'f32'}_k{k}", k, fp64, small)
    # narrow1 by size
    out += _both("narrow1_f32_k16_16k", 16, False, 16384 + TAIL_ROWS, ["default", "side_table"])
    # 64 rows per workgroup: ordinary rows cross the 512-entry chunk.  The truncated step drops below 65 536 rows x lanes: narrow4
    out += _both("narrow1_f32_k3_64k", 3, False, 65536 + TAIL_ROWS, limit=40961)
    # wide (256 threads): the headline instance first
    wide_ch = ["default", "serial", "pipelined"]
    out += _both("wide_f32_k16", 16, False, 32768 + TAIL_ROWS, wide_ch + ["side_table"])
    out += _both("wide_f32_k64", 64, False, 8192 + TAIL_ROWS, wide_ch + ["embed_wide"])
    out += _both("wide_f32_k48", 48, False, 8192 + TAIL_ROWS, ["embed_wide"])
    out += _both("wide_f64_k16", 16, True, 16384 + TAIL_ROWS, wide_ch)
    out += _both("wide_f64_k64", 64, True, 4096 + TAIL_ROWS, wide_ch)
    out += _both("wide_f64_k128", 128, True, 2048 + TAIL_ROWS, wide_ch)
    # wide with one and two lanes per row: steps of more than 65 536 rows, so only where the schedule is pinned
    out += _both("wide_f32_k3", 3, False, 131072 + TAIL_ROWS, ["serial", "pipelined"])
    out += _both("wide_f32_k6", 6, False, 65536 + TAIL_ROWS, ["serial", "pipelined"])
    # the (element type, lanes per row) instances of the three static forms that the cases above leave out
    for k in (4, 8):                                                 # narrow4, fp64, 2 and 4 lanes
        out += _both(f"narrow4_f64_k{k}", k, True, small)
    for k, fp64, rows in ((6, False, 32768), (32, False, 8192), (64, False, 4096),                       # narrow1 by size, fp32, 2 / 8 / 16 lanes
                          (2, True, 65536), (4, True, 32768), (8, True, 16384), (16, True, 8192), (32, True, 4096)):   # fp64, 1 .. 16 lanes
        out += _both(f"narrow1_{'f64' if fp64 else 'f32'}_k{k}_{rows // 1024}k", k, fp64, rows + TAIL_ROWS)
    for k, fp64, rows in ((32, False, 16384), (128, False, 4096), (8, True, 32768), (32, True, 8192)):   # wide: fp32 8 / 32 lanes, fp64 4 / 16
        out += _both(f"wide_{'f64' if fp64 else 'f32'}_k{k}", k, fp64, rows + TAIL_ROWS, wide_ch)
    out += _both("wide_f64_k2", 2, True, 131072 + TAIL_ROWS, ["serial", "pipelined"])   # one and two lanes: pinned children only
    out += _both("wide_f64_k4", 4, True, 65536 + TAIL_ROWS, ["serial", "pipelined"])
    # the k = 16 instance of each form under the other things phase 1 reads: table layout, task and clamps, w0 / w switched off, the Q planes.
    # One value kind each, rotating, so that every option meets both kinds and every form meets both.
    extras = [("wir", dict(w_in_row=1)), ("regr", dict(task="regression")), ("now0", dict(keep_w0=0)), ("now1", dict(keep_w1=0)), ("ftrlsum", dict(solver="ftrl_sum"))]
    for a, (form, rows) in enumerate((("narrow4", small), ("narrow1", 16384 + TAIL_ROWS), ("wide", 32768 + TAIL_ROWS))):
        for b, (tag, opts) in enumerate(extras):
            v = (a + b) % 2 == 0
            out.append(_case(f"{form}_f32_k16_{tag}_{'val' if v else 'onehot'}", 16, False, rows, v, **opts))
    out.append(_case("wide_f64_k16_ftrlsum_val", 16, True, 16384 + TAIL_ROWS, True, solver="ftrl_sum"))
    # a wide step cut into three tiles with a ragged last one: the form follows the STEP's row count, the w0 partial sums are offset per tile
    # (32 806 rows: tiles of 10 936, 10 936 and 10 934 rows -- the engine evens the tiles out -- and 10 917 in the truncated step)
    out.append(_case("wide_f32_k16_tiles_val", 16, False, 32768 + TAIL_ROWS + 1, True, tile_rows=12000))
    # the chunked exchange: phase 1 of the whole step, then phase 2 block by block (three blocks of features)
    out.append(_case("wide_f32_k16_chunks_onehot", 16, False, 32768 + TAIL_ROWS, False, chunks=3))
    out.append(_case("narrow4_f32_k12_chunks_val", 12, False, small, True, chunks=3, solver="ftrl_sum"))
    assert len({c["name"] for c in out}) == len(out)
    return out


CASES = _cases()
# compact records: one sparse tile per step (p much larger than the step's entries), fp32 and fp64 tables
COMPACT_CASES = [_case(f"compact_{'f64' if w else 'f32'}_k{k}_{s}", k, w, 960 + TAIL_ROWS, v, p=400000, solver=s, compact=1)
                 for k, w, v, s in ((16, False, True, "sgd"), (12, False, False, "ftrl_sum"), (16, True, True, "ftrl_sum"), (6, True, False, "sgd"))]


def cases_of(child):
    return [c for c in CASES + COMPACT_CASES if child in c["children"]]


def case_steps(case):
    """(batch, rows_limit, active rows) of the case's three steps: batch 0 and batch 1 in full, batch 2 truncated."""
    return [(0, 0, case["rows"]), (1, 0, case["rows"]), (2, case["limit"], case["limit"])]


def variants_of(case, rows):
    """The forms a step of `rows` rows is run through inside one child: the opt-in kernels only where the step is wide (and the exchange plain)."""
    wide = static_form(rows, lanes(case["k"], case["fp64"])) == "wide"
    if wide and case["chunks"] == 1 and not case.get("compact"):
        return ["pull", "flat", "plain"]   # plain last: its buffer is the one the update between the steps applies
    return ["plain"]


# --------------------------------------------------------------------------------------------------------------------- matrices
def _special_rows(rows):
    """(row index inside a step, entries) of the hand-placed rows.  Indices are relative to the step's first row; 0 mod 256 is the first row of a
    workgroup in every form (a workgroup holds 1 .. 256 rows, a power of two)."""
    base = [(0, 508), (1, 8),              # an 8-entry row over the 512-entry boundary of a one-wave workgroup of two or more rows
            (385, NARROW_CHUNK),           # exactly one narrow chunk, behind an ordinary row: it straddles wherever it shares a workgroup
            (512, WIDE_CHUNK),             # exactly one wide chunk from the workgroup's first entry: the next row starts a chunk
            (256, 2044), (257, 8),         # an 8-entry row over the 2 048-entry boundary of a wide workgroup (and over 4 x 512)
            (259, LONG_ROW)]               # ten narrow chunks, two and a half wide ones; the rows behind it start inside a later chunk
    assert rows * 5 // 8 > 513
    return base


def quiet_features(p):
    """(ghost, late): features that occur in no row at all, and features that occur only in the last LATE_ROWS rows of every step -- part of the
    step's lists, and without an active row once rows_limit cuts the step.  Both spread over the whole feature range."""
    ghost = np.arange(40, p, 97, dtype=np.int64)
    return ghost, ghost + 1


def problem(rows, p, values, seed):
    """Three steps of `rows` rows: Poisson(12) rows with empty and single-entry rows (the recipe of util.random_csr, vectorised), and in every step
    the hand-placed rows of _special_rows and the late features (quiet_features) in its last rows.  Columns distinct and ascending inside a row."""
    assert p >= MIN_P
    rng = np.random.default_rng(seed)
    ghost, late = quiet_features(p)
    free = np.setdiff1d(np.arange(p, dtype=np.int64), np.concatenate([ghost, late]))
    assert len(free) > LONG_ROW
    n = 3 * rows
    lens = rng.poisson(12, n).clip(0, p)
    lens[rng.integers(0, n, max(1, n // 50))] = 0
    lens[rng.integers(0, n, max(1, n // 50))] = 1
    special = {}
    for s in range(3):
        for i, length in _special_rows(rows):
            special[s * rows + i] = length
    for r in special:
        lens[r] = 0
    row_of = np.repeat(np.arange(n, dtype=np.int64), lens)
    col = free[rng.integers(0, len(free), len(row_of))]
    srow, scol = [], []
    for r, length in special.items():
        srow.append(np.full(length, r, np.int64))
        scol.append(free[rng.choice(len(free), length, replace=False)])
    for s in range(3):   # late feature i in row (i mod LATE_ROWS) of the step's last rows
        srow.append((s + 1) * rows - LATE_ROWS + np.arange(len(late), dtype=np.int64) % LATE_ROWS)
        scol.append(late)
    row_of, col = np.concatenate([row_of] + srow), np.concatenate([col] + scol)
    order = np.lexsort((col, row_of))
    row_of, col = row_of[order], col[order]
    keep = np.ones(len(col), bool)
    keep[1:] = (row_of[1:] != row_of[:-1]) | (col[1:] != col[:-1])   # a column drawn twice in a row stays once
    row_of, col = row_of[keep], col[keep]
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(row_of, minlength=n))
    val = rng.normal(0, 1, len(col)).astype(np.float32) if values else np.ones(len(col), np.float32)
    return dict(n=n, p=p, rows=rows, rp=rp, col=col.astype(np.uint32), val=val)


def labels(n, seed, task):
    rng = np.random.default_rng(seed + 7)
    if task == "classification":
        return np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    return rng.normal(0, 0.5, n).astype(np.float32)


def start_params(p, k, seed, task="classification"):
    """(w0, w[p], v[k][p]) exactly representable in float32, scaled so that the 5 000-entry row's score stays of the order of one: its pair term
    has a standard deviation of about 0.5 sqrt(2 k) L sigma^2 and its linear term one of sqrt(L) sigma_w.  A saturated score would make that
    row's multiplier vanish -- and with it everything a fault in that row's sums could change.  Regression has no such saturation (its multiplier is
    the clamped score minus the target), and takes linear weights ten times as large: the scores of ordinary rows then leave [-0.2, 0.3] on
    both sides, so both clamps act."""
    rng = np.random.default_rng(seed + 13)
    sigma = (0.5 * np.sqrt(2.0 * k) * LONG_ROW) ** -0.5
    w0 = float(np.float32(rng.normal(0, 0.1)))
    w = rng.normal(0, 0.1 if task == "regression" else 0.01, p).astype(np.float32).astype(np.float64)
    v = rng.normal(0, sigma, (k, p)).astype(np.float32).astype(np.float64)
    return w0, w, v


def case_seed(case):
    return int.from_bytes(hashlib.blake2b(case["name"].encode(), digest_size=4).digest(), "little") % 100000


def matrix_key(case):
    return (case["rows"], case["p"], case["values"])


def case_problem(case):
    rows, p, values = matrix_key(case)
    return problem(rows, p, values, 17 + rows % 1000 + (1 if values else 0))


# --------------------------------------------------------------------------------------------------------------------- the reference
def oracle_params(case):
    import oracle
    sum_ = case["solver"] == "ftrl_sum"
    regr = case["task"] == "regression"
    return oracle.params(task=oracle.REGRESSION if regr else oracle.CLASSIFICATION, k=case["k"], k0=bool(case["keep_w0"]), k1=bool(case["keep_w1"]),
                         l2_regw=L2, l2_regv=L2, learn_rate=LEARN_RATE, batch_mean=not sum_, **(dict(min_target=-0.2, max_target=0.3) if regr else {}))


def engine_options(case, L):
    regr = case["task"] == "regression"
    o = dict(task=L.TASK_REGRESSION if regr else L.TASK_CLASSIFICATION, solver=L.SOLVER_FTRL if case["solver"] == "ftrl_sum" else L.SOLVER_SGD,
             num_factor=case["k"], learn_rate=LEARN_RATE, l2_w1=L2, l2_v=L2, mode=L.MODE_MINIBATCH, batch_rows=case["rows"], state_fp64=int(case["fp64"]),
             keep_w0=case["keep_w0"], keep_w1=case["keep_w1"], batch_reduce=L.REDUCE_SUM if case["solver"] == "ftrl_sum" else L.REDUCE_MEAN)
    if regr:
        o.update(min_target=-0.2, max_target=0.3)
    if case["tile_rows"]:
        o["tile_rows"] = case["tile_rows"]
    if case["chunks"] > 1:
        o["exchange_chunks"] = case["chunks"]
    return o


def has_q(case):
    return case["solver"] == "ftrl_sum"


def multipliers(P, prob, y, w0, w, v, b0, b1):
    """The oracle's gradient multiplier of rows [b0, b1): oracle.predict_batch on those rows, then oracle.grad_mult row by row."""
    import oracle
    rp = prob["rp"]
    X = oracle.Matrix(rp[b0:b1 + 1] - rp[b0], prob["col"][rp[b0]:rp[b1]], prob["val"][rp[b0]:rp[b1]], prob["p"])
    y_hat = oracle.predict_batch(P, X, w0, w, np.asarray(v, np.float64).ravel())
    return np.array([oracle.grad_mult(P, float(y_hat[i]), float(y[b0 + i]))[0] for i in range(b1 - b0)], np.float64)


def sums_reference(prob, k, m, w0, w, v, b0, b1):
    """fmo_batch_sums over rows [b0, b1) restated over the flattened entries, in fp64, given the rows' multipliers m[b1 - b0]: the sums G0, Q0,
    Gw[p], Qw[p], cw[p], Gv[k][p], Qv[k][p] -- np.bincount adds a bin's weights in entry order, the oracle's own order -- and for every one of
    them the un-cancelled absolute sum it is measured against:
        A_v[f][j] = sum over the rows' entries of |m x| (|s_f| + |v_jf x|)     (g = m x (s_f - v_jf x))
        A_w[j]    = sum |m x|,   the Q planes: the sums of those terms' squares,   G0: sum |m|,   Q0: sum m^2."""
    rp, p = prob["rp"], prob["p"]
    e0, e1 = int(rp[b0]), int(rp[b1])
    col = prob["col"][e0:e1].astype(np.int64)
    x = prob["val"][e0:e1].astype(np.float64)
    row = np.repeat(np.arange(b1 - b0, dtype=np.int64), np.diff(rp[b0:b1 + 1]))
    R = b1 - b0
    mx = m[row] * x
    amx = np.abs(mx)
    out = dict(G0=float(np.sum(m)), Q0=float(np.sum(m * m)), A0=float(np.sum(np.abs(m))), rows=R,
               Gw=np.bincount(col, mx, p), Qw=np.bincount(col, mx * mx, p), cw=np.bincount(col, minlength=p).astype(np.float64),
               Aw=np.bincount(col, amx, p), Gv=np.zeros((k, p)), Qv=np.zeros((k, p)), Av=np.zeros((k, p)), AQv=np.zeros((k, p)))
    out["AQw"] = out["Qw"]
    for f in range(k):
        vx = v[f, col] * x
        s = np.bincount(row, vx, R)          # the row's factor sum, entries added in row order (core/Model.h:83-97)
        g = m[row] * (s[row] * x - vx * x)   # fmo_batch_sums: mult * (m_sum[f] * x - v * x * x)
        a = amx * (np.abs(s[row]) + np.abs(vx))
        out["Gv"][f] = np.bincount(col, g, p)
        out["Qv"][f] = np.bincount(col, g * g, p)
        out["Av"][f] = np.bincount(col, a, p)
        out["AQv"][f] = np.bincount(col, a * a, p)
    return out


def reference(case, prob, y, params, b0, b1):
    w0, w, v = params
    m = multipliers(oracle_params(case), prob, y, w0, w, v, b0, b1)
    return sums_reference(prob, case["k"], m, w0, w, v, b0, b1)


def worst_ratio(got, ref, scale):
    """max over the elements of |got - ref| / scale, an element whose scale is 0 counting through `exact` instead (it must then be 0 itself)."""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    live = scale > 0
    r = float(np.max(np.abs(got[live] - ref[live]) / scale[live])) if live.any() else 0.0
    return r if np.isfinite(r) else float("inf")


def split_buffer(buf, layout, p, kp, k, q):
    """The planes of an exchange buffer (fmx_internal.h: blocks of F features, each GV[F][kp] | GW[F] | CNT[F] (| QV[F][kp] | QW[F]), then the
    tail) as dict Gv[kp][p], Gw[p], cw[p] (, Qv, Qw), tail[4], and `spare`: every element of the blocks that belongs to no feature."""
    blocks, F, elems, tail = layout
    assert blocks * F >= p and tail == blocks * elems and len(buf) == tail + 4 and elems == F * kp * (2 if q else 1) + F * (3 if q else 2)
    b = buf[:tail].reshape(blocks, elems)
    gv = b[:, :F * kp].reshape(blocks * F, kp)
    out = dict(Gv=gv[:p].T, Gw=b[:, F * kp:F * kp + F].reshape(-1)[:p], cw=b[:, F * kp + F:F * kp + 2 * F].reshape(-1)[:p], tail=buf[tail:])
    spare = [gv[p:].ravel(), b[:, F * kp:F * kp + F].reshape(-1)[p:], b[:, F * kp + F:F * kp + 2 * F].reshape(-1)[p:]]
    if q:
        o = F * kp + 2 * F
        qv = b[:, o:o + F * kp].reshape(blocks * F, kp)
        out.update(Qv=qv[:p].T, Qw=b[:, o + F * kp:o + F * kp + F].reshape(-1)[:p])
        spare += [qv[p:].ravel(), b[:, o + F * kp:].reshape(-1)[p:]]
    out["spare"] = np.concatenate(spare)
    return out


def compare(planes, ref, k, q):
    """One figure per quantity of a step: the worst |device - reference| / absolute sum per plane, and the exact properties as booleans."""
    live = ref["cw"] > 0
    dead = ~live
    r = dict(gv=worst_ratio(planes["Gv"][:k], ref["Gv"], ref["Av"]), gw=worst_ratio(planes["Gw"], ref["Gw"], ref["Aw"]),
             g0=abs(float(planes["tail"][0]) - ref["G0"]) / ref["A0"], q0=abs(float(planes["tail"][1]) - ref["Q0"]) / max(ref["Q0"], 1e-300),
             pad_max=float(np.max(np.abs(planes["Gv"][k:]), initial=0.0)), spare_max=float(np.max(np.abs(planes["spare"]), initial=0.0)),
             cnt_exact=bool(np.array_equal(np.asarray(planes["cw"], np.float64), ref["cw"])),
             rows_exact=bool(float(planes["tail"][2]) == ref["rows"] // 4096 and float(planes["tail"][3]) == ref["rows"] % 4096),
             # features that occur in no active row: every sum exactly 0; so are the padded factor slots of every feature and the buffer's spare elements
             dead=int(dead.sum()), dead_zero=bool(np.all(planes["Gv"][:, dead] == 0) and np.all(planes["Gw"][dead] == 0)),
             pad_zero=bool(np.all(planes["Gv"][k:] == 0)), spare_zero=bool(np.all(planes["spare"] == 0)),
             finite=bool(np.isfinite(planes["Gv"]).all() and np.isfinite(planes["Gw"]).all() and np.isfinite(planes["tail"]).all()),
             # an element whose absolute sum is 0 (every term an exact zero) is an exact zero on the device too
             zero_scale_zero=bool(np.all(planes["Gv"][:k][ref["Av"] == 0] == 0) and np.all(planes["Gw"][ref["Aw"] == 0] == 0)))
    if q:
        r.update(qv=worst_ratio(planes["Qv"][:k], ref["Qv"], ref["AQv"]), qw=worst_ratio(planes["Qw"], ref["Qw"], ref["AQw"]))
        r["dead_zero"] = bool(r["dead_zero"] and np.all(planes["Qv"][:, dead] == 0) and np.all(planes["Qw"][dead] == 0))
        r["pad_zero"] = bool(r["pad_zero"] and np.all(planes["Qv"][k:] == 0))
        r["finite"] = bool(r["finite"] and np.isfinite(planes["Qv"]).all() and np.isfinite(planes["Qw"]).all())
    return r


# --------------------------------------------------------------------------------------------------------------------- the child process
def _counter(L):
    import ctypes
    a = (ctypes.c_int64 * 6)()
    L.check(L.lib().fmx_debug_rows_launches(a))
    return np.array(list(a), np.int64)


def _set_variant(variant):
    for name in ("FMX_ROWS_PULL", "FMX_ROWS_FLAT"):
        os.environ.pop(name, None)
    if variant == "pull":
        os.environ["FMX_ROWS_PULL"] = "1"
    elif variant == "flat":
        os.environ["FMX_ROWS_FLAT"] = "1"


def _read_buffer(e, util):
    e.sync()
    ptr, n = e.grad_buffer()
    return util.read_device(ptr, n, np.float64 if e.grad_elem_bytes() == 8 else np.float32)


def _cached(path, compute):
    """An npz of arrays and scalars: computed by the first child that needs it, read back by the later ones."""
    if path is None:
        return compute()
    if not os.path.exists(path):
        np.savez(path + ".tmp.npz", **compute())
        os.replace(path + ".tmp.npz", path)
    with np.load(path) as z:
        return {name: (z[name] if z[name].ndim else z[name].item()) for name in z.files}


def _reference(job, case, prob, y, held, b0, b1):
    """The reference of one step at the parameters the engine holds.  Children whose runs are bit-identical hold the same parameters: a case that
    runs in several children (and is small enough to keep) finds its reference under the digest of those parameters."""
    path = None
    if len(case["children"]) > 1 and case["k"] <= 64:
        h = hashlib.blake2b(np.float64(held[0]).tobytes() + held[1].tobytes() + held[2].tobytes(), digest_size=12).hexdigest()
        path = os.path.join(job["ref"], f"{case['name']}.{b0}.{b1}.{h}.npz")
    return _cached(path, lambda: reference(case, prob, y, held, b0, b1))


def _run_case(job, case, prob, engine, L, util):
    p, k, fp64 = case["p"], case["k"], case["fp64"]
    kp, q = padded(k, fp64), has_q(case)
    seed = case_seed(case)
    y = labels(prob["n"], seed, case["task"])
    m = engine.Matrix.from_csr(prob["rp"], prob["col"], prob["val"], p, y)
    if case["w_in_row"]:
        os.environ["FMX_W_IN_ROW"] = "1"   # read at engine creation
    try:
        e = engine.Engine(p, **engine_options(case, L))
    finally:
        os.environ.pop("FMX_W_IN_ROW", None)
    e.set_params(*start_params(p, k, seed, case["task"]))
    layout = e.grad_layout()
    out = dict(w_in_row=bool(e.w_in_row()) if not fp64 else False, blocks=layout[0], steps=[])
    t_ref = 0.0
    for batch, limit, active in case_steps(case):
        held = e.get_params()   # the oracle starts every step from what the engine holds: errors do not compound
        t0 = time.time()
        ref = _reference(job, case, prob, y, held, batch * case["rows"], batch * case["rows"] + active)
        t_ref += time.time() - t0
        step = dict(rows=active, variants={})
        for variant in variants_of(case, active):
            _set_variant(variant)
            before = _counter(L)
            if case["chunks"] > 1:
                e.grad_begin(m, batch, limit)
                for c in range(layout[0]):
                    e.grad_chunk(m, c)
            else:
                e.grad(m, batch, limit)
            buf = _read_buffer(e, util)
            launches = _counter(L) - before
            _set_variant("plain")
            r = compare(split_buffer(buf, layout, p, kp, k, q), ref, k, q)
            r.update(launches=[int(x) for x in launches], digest=hashlib.blake2b(buf.tobytes(), digest_size=16).hexdigest())
            step["variants"][variant] = r
        out["steps"].append(step)
        if case["chunks"] > 1:
            for c in range(layout[0]):
                e.apply_chunk(c, 0, c == layout[0] - 1)
        else:
            e.apply(0)          # the parameters move between the steps
    after = e.get_params()
    out["moved"] = bool(np.any(after[2] != held[2]))
    out["reference_seconds"] = t_ref
    e.close()
    m.close()
    return out


def _run_compact_case(job, case, prob, engine, L, util):
    """One sparse tile per step through fmx_grad_compact: a record G[kp] (| Q[kp]) | Gw | Qw | count | id per occurring feature of the tile, ids
    ascending, and the 4-element tail."""
    p, k, fp64 = case["p"], case["k"], case["fp64"]
    kp, q = padded(k, fp64), has_q(case)
    seed = case_seed(case)
    y = labels(prob["n"], seed, case["task"])
    m = engine.Matrix.from_csr(prob["rp"], prob["col"], prob["val"], p, y)
    e = engine.Engine(p, **engine_options(case, L))
    e.set_params(*start_params(p, k, seed, case["task"]))
    rec_elems, cap, usable = e.compact_info(m)
    dt = np.float64 if fp64 else np.float32
    out = dict(usable=bool(usable), rec_elems=int(rec_elems), steps=[])
    held = e.get_params()
    for batch, limit, active in case_steps(case):
        b0 = batch * case["rows"]
        ref = reference(case, prob, y, held, b0, b0 + active)
        tile = np.unique(prob["col"][prob["rp"][b0]:prob["rp"][b0 + case["rows"]]]).astype(np.int64)   # the features of the whole tile
        before = _counter(L)
        e.grad_compact(m, batch, limit)
        e.sync()
        ptr, n, tail_ptr = e.compact_records()
        rec = util.read_device(ptr, n * rec_elems, dt).reshape(n, rec_elems)
        tail = util.read_device(tail_ptr, 4, dt)
        launches = _counter(L) - before
        qo = kp if q else 0
        ids = (rec[:, kp + qo + 3].copy().view(np.uint32 if not fp64 else np.uint64)).astype(np.int64)
        ok_ids = bool(n == len(tile) and np.array_equal(ids, tile))
        planes = dict(Gv=np.zeros((kp, p)), Gw=np.zeros(p), cw=np.zeros(p), tail=tail, spare=np.zeros(1))
        if q:
            planes.update(Qv=np.zeros((kp, p)), Qw=np.zeros(p))
        if ok_ids:
            planes["Gv"][:, ids] = rec[:, :kp].T
            planes["Gw"][ids] = rec[:, kp + qo]
            planes["cw"][ids] = rec[:, kp + qo + 2]
            if q:
                planes["Qv"][:, ids] = rec[:, kp:2 * kp].T
                planes["Qw"][ids] = rec[:, kp + qo + 1]
        r = compare(planes, ref, k, q)
        r.update(ids_ascending=ok_ids, records=int(n), launches=[int(x) for x in launches], no_q_slot_zero=bool(q or np.all(rec[:, kp + 1] == 0)))
        out["steps"].append(dict(rows=active, variants=dict(plain=r)))
    e.close()
    m.close()
    return out


def child_main(path):
    with open(path) as f:
        job = json.load(f)
    from fmwr_amd import _lib as L
    from fmwr_amd import engine
    from tests import util
    t0 = time.time()
    results, probs = {}, {}
    for case in job["cases"]:
        key = matrix_key(case)
        if key not in probs:
            probs.clear()    # cases come sorted by matrix: one at a time stays resident
            probs[key] = _cached(os.path.join(job["ref"], "matrix.%d.%d.%d.npz" % key), lambda: case_problem(case))
        t1 = time.time()
        try:
            results[case["name"]] = (_run_compact_case if case.get("compact") else _run_case)(job, case, probs[key], engine, L, util)
        except L.FmxError as err:
            if err.status not in (L.ERR_INVALID, L.ERR_STATE):   # anything the device reported ends the child
                raise
            results[case["name"]] = dict(error=str(err), steps=[])   # a call the library refused: the parent's test of this case fails with its words
        results[case["name"]]["seconds"] = time.time() - t1
    with open(job["out"], "w") as f:
        json.dump(dict(seconds=time.time() - t0, cases=results), f)
    print("DONE", len(job["cases"]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main(sys.argv[1])
