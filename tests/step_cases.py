"""Cases, matrix builders, the oracle run and the child process shared by tests/test_gpu_step_forms.py, tests/test_step_cases_cpu.py and (the
case list only) tests/test_gpu_cols_lean.py.

Everything above `child_main` runs without a GPU: the case lists, the hand-made matrices (a ladder of list lengths, a tile with thousands of
long lists), the wrap-around batch schedule and the fp64 oracle run.  `child_main` is what a fresh child process executes per runtime form of
the mini-batch step's second half (the switches are read once per process): `python -m tests.step_cases <job.json>`.  A child asserts nothing
about the numerics; it writes one figure per quantity and the parent's tests hold them to their bars."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEARN_RATE, L2, L1 = 0.05, 1e-3, 1e-3   # the lean test's hyper-parameters (l1 = 0 for plain "sgd"); every other one is the engine's default
# TDAP on the hand-made matrices takes a stronger l2.  A coordinate's first TDAP update is theta = -(z -+ l1) / (|G| / alpha + l2) with
# z = G - |G| theta / alpha: a jump of alpha * sign(G), smoothed only over |G| of the order of l1 and alpha * l2.  With l1 = l2 = 1e-3 a coordinate
# whose mean gradient lands in that zone turns an absolute error of the gradient sum into several hundred times as much in theta, and a tile of
# one-entry lists over 400 000 features has millions of coordinates to find one.  That is the solver's conditioning, not a kernel's arithmetic:
# the fp64 ORACLE with nothing but its S rows, multipliers and stored state rounded to float32 (profiles/tdap_fp32_amplification.py) leaves the
# pure oracle by 2e-5 .. 3e-5 of max |V| on such cases at l2 = 1e-3 -- what every form of the engine showed (1.7e-5 .. 4.1e-5, all forms alike,
# 1e-13 with fp64 tables) -- by up to 8e-6 at l2 = 0.1 and by 3e-7 .. 6e-7 at l2 = 0.3.  The bar (V_RTOL) stays; the cases take l2 = 0.3, where
# every TDAP case still fails on a library whose sums_add is broken (profiles/step_forms_parity.txt).  FTRL's beta = 1 keeps its denominator
# above 10: no such zone.
TDAP_L2 = 0.3
SOLVERS = ("sgd", "sgd_l1", "ftrl", "tdap")

# --------------------------------------------------------------------------------------------------------------------- part A: the lean test's cases
N, Z, BATCH = 4096, 8, 2048
TOTAL = N + N // 2 + 5   # three full steps and one of five rows


def _case(name, k, values, solver, law="uniform", p=2000):
    return dict(name=name, k=k, values=values, solver=solver, law=law, p=p)


CASES = [_case(f"dense_k{k}_{'val' if v else 'onehot'}_sgd", k, v, "sgd") for k in (16, 12, 6, 32) for v in (False, True)]
CASES += [_case("dense_k8_val_sgd", 8, True, "sgd"), _case("dense_k4_onehot_ftrl", 4, False, "ftrl")]   # k == kp < 16: the specialised kernel without embedding
CASES += [_case(f"dense_k{k}_{'val' if v else 'onehot'}_{s}", k, v, s) for s in ("sgd_l1", "ftrl", "tdap") for k, v in ((16, False), (12, True))]
CASES += [_case(f"dense_zipf_k{k}_{s}", k, v, s, law="zipf") for k, v, s in ((16, False, "sgd"), (16, True, "ftrl"), (6, True, "sgd_l1"), (32, False, "sgd"))]
CASES += [_case(f"sparse_zipf_k{k}_{'val' if v else 'onehot'}_{s}", k, v, s, law="zipf", p=20000)
          for k, v, s in ((16, False, "sgd"), (16, True, "sgd"), (12, False, "ftrl"), (6, True, "tdap"), (32, True, "sgd"))]
CASES += [_case(f"sparse_uniform_k{k}_{'val' if v else 'onehot'}_{s}", k, v, s, p=400000)
          for k, v, s in ((16, False, "sgd"), (16, True, "sgd_l1"), (12, True, "sgd"), (32, False, "ftrl"))]


def schedule(n, batch, total):
    """Rows [b0, b1) of every step of fmx_train in MINIBATCH mode: consecutive batches, wrapping at the end of the matrix, the last one cut by
    `total` (the schedule of test_minibatch_matches_oracle)."""
    steps, done, s, nb = [], 0, 0, -(-n // batch)
    while done < total:
        b0 = (s % nb) * batch
        rows = min(batch, n - b0, total - done)
        steps.append((b0, b0 + rows))
        done += rows
        s += 1
    return steps


# --------------------------------------------------------------------------------------------------------------------- part B: a ladder of list lengths
LADDER = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025, 2049)   # around a round of FMX_U = 4 entries, the inline first entry, long_min = 64, LIST_SEG = 1024
LONG_MIN = 64
STEP = 4096              # rows per step; the matrix holds three steps, the third runs truncated
LIMIT = 2501             # rows of the truncated third step (no multiple of a round, a wave or a workgroup)
GHOSTS = (3, 65)         # ladder lengths whose third-step entries ALL sit in inactive rows: a short list and a long one
Z_FILL = 8               # filler entries per row
REGIMES = dict(dense=dict(p=600, pool=0),         # a tile's entries >= p: dense directory (every filler list ~56 entries)
               inline=dict(p=60000, pool=5000),   # entries < p, fillers from a pool of 5 000 features (~6.5 entries per list): sparse directory, first entry inline
               single=dict(p=400000, pool=0))     # fillers uniform over 400 000 features: mostly one-entry lists, no inline entry


def ladder_ids(p):
    """The ladder's feature ids (spread over several workgroups of lists, below every regime's p) and the id of the feature that occurs only in
    inactive rows of the truncated step."""
    ids = 5 + 37 * np.arange(len(LADDER) + 1, dtype=np.int64)
    assert ids[-1] < p
    return ids[:-1], int(ids[-1])


def _csr(n, p, rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert not np.any((rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])), "a row holds a column twice"
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), cols.astype(np.uint32), vals.astype(np.float32)


def _strata(rng, pool, parts, rows):
    """[rows][parts] ids: one of every contiguous part of `pool`, so a row's ids are distinct and ascending."""
    cut = np.linspace(0, len(pool), parts + 1).astype(np.int64)
    return np.stack([pool[cut[c] + rng.integers(0, cut[c + 1] - cut[c], rows)] for c in range(parts)], axis=1)


def _labels(n, seed):
    return np.where(np.random.default_rng(seed + 7).random(n) < 0.5, -1.0, 1.0).astype(np.float32)


def ladder_problem(regime, values, seed):
    """Three steps of STEP rows.  In each of them ladder feature i occurs in exactly LADDER[i] rows, and every row takes Z_FILL filler entries
    that set the directory's regime.  The third step runs with rows_limit = LIMIT: the ladder's lists are cut where their rows fall, the lists
    of the GHOSTS lengths lie wholly behind the limit (their features have a history from steps 0 and 1, and nothing to add in step 2), and one
    more feature (`virgin`) occurs nowhere but in two inactive rows."""
    R = REGIMES[regime]
    p = R["p"]
    rng = np.random.default_rng(seed)
    ids, virgin = ladder_ids(p)
    free = np.setdiff1d(np.arange(p, dtype=np.int64), np.append(ids, virgin))
    pool = np.sort(rng.choice(free, R["pool"], replace=False)) if R["pool"] else free
    rows, cols = [], []
    for s in range(3):
        fill = _strata(rng, pool, Z_FILL, STEP)
        rows.append(np.repeat(np.arange(STEP, dtype=np.int64), Z_FILL) + s * STEP)
        cols.append(fill.ravel())
        for j, length in zip(ids, LADDER):
            if s == 2 and length in GHOSTS:
                r = LIMIT + rng.choice(STEP - LIMIT, length, replace=False)
            else:
                r = rng.choice(STEP, length, replace=False)
            rows.append(r.astype(np.int64) + s * STEP)
            cols.append(np.full(length, j, np.int64))
        if s == 2:
            rows.append(LIMIT + rng.choice(STEP - LIMIT, 2, replace=False).astype(np.int64) + s * STEP)
            cols.append(np.full(2, virgin, np.int64))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.normal(0, 1, len(cols)).astype(np.float32) if values else np.ones(len(cols), np.float32)
    n = 3 * STEP
    rp, col, val = _csr(n, p, rows, cols, vals)
    ghosts = [int(ids[LADDER.index(g)]) for g in GHOSTS]
    return dict(n=n, p=p, rp=rp, col=col, val=val, y=_labels(n, seed), batch=STEP, ids=ids, virgin=virgin, ghosts=ghosts + [virgin],
                engine_steps=[(0, 0), (1, 0), (2, LIMIT)], oracle_steps=[(0, STEP), (STEP, 2 * STEP), (2 * STEP, 2 * STEP + LIMIT)])


def _ladder_cases():
    """A Latin-square style selection: every k meets every solver (20 cases, directory and value kind rotating so that every k sees all three
    directories and both value kinds), plus two more per k on other (directory, value kind) pairs: 30 cases, not the product's 120."""
    ks, regimes = (16, 12, 6, 8, 32), ("dense", "inline", "single")   # BITS, PAD in a quad, PAD in a pair, no embedding, rows too wide for the lean kernel
    out = []

    def add(a, b, regime, values):
        k, s = ks[a], SOLVERS[b]
        out.append(dict(name=f"{regime}_k{k}_{'val' if values else 'onehot'}_{s}", part="B", k=k, solver=s, regime=regime, values=bool(values), seed=500 + len(out),
                        l2=TDAP_L2 if s == "tdap" else L2))
    for a in range(len(ks)):
        for b in range(len(SOLVERS)):
            add(a, b, regimes[(a + b) % 3], b % 2)
    for a in range(len(ks)):
        for j in range(2):
            b = (a + 2 * j + 1) % 4
            add(a, b, regimes[(a + b + 1) % 3], (b + 1) % 2)
    return out


LADDER_CASES = _ladder_cases()

# --------------------------------------------------------------------------------------------------------------------- part C: thousands of long lists
SIDE_MIN_SEG = 2048      # long-list segments of a list-by-list tile from which the two long-list kernels go to the side stream
STEP_C, LIMIT_C, P_C = 16384, 9001, 400000
POOL_PARTS, POOL_PART, COLD_PARTS = 12, 183, 5   # a row takes one feature of each of 12 parts of 183: 2 196 lists of ~90 entries per step


def side_problem(values, seed):
    """Two steps of STEP_C rows (the second runs truncated at LIMIT_C).  Every row takes 12 entries from a pool of 2 196 features -- so each
    pool feature's list holds ~90 entries, one segment above long_min -- and 5 spread over the other ~398 000 features, which keeps the tile
    sparse (278 528 entries < p) and its average list short (list-by-list form)."""
    rng = np.random.default_rng(seed)
    n = 2 * STEP_C
    pool = np.arange(POOL_PARTS * POOL_PART, dtype=np.int64)
    cold = np.arange(len(pool), P_C, dtype=np.int64)
    cols = np.concatenate([_strata(rng, pool, POOL_PARTS, n), _strata(rng, cold, COLD_PARTS, n)], axis=1)
    z = cols.shape[1]
    rows = np.repeat(np.arange(n, dtype=np.int64), z)
    vals = rng.normal(0, 1, n * z).astype(np.float32) if values else np.ones(n * z, np.float32)
    rp, col, val = _csr(n, P_C, rows, cols.ravel(), vals)
    return dict(n=n, p=P_C, rp=rp, col=col, val=val, y=_labels(n, seed), batch=STEP_C, ghosts=[],
                engine_steps=[(0, 0), (1, LIMIT_C)], oracle_steps=[(0, STEP_C), (STEP_C, STEP_C + LIMIT_C)])


SIDE_CASES = [dict(name="side_k16_val_sgd", part="C", k=16, solver="sgd", values=True, seed=900),
              dict(name="side_k12_onehot_ftrl", part="C", k=12, solver="ftrl", values=False, seed=901)]


def step_lists(prob, step):
    """Entries per occurring feature of the rows of step `step` (a full tile): (feature ids, list lengths)."""
    b = prob["batch"]
    c = prob["col"][prob["rp"][step * b]:prob["rp"][min((step + 1) * b, prob["n"])]]
    return np.unique(c, return_counts=True)


# --------------------------------------------------------------------------------------------------------------------- the oracle's side
def oracle_params(case):
    import oracle
    l1 = 0.0 if case["solver"] == "sgd" else L1
    l2 = case.get("l2", L2)
    return oracle.params(task=oracle.CLASSIFICATION, k=case["k"], l1_regw=l1, l1_regv=l1, l2_regw=l2, l2_regv=l2, learn_rate=LEARN_RATE)


def engine_options(case, L, batch_rows, **extra):
    l1 = 0.0 if case["solver"] == "sgd" else L1
    solver = {"sgd": L.SOLVER_SGD, "sgd_l1": L.SOLVER_SGD, "ftrl": L.SOLVER_FTRL, "tdap": L.SOLVER_TDAP}[case["solver"]]
    l2 = case.get("l2", L2)
    return dict(task=L.TASK_CLASSIFICATION, solver=solver, num_factor=case["k"], learn_rate=LEARN_RATE, l2_w1=l2, l2_v=l2, l1_w1=l1, l1_v=l1,
                mode=L.MODE_MINIBATCH, batch_rows=batch_rows, **extra)


def _oracle_rows(mb, ids):
    """Everything the oracle holds per feature (parameters and optimizer state) for the listed features, as one vector."""
    p, k = mb.X.p, mb.P.k
    ids = np.asarray(ids, np.int64)
    parts = [mb.w[ids], mb.v.reshape(k, p)[:, ids].ravel()]
    for name in ("q_w", "z_w", "n_w"):
        if hasattr(mb, name):
            parts.append(getattr(mb, name)[ids])
    for name in ("q_v", "z_v", "n_v"):
        if hasattr(mb, name):
            parts.append(getattr(mb, name).reshape(k, p)[:, ids].ravel())
    if hasattr(mb, "sw"):
        parts += [mb.sw.reshape(5, p)[:, ids].ravel(), mb.sv.reshape(5, k, p)[:, :, ids].ravel()]
    return np.concatenate(parts)


def oracle_run(case, rp, col, val, y, p, w0, w, v, steps, ghosts=()):
    """The fp64 oracle over rows [b0, b1) of every step, from (w0, w[p], v[k][p]).  Returns w0, w, v[k][p] and whether the listed `ghosts` kept
    their parameters and optimizer state through the last step (they must: none of their entries lies in its rows)."""
    import oracle
    P = oracle_params(case)
    X = oracle.Matrix(rp, col, val, p)
    cls = {"sgd": oracle.SgdMinibatch, "sgd_l1": oracle.SgdMinibatch, "ftrl": oracle.FtrlMinibatch, "tdap": oracle.TdapMinibatch}[case["solver"]]
    mb = cls(P, X, y, w0, w, np.asarray(v, np.float64).ravel())
    before = None
    for i, (b0, b1) in enumerate(steps):
        if i == len(steps) - 1 and len(ghosts):
            before = _oracle_rows(mb, ghosts)
        mb.step(b0, b1)
    still = True if before is None else bool(np.array_equal(before, _oracle_rows(mb, ghosts)))
    return dict(w0=float(mb.w0.value), w=mb.w.copy(), v=mb.v.reshape(case["k"], p).copy(), ghost_still=still)


def start_params(p, k, seed):
    """(w0, w[p], v[k][p]) exactly representable in float32: V ~ N(0, 0.05) as the lean test's init_normal, w ~ N(0, 0.1)."""
    from tests import util
    return util.params(p, k, seed, stdev=0.05, fp32=True)


# --------------------------------------------------------------------------------------------------------------------- the child process
def _counters(L):
    import ctypes
    a, b = (ctypes.c_int64 * 3)(), (ctypes.c_int64 * 2)()
    L.check(L.lib().fmx_debug_cols_launches(a))
    L.check(L.lib().fmx_debug_long_launches(b))
    return np.array(list(a) + list(b), np.int64)


def _file_digest(path):
    h = hashlib.blake2b(digest_size=16)
    with open(path, "rb") as f:
        for piece in iter(lambda: f.read(1 << 24), b""):
            h.update(piece)
    return h.hexdigest()


def checkpoint_rows(path, ids):
    """(the bytes every per-feature table of a checkpoint holds for the listed features, the number of table pairs).  The file is a 64-byte header,
    the scalars, then pairs of tables [p][kp] and [p] -- parameters first, then the solver's optimizer tables -- of float32, or float64 with
    state_fp64 (fmx_api.hip: ckpt_tables)."""
    head = np.fromfile(path, np.uint8, 64)
    assert bytes(head[:4]) == b"FMX1"
    p = int(head[8:16].view(np.uint64)[0])
    kp = int(head[20:24].view(np.int32)[0])
    off = 64 + 8 * int(head[32:36].view(np.uint32)[0])
    elem = 8 if int(head[36:40].view(np.uint32)[0]) else 4
    body, pair = os.path.getsize(path) - off, p * (kp + 1) * elem
    assert body > 0 and body % pair == 0, (body, pair)
    mm = np.memmap(path, np.uint8, "r", offset=off)
    out = []
    for t in range(body // pair):
        for j in ids:
            out.append(bytes(mm[t * pair + j * kp * elem:t * pair + (j + 1) * kp * elem]))
            out.append(bytes(mm[t * pair + (p * kp + j) * elem:t * pair + (p * kp + j + 1) * elem]))
    del mm
    return b"".join(out), body // pair


def _errors(got, ref, start, touched):
    from tests import util
    g0, gw, gv = got
    w0, w, v = start
    return dict(err_v=float(util.rel_err(gv, ref["v"])), err_w=float(util.rel_err(gw, ref["w"])), err_w0=float(abs(g0 - ref["w0"]) / max(1.0, abs(ref["w0"]))),
                finite=bool(np.isfinite(g0) and np.isfinite(gw).all() and np.isfinite(gv).all()), moved=bool(np.any(gv != v)),
                untouched=int((~touched).sum()), untouched_kept=bool(np.array_equal(gv[:, ~touched], v[:, ~touched]) and np.array_equal(gw[~touched], w[~touched])),
                params_digest=hashlib.blake2b(np.float64(g0).tobytes() + gw.tobytes() + gv.tobytes(), digest_size=16).hexdigest())


def _reference(job, case, compute):
    """The oracle's answer for a case: computed by the first child that needs it, read back by the later ones."""
    path = os.path.join(job["ref"], case["name"] + ".npz")
    if not os.path.exists(path):
        t0 = time.time()
        ref = compute()
        np.savez(path, w0=np.float64(ref["w0"]), w=ref["w"], v=ref["v"], ghost_still=np.bool_(ref["ghost_still"]), seconds=np.float64(time.time() - t0))
    z = np.load(path)
    return dict(w0=float(z["w0"]), w=z["w"], v=z["v"], ghost_still=bool(z["ghost_still"]), seconds=float(z["seconds"]))


def _run_lean_case(job, case, engine, L):
    """Part A: the lean test's run of a case (device-generated matrix, init_normal, fmx_train), against the oracle on the exported rows."""
    i, p, k = case["index"], case["p"], case["k"]
    m = engine.Matrix.synthetic_iid(N, p, Z, 1000 + i, law=L.COLUMNS_ZIPF if case["law"] == "zipf" else L.COLUMNS_UNIFORM)
    if case["values"]:
        m.synthetic_values(2000 + i)
    rp, col, val, y = m.export()
    steps = schedule(N, BATCH, TOTAL)
    touched = np.zeros(p, bool)
    touched[col] = True
    out = {}
    start = None
    for run, wide in (("fp32", 0), ("fp64", 1)):
        t0 = time.time()
        e = engine.Engine(p, **engine_options(case, L, BATCH, state_fp64=wide))
        if start is None:
            e.init_normal(3000 + i, 0.0, 0.05)
            start = e.get_params()          # what the fp32 tables hold: the fp64 run starts from the same values
        else:
            e.set_params(*start)
        ref = _reference(job, case, lambda: oracle_run(case, rp, col, val, y, p, *start, steps))
        before = _counters(L)
        done = e.train(m, TOTAL)
        got = e.get_params()
        r = _errors(got, ref, start, touched)
        r.update(done=int(done), steps=len(steps), counters=[int(x) for x in _counters(L) - before], seconds=time.time() - t0, oracle_seconds=ref["seconds"])
        out[run] = r
        e.close()
    m.close()
    return out


def _run_made_case(job, case, engine, L):
    """Parts B and C: a hand-made matrix stepped batch by batch, the last step truncated; one checkpoint before the last step and one after."""
    prob = ladder_problem(case["regime"], case["values"], case["seed"]) if case["part"] == "B" else side_problem(case["values"], case["seed"])
    p, k = prob["p"], case["k"]
    start = start_params(p, k, case["seed"])
    ref = _reference(job, case, lambda: oracle_run(case, prob["rp"], prob["col"], prob["val"], prob["y"], p, *start, prob["oracle_steps"], prob["ghosts"]))
    touched = np.zeros(p, bool)
    for b0, b1 in prob["oracle_steps"]:
        touched[prob["col"][prob["rp"][b0]:prob["rp"][b1]]] = True
    m = engine.Matrix.from_csr(prob["rp"], prob["col"], prob["val"], p, prob["y"])
    out = {}
    for run, wide in (("fp32", 0), ("fp64", 1)):
        if wide and not job["fp64"]:
            continue
        t0 = time.time()
        e = engine.Engine(p, **engine_options(case, L, prob["batch"], state_fp64=wide))
        e.set_params(*start)
        usable = e.compact_info(m)[2]
        lists0 = e.compact_count(m, 0) if usable else -1
        before = _counters(L)
        ck = [os.path.join(job["ref"], f"{case['name']}.{run}.{i}.ck") for i in (0, 1)]
        for s, (batch, limit) in enumerate(prob["engine_steps"]):
            if s == len(prob["engine_steps"]) - 1 and prob["ghosts"]:
                e.sync()
                e.save(ck[0])
            e.step(m, batch, limit)
        e.sync()
        got = e.get_params()
        e.save(ck[1])
        r = _errors(got, ref, start, touched)
        r.update(counters=[int(x) for x in _counters(L) - before], steps=len(prob["engine_steps"]), sparse=bool(usable), lists0=int(lists0),
                 entries0=int(prob["rp"][prob["batch"]]), state_digest=_file_digest(ck[1]), oracle_ghost_still=ref["ghost_still"], oracle_seconds=ref["seconds"])
        if prob["ghosts"]:
            a, tables = checkpoint_rows(ck[0], prob["ghosts"])
            b, _ = checkpoint_rows(ck[1], prob["ghosts"])
            g = np.asarray(prob["ghosts"])
            scale = float(np.max(np.abs(ref["v"])))
            r.update(tables=int(tables), ghost_still=bool(a == b), ghost_err_v=float(np.max(np.abs(got[2][:, g] - ref["v"][:, g])) / scale),
                     ghost_err_w=float(np.max(np.abs(got[1][g] - ref["w"][g])) / max(float(np.max(np.abs(ref["w"]))), 1e-300)))
        for f in ck:
            if os.path.exists(f):
                os.remove(f)
        r["seconds"] = time.time() - t0
        out[run] = r
        e.close()
    m.close()
    return out


def child_main(path):
    with open(path) as f:
        job = json.load(f)
    from fmwr_amd import _lib as L
    from fmwr_amd import engine
    t0 = time.time()
    results = {}
    for case in job["cases"]:
        results[case["name"]] = (_run_lean_case if case["part"] == "A" else _run_made_case)(job, case, engine, L)
    with open(job["out"], "w") as f:
        json.dump(dict(seconds=time.time() - t0, cases=results), f)
    print("DONE", len(job["cases"]))


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    child_main(sys.argv[1])
