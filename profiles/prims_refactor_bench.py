"""The host paths that moved onto fm_prims.hip's sorts and scans, timed under two builds of libfmx.so (FMX_LIB_PATH), for the record in
profiles/prims_refactor.txt.  One call each, at the shapes of the features' own bench scripts scaled to run in seconds:

  pairs     fmx_matrix_pairs (uniform negatives), 100 000 users x 20 000 items one-hot, 2 M positives, n_neg = 1       (rank_bench.py, shape a)
  heldout   fmx_heldout_rank, 20 000 users x 10 000 items, 5 held-out items per user, k = 16                           (heldout_bench.py, shape a)
  lists     fmx_rank_lists, 2 000 contexts x lists of 1 500 candidates: above 1 024 entries, the general path          (lists_bench.py)
  metrics   fmx_metrics grouped, 2 M rows in 500 groups of about 4 000 rows: the global form of the pair count         (metrics_bench.py, grouped)
  split     fmx_split_assign WITHIN_GROUPS (5 folds, 50 000 groups) and fmx_matrix_take of fold 0's complement, 2 M rows x 10 entries
  foldin    fmx_fold_in, 1 M rows (user, item), the 50 000 users folded in, k = 16, squared loss                       (foldin_bench.py)

    python profiles/prims_refactor_bench.py --before <parent's libfmx.so> [--after <libfmx.so>] [--rounds 5]
Every round starts one fresh child process per build, the two alternated; a child builds its inputs, calls each path once to warm up and once
timed.  Per build and path: the median of the rounds and the spread [min, max].  No threshold: the expectation is "equal within the larger of
the two spreads"."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ["pairs", "heldout", "lists", "metrics", "split", "foldin"]


def _onehot(engine, n, first, p):
    return engine.Matrix.from_csr(np.arange(n + 1, dtype=np.int64), np.arange(first, first + n, dtype=np.uint32), np.ones(n, np.float32), p)


def _rows_of(engine, n_rows, per_row, n_cols, rng):
    """n_rows rows of per_row column ids below n_cols each (repeats inside a row allowed: the pipelines make them distinct)"""
    col = rng.integers(0, n_cols, n_rows * per_row).astype(np.uint32)
    return engine.Matrix.from_csr(np.arange(n_rows + 1, dtype=np.int64) * per_row, col, np.ones(len(col), np.float32), n_cols)


def child():
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(17)
    calls = {}

    users, items, k = 100_000, 20_000, 16
    C_, I_ = _onehot(engine, users, 0, users + items), _onehot(engine, items, users, users + items)
    X = _rows_of(engine, users, 20, items, rng)
    calls["pairs"] = lambda: engine.Matrix.pairs(C_, I_, X, 1, 77, 3)

    hu, hi = 20_000, 10_000
    e = engine.Engine(hu + hi, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    hc, hit = _onehot(engine, hu, 0, hu + hi), _onehot(engine, hi, hu, hu + hi)
    held = _rows_of(engine, hu, 5, hi, rng)
    calls["heldout"] = lambda: e.heldout_rank(hc, hit, held)

    lc = _onehot(engine, 2_000, 0, hu + hi)
    lists = _rows_of(engine, 2_000, 1_500, hi, rng)
    calls["lists"] = lambda: e.rank_lists(lc, hit, lists)

    n, G = 2_000_000, 500
    grp = rng.integers(0, G, n).astype(np.uint32)
    col = np.stack([rng.integers(0, hu, n), hu + rng.integers(0, hi, n)], 1).ravel().astype(np.uint32)
    m = engine.Matrix.from_csr(np.arange(0, 2 * n + 1, 2, dtype=np.int64), col, np.ones(2 * n, np.float32), hu + hi,
                               np.where(rng.random(n) < 0.25, 1.0, -1.0).astype(np.float32))
    ec = engine.Engine(hu + hi, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_CLASSIFICATION, batch_rows=4096)
    ec.init_normal(7, 0.0, 0.1)
    calls["metrics"] = lambda: ec.metrics(m, grp, G)

    sm = engine.Matrix.synthetic(n, 1_000_000, 10, 5)
    sg = rng.integers(0, 50_000, n).astype(np.uint32)

    def split():
        part = engine.split_assign(n, sg, 50_000, scope=L.SPLIT_WITHIN_GROUPS, n_folds=5, seed=9)
        return sm.take(np.flatnonzero(part != 0))
    calls["split"] = split

    fu, fi, fn = 50_000, 5_000, 1_000_000
    fcol = np.stack([rng.integers(0, fu, fn), fu + rng.integers(0, fi, fn)], 1).ravel().astype(np.uint32)
    fm = engine.Matrix.from_csr(np.arange(fn + 1, dtype=np.int64) * 2, fcol, np.ones(2 * fn, np.float32), fu + fi, rng.normal(3.5, 1.0, fn).astype(np.float32))
    ef = engine.Engine(fu + fi, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    ef.init_normal(7, 0.0, 0.1)
    ids = np.arange(fu, dtype=np.uint32)
    calls["foldin"] = lambda: ef.fold_in(fm, ids, 0.1, 0.1)

    out = {}
    for name in SHAPES:
        calls[name]()
        t = time.perf_counter()
        calls[name]()
        out[name] = time.perf_counter() - t
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--before", help="the parent commit's libfmx.so")
    ap.add_argument("--after", default=os.path.join(ROOT, "fmwr_amd", "libfmx.so"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if args.child:
        return child()
    libs = {"before": os.path.abspath(args.before), "after": os.path.abspath(args.after)}
    ts = {b: {s: [] for s in SHAPES} for b in libs}
    for _ in range(args.rounds):
        for b, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, FMX_LIB_PATH=path), capture_output=True,
                               text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"the child for {b} ended with {r.returncode}:\n{r.stdout}\n{r.stderr}")   # nothing more is started
            res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            for s in SHAPES:
                ts[b][s].append(res[s])
    print(f"moved host paths, seconds: median of {args.rounds} fresh processes per build, alternated [min, max]")
    for s in SHAPES:
        st = {b: sorted(ts[b][s]) for b in libs}
        med = {b: st[b][len(st[b]) // 2] for b in libs}
        spread = max(st[b][-1] - st[b][0] for b in libs)
        verdict = "equal within the larger spread" if abs(med["after"] - med["before"]) <= spread else ("after is slower" if med["after"] > med["before"] else "after is faster")
        print(f"  {s:8s} before {med['before']:.4f} [{st['before'][0]:.4f}, {st['before'][-1]:.4f}]   after {med['after']:.4f} "
              f"[{st['after'][0]:.4f}, {st['after'][-1]:.4f}]   {verdict}", flush=True)


if __name__ == "__main__":
    main()
