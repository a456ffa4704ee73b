"""The host forms of three query entry points timed under two builds of libfmx.so (FMX_LIB_PATH), for the record in
profiles/query_refactor.txt: the entry points moved into fmx_query.hip onto one staging helper, and the host forms are where that shows.

  topk          fmx_topk, 100 000 contexts x 100 000 items, K = 100, k = 16
  interactions  fmx_interactions, 1 M rows x 30 entries, top_m = 5, k = 16
  project       fmx_project, 1 M rows x 30 entries, k = 16

    python profiles/query_refactor_bench.py --before <parent's libfmx.so> [--after <libfmx.so>] [--rounds 5]
Every round starts one fresh child process per build, the two alternated; a child builds the matrices, calls each host form once to warm up and
once timed.  Per build and shape: the median of the rounds and the spread [min, max].  No threshold: the expectation is "equal within the
larger of the two spreads"."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = ["topk", "interactions", "project"]


def child():
    from fmwr_amd import _lib as L, engine
    p, k = 1_000_000, 16
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    ctx = engine.Matrix.synthetic(100_000, p, 30, 3)
    items = engine.Matrix.synthetic(100_000, p, 30, 5)
    rows = engine.Matrix.synthetic(1_000_000, p, 30, 11).synthetic_values(12)
    calls = {"topk": lambda: e.topk(ctx, items, 100), "interactions": lambda: e.interactions(rows, 5), "project": lambda: e.project(rows)}
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
    print(f"host forms, seconds: median of {args.rounds} fresh processes per build, alternated [min, max]")
    for s in SHAPES:
        st = {b: sorted(ts[b][s]) for b in libs}
        med = {b: st[b][len(st[b]) // 2] for b in libs}
        spread = max(st[b][-1] - st[b][0] for b in libs)
        verdict = "equal within the larger spread" if abs(med["after"] - med["before"]) <= spread else ("after is slower" if med["after"] > med["before"] else "after is faster")
        print(f"  {s:13s} before {med['before']:.4f} [{st['before'][0]:.4f}, {st['before'][-1]:.4f}]   after {med['after']:.4f} "
              f"[{st['after'][0]:.4f}, {st['after'][-1]:.4f}]   {verdict}")


if __name__ == "__main__":
    main()
