"""fmx_contrib measured at two shapes against fmx_predict on the same rows and against the same formula in torch on the same device (the
yardstick only, never the product path).  Writes profiles/contrib.json and a one-page profiles/contrib.txt.

  (a) configs[1]'s matrix: 10 M rows x 1 M features, 30 nnz per row (uniform columns, values in (0, 1)), k = 16; fp32 mini-batch tables and
      the fp64 form (sequential engine)
  (b) MovieLens-20M-shaped one-hot rows: 20 M ratings of (user, item), 138 493 users + 26 744 items, k = 64; fp32 and fp64

Each timed figure ends with a device synchronise: one warm-up call, then --reps calls; the median and the spread (min, max) are reported.
  contrib   fmx_contrib_device over all rows into a torch buffer
  predict   fmx_predict_device over the same rows (link NONE)
  torch     per chunk of rows: T = V[col] * x (index_select), s = index_add_ of T over the rows, phi = x w[col] + 1/2 sum_f T (s[row] - T), fp64
  summary   fmx_contrib_summary (contributions, per-chunk sort and reduce-by-key, p-long sums copied to the host)
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--reps 1 --no-baseline); its stats CSV goes into the
record with --kernel-stats.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def _timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return _stats(ts)


def _engine(prec, p, k):
    from fmwr_amd import _lib as L, engine
    if prec == "fp64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    rng = np.random.default_rng(7)
    e.set_params(0.1, rng.normal(0, 0.1, p), rng.normal(0, 0.1, (k, p)))
    return e


def _matrix(shape, n_scale):
    from fmwr_amd import engine
    if shape == "a_configs1":
        n, p = int(10_000_000 * n_scale), 1_000_000
        return engine.Matrix.synthetic(n, p, 30, 11).synthetic_values(12), n, p, 16
    users, items = 138_493, 26_744
    n = int(20_000_263 * n_scale)
    rng = np.random.default_rng(3)
    col = np.stack([rng.integers(0, users, n), users + rng.integers(0, items, n)], 1).ravel().astype(np.uint32)
    m = engine.Matrix.from_csr(np.arange(0, 2 * n + 1, 2, dtype=np.int64), col, np.ones(2 * n, np.float32), users + items)
    return m, n, users + items, 64


def torch_baseline(e, m, reps, torch, chunk_rows=1 << 20):
    w0, w, v = e.get_params()
    V = torch.from_numpy(np.ascontiguousarray(v.T)).cuda()      # [p][k] fp64
    W = torch.from_numpy(w).cuda()
    rp, col, val, _ = m.export()
    rp_d = torch.from_numpy(rp).cuda()
    col_d = torch.from_numpy(col.astype(np.int64)).cuda()
    val_d = torch.from_numpy(val).cuda().double()
    out = torch.empty(len(col), dtype=torch.float64, device="cuda")
    lens = (rp_d[1:] - rp_d[:-1])

    def call():
        for r0 in range(0, m.n, chunk_rows):
            r1 = min(m.n, r0 + chunk_rows)
            a, b = int(rp[r0]), int(rp[r1])
            c, x = col_d[a:b], val_d[a:b]
            row = torch.repeat_interleave(torch.arange(r1 - r0, device="cuda"), lens[r0:r1])
            T = torch.index_select(V, 0, c) * x[:, None]
            S = torch.zeros((r1 - r0, V.shape[1]), dtype=torch.float64, device="cuda").index_add_(0, row, T)
            out[a:b] = x * torch.index_select(W, 0, c) + 0.5 * (T * (torch.index_select(S, 0, row) - T)).sum(1)
        torch.cuda.synchronize()

    st = _timed(call, reps)
    return st, out


def run(shape, prec, reps, baseline, n_scale, torch):
    from fmwr_amd import _lib as L
    m, n, p, k = _matrix(shape, n_scale)
    e = _engine(prec, p, k)
    phi = torch.empty(m.nnz, dtype=torch.float64, device="cuda")
    yh = torch.empty(n, dtype=torch.float64, device="cuda")

    def contrib():
        e.contrib_device(m, 0, n, phi.data_ptr()); e.sync()

    def predict():
        L.check(L.lib().fmx_predict_device(e.h, m.h, 0, n, __import__("ctypes").c_void_p(yh.data_ptr()), L.LINK_NONE)); e.sync()

    out = {"shape": shape, "precision": prec, "rows": n, "nnz": m.nnz, "p": p, "k": k}
    out["contrib"] = _timed(contrib, reps)
    out["predict"] = _timed(predict, reps)
    out["contrib_over_predict"] = out["contrib"]["median_s"] / out["predict"]["median_s"]
    out["contrib_entries_per_s"] = m.nnz / out["contrib"]["median_s"]
    out["summary"] = _timed(lambda: e.contrib_summary(m), max(1, reps // 2))
    if baseline:
        st, ref = torch_baseline(e, m, reps, torch)
        out["torch"] = st
        out["contrib_speedup_vs_torch"] = st["median_s"] / out["contrib"]["median_s"]
        out["max_abs_diff_vs_torch"] = float((phi - ref).abs().max().item())
        del ref
    print(json.dumps(out), flush=True)
    return out


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            rows.append({"kernel": r["Name"][:120], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                         "avg_us": float(r["AverageNs"]) / 1e3, "percent": float(r["Percentage"])})
    return rows


def write_text(res, stats, path):
    lines = [f"fmx_contrib record (profiles/contrib_bench.py); times: median of {res[0]['contrib']['reps']} calls after one warm-up, [min, max]", ""]
    ms = lambda s: f"{1e3 * s['median_s']:9.2f} ms [{1e3 * s['min_s']:.2f}, {1e3 * s['max_s']:.2f}]"  # noqa: E731
    for r in res:
        lines.append(f"{r['shape']} {r['precision']}: {r['rows']} rows, {r['nnz']} entries, p {r['p']}, k {r['k']}")
        lines.append(f"  contrib  {ms(r['contrib'])}   {r['contrib_entries_per_s'] / 1e9:.2f} G entries/s")
        lines.append(f"  predict  {ms(r['predict'])}   -> contrib / predict {r['contrib_over_predict']:.2f}x")
        if "torch" in r:
            lines.append(f"  torch    {ms(r['torch'])}   -> contrib {r['contrib_speedup_vs_torch']:.2f}x faster;  max |phi diff| {r['max_abs_diff_vs_torch']:.2e}")
        lines.append(f"  summary  {ms(r['summary'])}")
    if stats:
        lines += ["", "kernels (rocprofv3 --kernel-trace --stats, separate run, every shape once):"]
        for s in stats[:12]:
            lines.append(f"  {s['percent']:5.1f} %  {s['calls']:6d} calls  {s['avg_us']:10.1f} us avg  {s['kernel'][:90]}")
    open(path, "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape", choices=["a", "b", "all"], default="all")
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows (quick checks)")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv to fold into the record")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contrib"))
    a = ap.parse_args()
    import torch
    jobs = []
    if a.shape in ("a", "all"):
        jobs += [("a_configs1", "fp32"), ("a_configs1", "fp64")]
    if a.shape in ("b", "all"):
        jobs += [("b_movielens20m", "fp32"), ("b_movielens20m", "fp64")]
    res = [run(s, prec, a.reps, not a.no_baseline, a.n_scale, torch) for s, prec in jobs]
    stats = kernel_stats(a.kernel_stats) if a.kernel_stats else None
    if a.out:
        json.dump({"results": res, "kernel_stats": stats}, open(a.out + ".json", "w"), indent=1)
        write_text(res, stats, a.out + ".txt")


if __name__ == "__main__":
    main()
