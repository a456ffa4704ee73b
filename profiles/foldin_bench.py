"""fmx_fold_in measured against a torch formulation on the same device (the yardstick only, never the product path) and against the
bound of its row gather.  Writes profiles/foldin.json and appends a section to the one-page profiles/foldin.txt.  Each case records its own number of rounds, so runs
of one k per process (the k = 64 torch side takes minutes per round) are joined with --merge.

Shape: MovieLens-20M -- 138 493 one-hot user columns, 26 744 one-hot item columns, 20 M rows (user, item), item popularity and user
activity drawn from a power law.  EVERY user is folded in one call against the items' rows of an untrained model (V ~ N(0, 0.1)), at
k = 16 and k = 64, for the squared loss and for the logistic loss (8 Newton steps), fp32 tables.
Per case, alternated inside one process after one warm-up call each, --reps rounds (median, [min, max]):
  fold_in   Engine.fold_in(apply = False): find, sort, row pass, Gram, solve, results to the host
  torch     the same solve in fp64 torch: the items' side (fm_embed's sums: base and s of every row, here the item's own w and V row),
            per-group Gram matrices by index_add_ of the rows' outer products (chunked to bound memory), torch.linalg.cholesky +
            cholesky_solve; the Newton loop repeats it
  gate      fold_in faster than torch by more than the spread (max - min) of either side
  bound     bytes of the V rows the row pass must gather / the rate fmx_measure_gather reports for that row size and table size
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU, NI, N = 138_493, 26_744, 20_000_000


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def make_rows(n, seed=3):
    rng = np.random.default_rng(seed)
    pu = rng.pareto(1.2, NU) + 1.0
    pi = rng.pareto(1.0, NI) + 1.0
    users = rng.choice(NU, n, p=pu / pu.sum()).astype(np.uint32)
    items = rng.choice(NI, n, p=pi / pi.sum()).astype(np.uint32)
    return users, items


def torch_fold(torch, users, items, y, w0, w_items, v_items, lam, logistic, steps, chunk):
    """theta [NU][1 + k] in fp64: z = (1, v_item), b = w0 + w_item; Gram by index_add_ of outer products"""
    k = v_items.shape[1]
    D = 1 + k
    theta = torch.zeros((NU, D), dtype=torch.float64, device="cuda")
    eye = torch.diag(torch.full((D,), lam, dtype=torch.float64, device="cuda"))
    for _ in range(steps if logistic else 1):
        H = torch.zeros((NU, D, D), dtype=torch.float64, device="cuda")
        rhs = torch.zeros((NU, D), dtype=torch.float64, device="cuda")
        for c0 in range(0, len(users), chunk):
            u, it, yy = users[c0:c0 + chunk], items[c0:c0 + chunk], y[c0:c0 + chunk]
            z = torch.cat([torch.ones((len(u), 1), dtype=torch.float64, device="cuda"), v_items[it]], dim=1)
            yh = w0 + w_items[it] + (z * theta[u]).sum(1)
            if logistic:
                sg = torch.sigmoid(yy * yh)
                c, d = sg * (1 - sg), yy * (1 - sg)
                H.index_add_(0, u, (z * c[:, None]).unsqueeze(2) * z.unsqueeze(1))
            else:
                d = yy - yh
                H.index_add_(0, u, z.unsqueeze(2) * z.unsqueeze(1))
            rhs.index_add_(0, u, z * d[:, None])
        rhs -= lam * theta
        L = torch.linalg.cholesky(H + eye)
        theta = theta + torch.cholesky_solve(rhs.unsqueeze(2), L).squeeze(2)
    return theta


def run_case(torch, k, logistic, reps, n, only=None):
    from fmwr_amd import _lib as L, engine
    p = NU + NI
    users, items = make_rows(n)
    rng = np.random.default_rng(5)
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32) if logistic else rng.normal(3.5, 1.0, n).astype(np.float32)
    col = np.stack([users, items + NU], 1).ravel().astype(np.uint32)
    m = engine.Matrix.from_csr(np.arange(n + 1, dtype=np.int64) * 2, col, np.ones(2 * n, np.float32), p, y)
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, batch_rows=4096, task=L.TASK_CLASSIFICATION if logistic else L.TASK_REGRESSION)
    e.init_normal(7, 0.0, 0.1)
    w0, w, v = e.get_params()
    ids = np.arange(NU, dtype=np.uint32)
    t_users = torch.tensor(users.astype(np.int64), device="cuda")
    t_items = torch.tensor(items.astype(np.int64), device="cuda")
    t_y = torch.tensor(y.astype(np.float64), device="cuda")
    t_w = torch.tensor(w[NU:], device="cuda", dtype=torch.float64)
    t_v = torch.tensor(v[:, NU:].T.copy(), device="cuda", dtype=torch.float64)
    chunk = max(1, (1 << 28) // ((1 + k) * (1 + k)))   # 2 GiB of outer products at a time
    res = {}

    def fold():
        res["f"] = e.fold_in(m, ids, 0.1, 0.1, newton_steps=8)

    def torch_():
        res["t"] = torch_fold(torch, t_users, t_items, t_y, w0, t_w, t_v, 0.1, logistic, 8, chunk)
        torch.cuda.synchronize()

    versions = {"fold_in": fold, "torch": torch_}
    if only:   # a run under a kernel trace: one version alone, no comparison
        fn = versions[only]
        fn()
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
        out = {"case": f"k={k} {'logistic' if logistic else 'squared'} {only} only", only: _stats(ts)}
        print(json.dumps(out), flush=True)
        return None
    ts = {name: [] for name in versions}
    for fn in versions.values():
        fn()
    for _ in range(reps):
        for name, fn in versions.items():
            t = time.perf_counter(); fn(); ts[name].append(time.perf_counter() - t)
    out = {"case": f"movielens20m k={k} {'logistic x8' if logistic else 'squared'}", "reps": reps, "k": k, "loss": "logistic" if logistic else "squared", "rows": n,
           "groups": NU, "fold_in": _stats(ts["fold_in"]), "torch": _stats(ts["torch"])}
    gw, gv, rows, status = res["f"]
    th = res["t"].cpu().numpy()
    scale = np.maximum(np.abs(th).max(1), 1e-300)
    out["max_rel_diff_vs_torch"] = float((np.abs(np.concatenate([gw[:, None], gv.T], 1) - th).max(1) / scale).max())
    out["status_failed"] = int(status.sum())
    gap = out["torch"]["median_s"] - out["fold_in"]["median_s"]
    spread = max(out["torch"]["max_s"] - out["torch"]["min_s"], out["fold_in"]["max_s"] - out["fold_in"]["min_s"])
    out["ratio_torch_over_fold_in"] = out["torch"]["median_s"] / out["fold_in"]["median_s"]
    out["gate_fold_in_faster_than_torch"] = bool(gap > spread)
    row_bytes = max(k, 4) * 4
    probe = min(row_bytes, 256)
    rate = engine.measure_gather(p * row_bytes, probe) * probe / row_bytes
    out["row_bytes"], out["gather_rows_per_s"], out["bound_s"] = row_bytes, rate, n / rate
    out["fold_in_over_bound"] = out["fold_in"]["median_s"] / out["bound_s"]
    print(json.dumps(out), flush=True)
    return out


def write_txt(rec, path):
    lines = ["", "fmx_fold_in timing record (profiles/foldin_bench.py); medians of alternated calls after one warm-up, [min, max]"]
    for o in rec["cases"]:
        lines.append(f"{o['case']} ({o['reps']} rounds): {o['rows']} rows, {o['groups']} users folded in one call, fp32 tables, V rows of {o['row_bytes']} bytes")
        for name in ("fold_in", "torch"):
            t = o[name]
            lines.append(f"  {name:8s} {t['median_s'] * 1e3:10.1f} ms [{t['min_s'] * 1e3:.1f}, {t['max_s'] * 1e3:.1f}]")
        lines.append(f"  torch / fold_in = {o['ratio_torch_over_fold_in']:.2f}; gate (faster by more than the spread of either side): "
                     f"{'PASS' if o['gate_fold_in_faster_than_torch'] else 'FAIL'}")
        lines.append(f"  row-gather bound {o['bound_s'] * 1e3:.2f} ms ({o['gather_rows_per_s'] / 1e9:.2f} G rows/s measured): fold_in = {o['fold_in_over_bound']:.1f}x bound")
        lines.append(f"  largest difference from the torch result relative to a user's max |theta|: {o['max_rel_diff_vs_torch']:.3g}; unsolved groups: {o['status_failed']}")
    open(path, "a").write("\n".join(lines) + "\n")


def fold_stats(csv_path, label, txt_path):
    """append the kernel shares of a `--only fold_in` run under `rocprofv3 --kernel-trace --stats --output-format csv` to the text record"""
    import csv
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            rows.append((float(r.get("Percentage", 0)), float(r.get("TotalDurationNs", 0)) / 1e6, int(r.get("Calls", 0)), (r.get("Name") or r.get("KernelName") or "")[:100]))
    rows.sort(reverse=True)
    total = sum(r[1] for r in rows)
    lines = ["", f"kernel shares, {label} (rocprofv3 --kernel-trace --stats, fold_in alone: one warm-up call + 2 timed calls; all kernels {total:.1f} ms)"]
    for share, ms, calls, name in rows[:10]:
        lines.append(f"  {share:6.2f} %  {ms:9.2f} ms  {calls:6d} calls  {name}")
    open(txt_path, "a").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--k", default="16,64")
    ap.add_argument("--loss", default="squared,logistic")
    ap.add_argument("--only", default="", help="fold_in or torch: time that version alone and write no record (runs under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--merge", nargs="+", metavar="RECORD_JSON", help="join the records of separate runs (one k per process) into --out and write its text")
    ap.add_argument("--fold", nargs=2, action="append", metavar=("STATS_CSV", "LABEL"), help="append a kernel-stats table to the text record of --out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin.json"))
    args = ap.parse_args()
    if args.fold and not args.merge:
        for csv_path, label in args.fold:
            fold_stats(csv_path, label, args.out.replace(".json", ".txt"))
        return
    if args.merge:
        rec = {"cases": [c for f in args.merge for c in json.load(open(f))["cases"]]}
        json.dump(rec, open(args.out, "w"), indent=1)
        write_txt(rec, args.out.replace(".json", ".txt"))
        for csv_path, label in args.fold or []:
            fold_stats(csv_path, label, args.out.replace(".json", ".txt"))
        return
    import torch
    rec = {"cases": []}
    for k in [int(x) for x in args.k.split(",")]:
        for loss in args.loss.split(","):
            out = run_case(torch, k, loss == "logistic", args.reps, args.rows, args.only)
            if out is not None:
                rec["cases"].append(out)
                json.dump(rec, open(args.out, "w"), indent=1)
    if rec["cases"]:
        write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
