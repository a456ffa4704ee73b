"""fmx_topk measured at two shapes against a chunked torch.mm + torch.topk baseline in the same precision (the yardstick only, never
the product path).  Writes profiles/topk_r07.json and a one-page profiles/topk_r07.txt.

  (a) MovieLens-20M-shaped: 138 493 one-hot users x 26 744 one-hot items, k = 64, K = 100, fp64 (sequential) and fp32 (mini-batch) engines
  (b) 100 000 contexts (25 nnz) x 1 000 000 items (5 nnz), p = 1 M, k = 16, K = 100, fp32

Each timed figure is fmx_topk_device over all contexts, ended by a device synchronise: one warm-up call, then --reps calls; the median
and the spread (min, max) are reported.  The kernel split (projection / score+select / merge) comes from a separate run of this script
under `rocprofv3 --kernel-trace --stats` (--shape b --reps 1 --no-baseline); pass its results database with --kernel-stats to put it into
the record (or fold it into an existing record with --fold).  Dot-product peak: 2k flop per score against 157.3 TF (fp32) / 78.6 TF (fp64).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF = {"fp32": 157.3, "fp64": 78.6}


def _synthetic(n, lo, hi, nnz, seed, one_hot=False):
    rng = np.random.default_rng(seed)
    col = np.sort(rng.integers(lo, hi, (n, nnz)), axis=1).astype(np.uint32).ravel() if not one_hot else np.arange(lo, lo + n, dtype=np.uint32)
    val = np.ones(len(col), np.float32) if one_hot else rng.uniform(0.5, 1.5, n * nnz).astype(np.float32)
    return np.arange(n + 1, dtype=np.int64) * (1 if one_hot else nnz), col, val


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def run_shape(name, prec, nc, ni, p, k, K, C_csr, I_csr, reps, baseline, torch):
    from fmwr_amd import _lib as L, engine
    if prec == "fp64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    mc = engine.Matrix.from_csr(*C_csr, p)
    mi = engine.Matrix.from_csr(*I_csr, p)
    di = torch.empty((nc, K), dtype=torch.int64, device="cuda")
    ds = torch.empty((nc, K), dtype=torch.float64, device="cuda")

    def call():
        e.topk_device(mc, 0, nc, mi, K, di.data_ptr(), ds.data_ptr())
        e.sync()

    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
    st = _stats(ts)
    scores = nc * ni
    rate = scores / st["median_s"]
    out = {"shape": name, "precision": prec, "n_ctx": nc, "n_items": ni, "p": p, "k": k, "K": K, "fmx_topk": st,
           "scores_per_s": rate, "dot_peak_fraction": rate * 2 * k / (PEAK_TF[prec] * 1e12)}
    if baseline:
        out["torch_baseline"] = torch_baseline(e, mc, mi, C_csr, I_csr, p, k, K, prec, reps, torch)
        out["speedup_vs_torch"] = out["torch_baseline"]["median_s"] / st["median_s"]
        # the two agree on the selected scores (the baseline's dot is torch's own summation order)
        ref_i, ref_s = out["torch_baseline"].pop("_first_rows")
        got = ds[: ref_s.shape[0]].cpu().numpy()
        out["max_abs_score_diff_first_rows"] = float(np.max(np.abs(got - ref_s)))
    print(json.dumps({k_: v for k_, v in out.items()}), flush=True)
    return out


def torch_baseline(e, mc, mi, C_csr, I_csr, p, k, K, prec, reps, torch):
    """base and s from the engine's own projection (fmx_predict of each row, the factor sums by a sparse product on the host), then
    per chunk of contexts: scores = base_c + base_i + S_c S_i^T by torch.mm, torch.topk along the items"""
    dt = torch.float64 if prec == "fp64" else torch.float32
    w0, w, v = e.get_params()
    import scipy.sparse as sp
    Ac = sp.csr_matrix((C_csr[2].astype(np.float64), C_csr[1], C_csr[0]), shape=(len(C_csr[0]) - 1, p))
    Ai = sp.csr_matrix((I_csr[2].astype(np.float64), I_csr[1], I_csr[0]), shape=(len(I_csr[0]) - 1, p))
    Sc, Si = Ac @ v.T, Ai @ v.T
    bc = e.predict(mc)
    bi = e.predict(mi) - w0
    Sc_d = torch.from_numpy(np.ascontiguousarray(Sc)).to("cuda", dt)
    Si_d = torch.from_numpy(np.ascontiguousarray(Si)).to("cuda", dt)
    bc_d = torch.from_numpy(bc).to("cuda", dt)
    bi_d = torch.from_numpy(bi).to("cuda", dt)
    nc, ni = Sc.shape[0], Si.shape[0]
    chunk = max(1, (1 << 31) // (ni * (8 if prec == "fp64" else 4)))  # a 2 GB score block per chunk
    oi = torch.empty((nc, K), dtype=torch.int64, device="cuda")
    os_ = torch.empty((nc, K), dtype=dt, device="cuda")

    def call():
        for c0 in range(0, nc, chunk):
            c1 = min(nc, c0 + chunk)
            sc = torch.addmm(bi_d.unsqueeze(0).expand(c1 - c0, ni), Sc_d[c0:c1], Si_d.T).add_(bc_d[c0:c1].unsqueeze(1))
            s, i = torch.topk(sc, K, dim=1)
            os_[c0:c1] = s; oi[c0:c1] = i
        torch.cuda.synchronize()

    call()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); call(); ts.append(time.perf_counter() - t)
    st = _stats(ts)
    st["chunk_rows"] = chunk
    st["_first_rows"] = (oi[:16].cpu().numpy(), os_[:16].double().cpu().numpy())
    return st


def kernel_split(path, calls):
    """rocprofv3 results database (--kernel-trace) -> ms per stage and per call"""
    import sqlite3
    stages = {"projection": 0.0, "score_select": 0.0, "merge": 0.0}
    for name, ns in sqlite3.connect(path).execute("select name, duration from kernels"):
        if "topk_score_k" in name:
            stages["score_select"] += ns / 1e6 / calls
        elif "topk_merge_k" in name:
            stages["merge"] += ns / 1e6 / calls
        elif "rows_forward" in name or "topk_pack_k" in name or "topk_sort_excl_k" in name:
            stages["projection"] += ns / 1e6 / calls
    return stages


def write_record(rec, out):
    with open(out + ".json", "w") as f:
        json.dump(rec, f, indent=1)
    lines = ["fmx_topk record (profiles/topk_bench.py); times: median of %d calls after one warm-up, [min, max]" % rec["reps"], ""]
    for r in rec["runs"]:
        t = r["fmx_topk"]
        lines.append(f"{r['shape']} {r['precision']}: {r['n_ctx']} x {r['n_items']}, k {r['k']}, K {r['K']}")
        lines.append(f"  fmx_topk  {t['median_s'] * 1e3:9.2f} ms [{t['min_s'] * 1e3:.2f}, {t['max_s'] * 1e3:.2f}]  {r['scores_per_s'] / 1e9:8.1f} G scores/s"
                     f"  {100 * r['dot_peak_fraction']:.1f} % of the dot-product peak")
        if "torch_baseline" in r:
            b = r["torch_baseline"]
            lines.append(f"  torch     {b['median_s'] * 1e3:9.2f} ms [{b['min_s'] * 1e3:.2f}, {b['max_s'] * 1e3:.2f}]  (mm + topk, {b['chunk_rows']} rows per chunk)"
                         f"  -> fmx_topk {r['speedup_vs_torch']:.2f}x;  max |score diff| first rows {r['max_abs_score_diff_first_rows']:.2e}")
    if "kernel_ms_shape_b_per_call" in rec:
        lines += ["", "kernel time per shape-(b) call (rocprofv3 --kernel-trace, separate run): " +
                  ", ".join(f"{k_} {v:.2f} ms" for k_, v in rec["kernel_ms_shape_b_per_call"].items())]
    lines += [""] + rec.get("notes", [])
    with open(out + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["a", "b", "all"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 results database of a separate run (--shape b --reps 1 --no-baseline), folded in")
    ap.add_argument("--profiled-calls", type=int, default=2, help="fmx_topk calls in that run (warm-up included)")
    ap.add_argument("--fold", default=None, help="an earlier record (.json): add --kernel-stats and --note lines to it, run nothing")
    ap.add_argument("--note", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_r07"))
    args = ap.parse_args()
    if args.fold:
        rec = json.load(open(args.fold))
        if args.kernel_stats:
            rec["kernel_ms_shape_b_per_call"] = kernel_split(args.kernel_stats, args.profiled_calls)
        rec["notes"] = rec.get("notes", []) + args.note
        write_record(rec, args.out)
        return
    import torch
    torch.cuda.init()  # before libfmx: the same process
    sys.path.insert(0, ROOT)
    rec = {"script": "profiles/topk_bench.py", "reps": args.reps, "runs": []}
    if args.shape in ("a", "all"):
        users, items = 138_493, 26_744
        p = users + items
        Cm = _synthetic(users, 0, users, 1, 0, one_hot=True)
        Im = _synthetic(items, users, p, 1, 0, one_hot=True)
        for prec in ("fp64", "fp32"):
            rec["runs"].append(run_shape("a_movielens20m", prec, users, items, p, 64, 100, Cm, Im, args.reps, not args.no_baseline, torch))
    if args.shape in ("b", "all"):
        p = 1_000_000
        Cm = _synthetic(100_000, 0, p, 25, 1)
        Im = _synthetic(1_000_000, 0, p, 5, 2)
        rec["runs"].append(run_shape("b_100k_x_1m", "fp32", 100_000, 1_000_000, p, 16, 100, Cm, Im, args.reps, not args.no_baseline, torch))
    if args.kernel_stats:
        rec["kernel_ms_shape_b_per_call"] = kernel_split(args.kernel_stats, args.profiled_calls)
    write_record(rec, args.out)


if __name__ == "__main__":
    main()
