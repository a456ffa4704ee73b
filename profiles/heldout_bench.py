"""fmx_heldout_metrics measured against fmx_topk on the same inputs and against a chunked torch baseline (the yardstick only, never the
product path).  Writes profiles/heldout.json and a one-page profiles/heldout.txt.

  (a) MovieLens-20M-shaped: 138 493 one-hot users x 26 744 one-hot items, k = 64, fp64 (sequential) and fp32 (mini-batch) engines.  Every
      user gets 20 + Pareto(1.2) x 40 positives (at most 3 000, about 20 M in all), drawn without replacement with probability ~ exp(planted
      score) (Gumbel top-n over U W' + b, b = a Zipf popularity).  Held out: one positive per user (leave-one-out), or a 20 % split (at
      least one).  exclude = the training positives.
  (b) 100 000 contexts (25 nnz) x 1 000 000 items (5 nnz), p = 1 M, k = 16, fp32, 10 held-out items per context, no exclusion.
Models: "untrained" = V ~ N(0, 0.1), w = 0 (held-out items land mid-list: the count pass's worst case); "trained" = the planted factors the
positives were drawn from (held-out items near the top, as after training).  At (b) "trained" draws the held-out items among the model's
top 200 items.

Each timed figure is one call (fmx_heldout_metrics with K = 10, 100; fmx_topk_device), ended by a device synchronise: one warm-up call, then
--reps calls; the median and the spread are reported.  The torch baseline forms the same scores with chunked torch.mm, masks the excluded
items, and counts per held-out entry the scores above it (in the engine's precision).  A numpy spot check recomputes sampled ranks from the
engine's parameters (fp64 engines).  Kernel shares come from a separate run of this script under `rocprofv3 --kernel-trace --stats
--output-format csv` (--shape a --prec fp64 --cases loo --reps 1 --no-baseline), folded into the record with --fold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _csr_of(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return rp, (np.concatenate(rows).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32))


def movielens_data(torch, seed=1):
    nu, ni, kf = 138_493, 26_744, 16
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    U = torch.randn(nu, kf, device="cuda", dtype=torch.float64, generator=g) * 0.5
    W = torch.randn(ni, kf, device="cuda", dtype=torch.float64, generator=g) * 0.5
    b = torch.tensor(-1.0 * np.log(np.arange(1, ni + 1)), device="cuda", dtype=torch.float64)[torch.randperm(ni, device="cuda", generator=g)]
    n_u = np.minimum(3000, 20 + (rng.pareto(1.2, nu) * 40).astype(np.int64))
    pos = []
    for c0 in range(0, nu, 4096):
        c1 = min(nu, c0 + 4096)
        S = U[c0:c1] @ W.T + b[None, :]
        gum = -torch.log(-torch.log(torch.rand(S.shape, device="cuda", dtype=torch.float64, generator=g).clamp_min(1e-300)))
        top = torch.topk(S + gum, int(n_u[c0:c1].max()), dim=1).indices.cpu().numpy()
        pos += [top[r, : n_u[c0 + r]] for r in range(c1 - c0)]
    return U, W, b, pos


def split(pos, frac, rng):
    held, train = [], []
    for p in pos:
        q = rng.permutation(p)
        m = 1 if frac is None else max(1, int(round(frac * len(p))))
        held.append(np.sort(q[:m])); train.append(np.sort(q[m:]))
    return held, train


def make_engine(prec, p, k):
    from fmwr_amd import _lib as L, engine
    if prec == "fp64":
        return engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION)
    return engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)


def torch_baseline(torch, prec, base_c, s_c, base_i, s_i, held, train, chunk_elems=1 << 28):
    """ranks by chunked torch.mm + masked counting (strictly greater scores; ties are not split by index here)"""
    dt = torch.float64 if prec == "fp64" else torch.float32
    nc, ni = s_c.shape[0], s_i.shape[0]
    bc, sc, bi, si = base_c.to(dt), s_c.to(dt), base_i.to(dt), s_i.to(dt)
    hrp, hcol = _csr_of(held)
    hrp_t, hcol_t = torch.tensor(hrp, device="cuda"), torch.tensor(hcol.astype(np.int64), device="cuda")
    if train is not None:
        xrp, xcol = _csr_of(train)
        xrp_t, xcol_t = torch.tensor(xrp, device="cuda"), torch.tensor(xcol.astype(np.int64), device="cuda")
    out = torch.empty(len(hcol), dtype=torch.int64, device="cuda")
    rows = max(1, chunk_elems // ni)
    for c0 in range(0, nc, rows):
        c1 = min(nc, c0 + rows)
        S = bc[c0:c1, None] + bi[None, :] + sc[c0:c1] @ si.T
        if train is not None:
            a, z = int(xrp[c0]), int(xrp[c1])
            r = torch.repeat_interleave(torch.arange(c1 - c0, device="cuda"), (xrp_t[c0 + 1:c1 + 1] - xrp_t[c0:c1]))
            S[r, xcol_t[a:z]] = -float("inf")
        a, z = int(hrp[c0]), int(hrp[c1])
        r = torch.repeat_interleave(torch.arange(c1 - c0, device="cuda"), (hrp_t[c0 + 1:c1 + 1] - hrp_t[c0:c1]))
        sh = S[r, hcol_t[a:z]]
        step = max(1, chunk_elems // ni)
        for e0 in range(0, z - a, step):
            e1 = min(z - a, e0 + step)
            out[a + e0:a + e1] = (S[r[e0:e1]] > sh[e0:e1, None]).sum(1)
    return out


def run_case(torch, name, prec, e, mc, mi, held, train, nc, ni, p, k, reps, baseline, proj, spot):
    from fmwr_amd import engine
    hrp, hcol = _csr_of(held)
    mh = engine.Matrix.from_csr(hrp, hcol, np.ones(len(hcol), np.float32), ni)
    mx = None
    if train is not None:
        xrp, xcol = _csr_of(train)
        mx = engine.Matrix.from_csr(xrp, xcol, np.ones(len(xcol), np.float32), ni)
    out = {"case": name, "precision": prec, "n_ctx": nc, "n_items": ni, "p": p, "k": k, "heldout_nnz": int(hrp[-1]),
           "exclude_nnz": 0 if train is None else int(len(xcol))}
    res = {}

    def metrics():
        res["m"] = e.heldout_metrics(mc, mi, mh, [10, 100], exclude=mx)
    out["heldout_metrics"] = _timed(metrics, reps)
    out["metrics"] = dict(zip(["precision@10", "recall@10", "ndcg@10", "hit@10", "precision@100", "recall@100", "ndcg@100", "hit@100", "mrr", "auc"],
                              [float(x) for x in res["m"]["mean"]]))
    for K in (10, 100):
        di = torch.empty((nc, K), dtype=torch.int64, device="cuda")
        ds = torch.empty((nc, K), dtype=torch.float64, device="cuda")

        def topk():
            e.topk_device(mc, 0, nc, mi, K, di.data_ptr(), ds.data_ptr(), exclude=mx)
            e.sync()
        out[f"fmx_topk_K{K}"] = _timed(topk, reps)
        del di, ds
    out["ratio_vs_topk10"] = out["heldout_metrics"]["median_s"] / out["fmx_topk_K10"]["median_s"]
    rank, _ = e.heldout_rank(mc, mi, mh, exclude=mx)
    if baseline:
        bc, sc, bi, si = proj

        def base():
            res["b"] = torch_baseline(torch, prec, bc, sc, bi, si, held, train)
            torch.cuda.synchronize()
        out["torch_baseline"] = _timed(base, max(1, min(reps, 3)))
        b = res["b"].cpu().numpy()
        out["speedup_vs_torch"] = out["torch_baseline"]["median_s"] / out["heldout_metrics"]["median_s"]
        out["torch_rank_mismatches"] = int(np.sum(b != rank))
    if spot is not None:
        out["numpy_spot_check"] = spot(rank, hrp, hcol)
    print(json.dumps(out), flush=True)
    return out


def shape_a(torch, prec, reps, baseline, cases):
    from fmwr_amd import engine
    nu, ni, k = 138_493, 26_744, 64
    p = nu + ni
    U, W, b, pos = movielens_data(torch)
    rng = np.random.default_rng(5)
    mc = engine.Matrix.from_csr(np.arange(nu + 1, dtype=np.int64), np.arange(nu, dtype=np.uint32), np.ones(nu, np.float32), p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64), np.arange(nu, nu + ni, dtype=np.uint32), np.ones(ni, np.float32), p)
    e = make_engine(prec, p, k)
    outs = []
    for model in ("untrained", "trained"):
        if model == "untrained":
            e.init_normal(7, 0.0, 0.1)
        else:  # planted: user factors and a bias column; the item bias as w
            v = np.zeros((k, p))
            v[:16, :nu] = U.cpu().numpy().T
            v[:16, nu:] = W.cpu().numpy().T
            w = np.zeros(p)
            w[nu:] = b.cpu().numpy()
            e.set_params(0.0, w, v)
        w0, w, v = e.get_params()
        bc = torch.tensor(w0 + w[:nu], device="cuda"); sc = torch.tensor(v[:, :nu].T.copy(), device="cuda")
        bi = torch.tensor(w[nu:], device="cuda"); si = torch.tensor(v[:, nu:].T.copy(), device="cuda")
        for split_name, frac in (("loo", None), ("split20", 0.2)):
            if split_name not in cases:
                continue
            held, train = split(pos, frac, rng)
            Vc, Vi = v[:, :nu], v[:, nu:]
            def spot(rank, hrp, hcol, held=held, train=train):
                pick = np.random.default_rng(3).choice(len(hcol), 200, replace=False)
                rows = np.searchsorted(hrp, pick, side="right") - 1
                bad = 0
                for q, c in zip(pick, rows):
                    s = (w0 + w[c]) + w[nu:] + Vc[:, c] @ Vi
                    h = int(hcol[q])
                    ok = np.ones(ni, bool); ok[train[c]] = False; ok[h] = False
                    r = int(np.sum(ok & ((s > s[h]) | ((s == s[h]) & (np.arange(ni) < h)))))
                    bad += int(r != rank[q])
                return {"sampled": 200, "mismatches": bad}
            outs.append(run_case(torch, f"a_movielens20m_{split_name}_{model}", prec, e, mc, mi, held, train, nu, ni, p, k, reps, baseline,
                                 (bc, sc, bi, si), spot if prec == "fp64" else None))
    return outs


def shape_b(torch, reps, baseline):
    from fmwr_amd import engine
    nc, ni, p, k = 100_000, 1_000_000, 1_000_000, 16
    rng = np.random.default_rng(2)
    ccol = np.sort(rng.integers(0, p, (nc, 25)), axis=1).astype(np.uint32).ravel()
    icol = np.sort(rng.integers(0, p, (ni, 5)), axis=1).astype(np.uint32).ravel()
    cval = rng.uniform(0.5, 1.5, nc * 25).astype(np.float32)
    ival = rng.uniform(0.5, 1.5, ni * 5).astype(np.float32)
    mc = engine.Matrix.from_csr(np.arange(nc + 1, dtype=np.int64) * 25, ccol, cval, p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64) * 5, icol, ival, p)
    e = make_engine("fp32", p, k)
    e.init_normal(7, 0.0, 0.1)
    outs = []
    # the baseline's projections: base and s of every row with torch, from the engine's parameters
    w0, w, v = e.get_params()
    vt = torch.tensor(v.T.copy(), device="cuda", dtype=torch.float64)
    wt = torch.tensor(w, device="cuda", dtype=torch.float64)

    def proj(m_col, m_val, n, nnz):
        col = torch.tensor(m_col.astype(np.int64), device="cuda").view(n, nnz)
        val = torch.tensor(m_val.astype(np.float64), device="cuda").view(n, nnz)
        s = torch.einsum("rz,rzf->rf", val, vt[col])
        base = (val * wt[col]).sum(1) + 0.5 * ((s * s).sum(1) - torch.einsum("rz,rzf->r", val * val, vt[col] ** 2))
        return base, s
    bc, sc = proj(ccol, cval, nc, 25)
    bi, si = proj(icol, ival, ni, 5)
    bc = bc + w0
    for model in ("untrained", "trained"):
        if model == "untrained":
            held = [np.sort(rng.choice(ni, 10, replace=False)) for _ in range(nc)]
        else:  # held-out items among each context's 200 best items: what a trained model's held-out items look like
            idx, _ = e.topk(mc, mi, 200)
            held = [np.sort(idx[c, rng.choice(200, 10, replace=False)]) for c in range(nc)]
        outs.append(run_case(torch, f"b_100k_x_1m_{model}", "fp32", e, mc, mi, held, None, nc, ni, p, k, reps, baseline, (bc, sc, bi, si), None))
    return outs


def write_txt(rec, path):
    lines = ["fmx_heldout_metrics record (profiles/heldout_bench.py); times: median of %d calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        hm = o["heldout_metrics"]
        lines.append(f"{o['case']} {o['precision']}: {o['n_ctx']} x {o['n_items']}, k {o['k']}, held-out {o['heldout_nnz']}, excluded {o['exclude_nnz']}")
        lines.append(f"  heldout_metrics {hm['median_s'] * 1e3:9.2f} ms [{hm['min_s'] * 1e3:.2f}, {hm['max_s'] * 1e3:.2f}]   "
                     f"= {o['ratio_vs_topk10']:.2f}x fmx_topk(K=10) {o['fmx_topk_K10']['median_s'] * 1e3:.2f} ms; fmx_topk(K=100) "
                     f"{o['fmx_topk_K100']['median_s'] * 1e3:.2f} ms")
        if "torch_baseline" in o:
            lines.append(f"  torch baseline  {o['torch_baseline']['median_s'] * 1e3:9.2f} ms  -> {o['speedup_vs_torch']:.2f}x; rank mismatches "
                         f"{o['torch_rank_mismatches']} (ties split by index here, not there)")
        if "numpy_spot_check" in o:
            lines.append(f"  numpy spot check: {o['numpy_spot_check']['mismatches']} of {o['numpy_spot_check']['sampled']} sampled ranks differ")
        m = o["metrics"]
        lines.append(f"  recall@10 {m['recall@10']:.4f}  ndcg@10 {m['ndcg@10']:.4f}  mrr {m['mrr']:.4f}  auc {m['auc']:.4f}")
    if rec.get("kernel_stats"):
        lines += ["", "kernel shares (rocprofv3 --kernel-trace --stats, separate run): " + rec["kernel_stats"].get("run", "")]
        for row in rec["kernel_stats"]["rows"]:
            lines.append(f"  {row['share']:6.2f} %  {row['total_ms']:9.2f} ms  {row['name']}")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")


def fold_stats(csv_path, run):
    import csv
    rows = []
    with open(csv_path) as f:
        for r in csv.DictReader(f):
            name = r.get("Name") or r.get("KernelName") or ""
            rows.append({"name": name[:90], "total_ms": float(r.get("TotalDurationNs", 0)) / 1e6, "share": float(r.get("Percentage", 0))})
    rows.sort(key=lambda x: -x["share"])
    return {"run": run, "rows": rows[:12]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["all", "a", "b"])
    ap.add_argument("--prec", default="both", choices=["both", "fp64", "fp32"])
    ap.add_argument("--cases", default="loo,split20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heldout.json"))
    ap.add_argument("--fold", nargs=3, metavar=("RECORD_JSON", "STATS_CSV", "RUN"), help="add kernel shares to a record and rewrite its .txt")
    args = ap.parse_args()
    if args.fold:
        rec = json.load(open(args.fold[0]))
        rec["kernel_stats"] = fold_stats(args.fold[1], args.fold[2])
        json.dump(rec, open(args.fold[0], "w"), indent=1)
        write_txt(rec, args.fold[0].replace(".json", ".txt"))
        return
    import torch
    rec = {"reps": args.reps, "cases": []}
    if args.shape in ("all", "a"):
        for prec in (["fp64", "fp32"] if args.prec == "both" else [args.prec]):
            rec["cases"] += shape_a(torch, prec, args.reps, not args.no_baseline, args.cases.split(","))
    if args.shape in ("all", "b"):
        rec["cases"] += shape_b(torch, args.reps, not args.no_baseline)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
