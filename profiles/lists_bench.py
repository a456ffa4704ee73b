"""fmx_rank_lists_device measured against the only earlier way to the same scores (fmx_heldout_rank with the lists as "held-out" items),
against a torch formulation on the same projections (the yardstick only, never the product path) and against the shape bound of the row
gather.  Writes profiles/lists.json and a one-page profiles/lists.txt.

Shapes (the matrices and the untrained model of profiles/heldout_bench.py):
  A   MovieLens-20M-shaped: 138 493 one-hot users x 26 744 one-hot items, k = 64, fp32 (mini-batch) and fp64 (sequential) engines;
      lists of (i) 100 candidates per context -- one "held-out" item plus 99 uniform draws, the sampled-evaluation protocol (every draw is
      uniform here: which item is the held-out one does not change the work) -- and (ii) 1 000 uniform candidates;
  B   100 000 contexts (25 nnz) x 1 000 000 items (5 nnz), p = 1 M, k = 16, fp32, 500 uniform candidates per context.
Per shape, alternated inside one process after one warm-up call each, --reps rounds (median, [min, max]):
  lists     fmx_rank_lists_device, scores + positions (the fused LDS path: every list fits it)
  general   the same call with the test hook forcing every list through the general (radix sort) path
  heldout   fmx_heldout_rank_device(heldout = lists): the parent's way (it also counts every item against every context)
  torch     gather of the candidates' projected rows, batched dot, per-list sort and inverse permutation, chunked to bound memory;
            the projections are made beforehand and not timed
  gate      recorded per shape: lists faster than heldout, and than torch, by more than the spread (max - min) of either side
  bound     bytes of the gathered s rows / the rate fmx_measure_gather reports for that row size and table size on the same device
            (it takes rows of at most 256 bytes: the 512-byte rows of fp64 at k = 64 are priced at the byte rate of 256-byte rows)
Every shape may run in a process of its own (--shape, --prec, --out) and the records be joined with --merge.  Kernel shares come from a
separate run under `rocprofv3 --kernel-trace --stats` (--shape a1,a2 --prec fp32 --reps 1 --only lists), folded in with --fold.
"""
import argparse
import ctypes
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


def make_engine(prec, p, k):
    from fmwr_amd import _lib as L, engine
    if prec == "fp64":
        return engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION)
    return engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)


def torch_lists(torch, bc, sc, bi, si, cand, chunk):
    """scores and positions of fixed-length lists cand [nc][m] (int64, on the device) in the projections' precision"""
    nc, m = cand.shape
    score = torch.empty((nc, m), dtype=torch.float64, device="cuda")
    pos = torch.empty((nc, m), dtype=torch.int64, device="cuda")
    ar = torch.arange(m, device="cuda").expand(chunk, m)
    for c0 in range(0, nc, chunk):
        c1 = min(nc, c0 + chunk)
        j = cand[c0:c1]
        g = si[j]                                                          # [T, m, k]
        d = torch.bmm(g, sc[c0:c1].unsqueeze(2)).squeeze(2)                # [T, m]
        s = (bc[c0:c1, None] + bi[j]).to(torch.float64) + d.to(torch.float64)
        order = torch.argsort(s, dim=1, descending=True, stable=True)
        p = torch.empty_like(order)
        p.scatter_(1, order, ar[: c1 - c0])
        score[c0:c1] = s
        pos[c0:c1] = p
    return score, pos


def run_shape(torch, name, prec, e, mc, mi, nc, ni, k, m, reps, only, proj):
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(11)
    cand = rng.integers(0, ni, (nc, m), dtype=np.int64)
    ml = engine.Matrix.from_csr(np.arange(nc + 1, dtype=np.int64) * m, cand.astype(np.uint32).ravel(), np.ones(nc * m, np.float32), ni)
    nnz = nc * m
    d_score = torch.empty(nnz, dtype=torch.float64, device="cuda")
    d_pos = torch.empty(nnz, dtype=torch.int64, device="cuda")
    d_rank = torch.empty(nnz, dtype=torch.int64, device="cuda")
    d_hs = torch.empty(nnz, dtype=torch.float64, device="cuda")
    cand_t = torch.tensor(cand, device="cuda")
    esz = 8 if prec == "fp64" else 4
    fb = 8 if prec == "fp64" else 16
    row_bytes = (k + fb - 1) // fb * fb * esz
    hook = L.lib().fmx_debug_lists_limits

    def lists():
        e.rank_lists_device(mc, 0, nc, mi, ml, d_score.data_ptr(), d_pos.data_ptr())
        e.sync()

    def general():
        hook(ctypes.c_int32(1), ctypes.c_int64(0))
        try:
            e.rank_lists_device(mc, 0, nc, mi, ml, d_score.data_ptr(), d_pos.data_ptr())
            e.sync()
        finally:
            hook(ctypes.c_int32(0), ctypes.c_int64(0))

    def heldout():
        e.heldout_rank_device(mc, 0, nc, mi, ml, d_rank.data_ptr(), d_hs.data_ptr())
        e.sync()

    res = {}

    def torch_():
        bc, sc, bi, si = proj
        res["t"] = torch_lists(torch, bc, sc, bi, si, cand_t, max(1, (1 << 25) // (m * k)))
        torch.cuda.synchronize()

    versions = {"lists": lists, "general": general, "heldout": heldout, "torch": torch_}
    if only:
        versions = {v: versions[v] for v in only}
    out = {"case": name, "precision": prec, "n_ctx": nc, "n_items": ni, "k": k, "list_len": m, "entries": nnz, "row_bytes": row_bytes}
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for _ in range(reps):          # alternated: one call of each version per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    for v in versions:
        out[v] = _stats(ts[v])
    if "lists" in versions and "heldout" in versions:   # the two give the same scores
        lists()
        out["score_mismatches_vs_heldout"] = int((d_score.view(torch.int64) != d_hs.view(torch.int64)).sum().item())
    if "lists" in versions and "torch" in versions:
        lists()
        tol = 1e-9 if prec == "fp64" else 1e-3
        out["torch_max_abs_diff"] = float((res["t"][0].ravel() - d_score).abs().max().item())
        out["torch_positions_differing"] = int((res["t"][1].ravel() != d_pos).sum().item())   # duplicates and near-ties are ranked differently there
        out["torch_scores_within_tol"] = bool(out["torch_max_abs_diff"] <= tol)
    # the gate: lists faster than the parent's way and than torch by more than the measured spread (max - min) of either side
    for v in ("heldout", "torch"):
        if "lists" in out and v in out:
            gap = out[v]["median_s"] - out["lists"]["median_s"]
            spread = max(out[v]["max_s"] - out[v]["min_s"], out["lists"]["max_s"] - out["lists"]["min_s"])
            out[f"gate_lists_faster_than_{v}"] = bool(gap > spread)
    # rows / s; fmx_measure_gather takes rows of at most 256 bytes: a longer row is priced as its bytes at the 256-byte rows' byte rate
    probe = min(row_bytes, 256)
    rate = engine.measure_gather(ni * row_bytes, probe) * probe / row_bytes
    out["gather_probe_row_bytes"] = probe
    out["gather_rows_per_s"] = rate
    out["bound_s"] = nnz / rate
    for v in ("lists", "general"):
        if v in out:
            out[f"{v}_over_bound"] = out[v]["median_s"] / out["bound_s"]
    print(json.dumps(out), flush=True)
    return out


def shape_a(torch, prec, m, reps, only):
    from fmwr_amd import engine
    nu, ni, k = 138_493, 26_744, 64
    p = nu + ni
    mc = engine.Matrix.from_csr(np.arange(nu + 1, dtype=np.int64), np.arange(nu, dtype=np.uint32), np.ones(nu, np.float32), p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64), np.arange(nu, nu + ni, dtype=np.uint32), np.ones(ni, np.float32), p)
    e = make_engine(prec, p, k)
    e.init_normal(7, 0.0, 0.1)
    w0, w, v = e.get_params()
    dt = torch.float64 if prec == "fp64" else torch.float32
    proj = (torch.tensor(w0 + w[:nu], device="cuda", dtype=dt), torch.tensor(v[:, :nu].T.copy(), device="cuda", dtype=dt),
            torch.tensor(w[nu:], device="cuda", dtype=dt), torch.tensor(v[:, nu:].T.copy(), device="cuda", dtype=dt))
    return run_shape(torch, f"a_movielens20m_{m}", prec, e, mc, mi, nu, ni, k, m, reps, only, proj)


def shape_b(torch, reps, only):
    from fmwr_amd import engine
    nc, ni, p, k, m = 100_000, 1_000_000, 1_000_000, 16, 500
    rng = np.random.default_rng(2)
    ccol = np.sort(rng.integers(0, p, (nc, 25)), axis=1).astype(np.uint32).ravel()
    icol = np.sort(rng.integers(0, p, (ni, 5)), axis=1).astype(np.uint32).ravel()
    cval = rng.uniform(0.5, 1.5, nc * 25).astype(np.float32)
    ival = rng.uniform(0.5, 1.5, ni * 5).astype(np.float32)
    mc = engine.Matrix.from_csr(np.arange(nc + 1, dtype=np.int64) * 25, ccol, cval, p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64) * 5, icol, ival, p)
    e = make_engine("fp32", p, k)
    e.init_normal(7, 0.0, 0.1)
    bc, sc = e.project(mc, with_w0=True)   # (the torch baseline's inputs; made by the library here, not timed)
    bi, si = e.project(mi, with_w0=False)
    proj = tuple(torch.tensor(x, device="cuda", dtype=torch.float32) for x in (bc, sc, bi, si))
    return run_shape(torch, "b_100k_x_1m_500", "fp32", e, mc, mi, nc, ni, k, m, reps, only, proj)


def write_txt(rec, path):
    lines = ["fmx_rank_lists_device record (profiles/lists_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        lines.append(f"{o['case']} {o['precision']}: {o['n_ctx']} contexts x {o['list_len']} candidates of {o['n_items']} items, k {o['k']}, "
                     f"{o['entries']} entries, s rows of {o['row_bytes']} bytes")
        for v in ("lists", "general", "heldout", "torch"):
            if v in o:
                t = o[v]
                extra = f"   = {t['median_s'] / o['lists']['median_s']:.2f}x lists" if v != "lists" and "lists" in o else ""
                lines.append(f"  {v:8s} {t['median_s'] * 1e3:10.3f} ms [{t['min_s'] * 1e3:.3f}, {t['max_s'] * 1e3:.3f}]{extra}")
        lines.append(f"  bound    {o['bound_s'] * 1e3:10.3f} ms ({o['gather_rows_per_s'] / 1e9:.2f} G rows/s measured)"
                     + "".join(f"; {v} = {o[v + '_over_bound']:.2f}x bound" for v in ("lists", "general") if v + "_over_bound" in o))
        gates = [f"{g[len('gate_'):]}: {'PASS' if o[g] else 'FAIL'}" for g in sorted(o) if g.startswith("gate_")]
        if gates:
            lines.append("  gate (faster by more than the spread of either side): " + "; ".join(gates))
        if "score_mismatches_vs_heldout" in o:
            lines.append(f"  scores differing in bits from fmx_heldout_rank's: {o['score_mismatches_vs_heldout']}")
        if "torch_max_abs_diff" in o:
            lines.append(f"  torch: max |score difference| {o['torch_max_abs_diff']:.3g}; positions differing {o['torch_positions_differing']} "
                         f"(duplicates count twice there)")
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
    ap.add_argument("--shape", default="all", help="comma list of a1 (100 candidates), a2 (1 000), b; or all")
    ap.add_argument("--prec", default="both", choices=["both", "fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="", help="comma list of versions to run (lists, general, heldout, torch); default all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lists.json"))
    ap.add_argument("--merge", nargs="+", metavar="RECORD_JSON", help="join the records of separate runs (one process per shape) into --out")
    ap.add_argument("--fold", nargs=3, metavar=("RECORD_JSON", "STATS_CSV", "RUN"), help="add kernel shares to a record and rewrite its .txt")
    args = ap.parse_args()
    if args.fold:
        rec = json.load(open(args.fold[0]))
        rec["kernel_stats"] = fold_stats(args.fold[1], args.fold[2])
        json.dump(rec, open(args.fold[0], "w"), indent=1)
        write_txt(rec, args.fold[0].replace(".json", ".txt"))
        return
    if args.merge:
        recs = [json.load(open(f)) for f in args.merge]
        rec = {"reps": recs[0]["reps"], "cases": [c for r in recs for c in r["cases"]]}
        json.dump(rec, open(args.out, "w"), indent=1)
        write_txt(rec, args.out.replace(".json", ".txt"))
        return
    import torch
    shapes = ["a1", "a2", "b"] if args.shape == "all" else args.shape.split(",")
    only = [v for v in args.only.split(",") if v]
    rec = {"reps": args.reps, "cases": []}
    for prec in (["fp32", "fp64"] if args.prec == "both" else [args.prec]):
        for sh, m in (("a1", 100), ("a2", 1000)):
            if sh in shapes:
                rec["cases"].append(shape_a(torch, prec, m, args.reps, only))
    if "b" in shapes:
        rec["cases"].append(shape_b(torch, args.reps, only))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
