"""fmx_diversify_device measured against a torch formulation of the same greedy MMR on the same device and the same projections (the
yardstick only, never the product path).  Writes profiles/diversify.json and a one-page profiles/diversify.txt.

Shapes (the matrices and the untrained model of profiles/lists_bench.py):
  a1, a2  MovieLens-20M-shaped: 138 493 one-hot users x 26 744 one-hot items, k = 64, fp32 (mini-batch) and fp64 (sequential) engines;
          pools of P = 100 with K = 10, and of P = 1 000 with K = 50;
  b       100 000 contexts (25 nnz) x 1 000 000 items (5 nnz), p = 1 M, k = 16, fp32, P = 500, K = 20.
The pools are made beforehand by fmx_topk_lists_device(top_k = P) from P uniform candidates per context (its one call is timed once, for
the ratio).  trade_off 0.7, min-max relevance.  Per shape, in one process, after one warm-up call of every version, --reps rounds with the
versions alternated (median, [min, max]):
  diversify  fmx_diversify_device as it runs by default (the pool in LDS where its tile fits the budget, else read from global memory)
  global     the same call with the test hook forcing the global form (recorded only where the default is the LDS form)
  torch      row gather of the pool's projections, normalisation, bmm to the [n, P, P] cosine tensor in slabs that fit memory, and a K-step
             masked-argmax loop; the projections are made beforehand and not timed
  gate       diversify faster than torch by more than the spread (max - min) of either side
Every shape may run in a process of its own (--shape, --prec, --nctx, --out) and the records be joined with --merge.  Kernel shares come
from a separate run under `rocprofv3 --kernel-trace --stats` (--shape a1 --prec fp32 --reps 1 --only diversify), folded in with --fold.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lists_bench import _stats, fold_stats, make_engine  # noqa: E402

LAMBDA = 0.7
TILE_BYTES = 56 << 10   # fm_diversify.hip's DV_TILE_BYTES


def torch_mmr(torch, si, index, score, K, lam, slab):
    """greedy MMR (min-max relevance, cosine of the projections) of pools index / score [n][P] on the device, in slabs of `slab` rows"""
    n, P = index.shape
    out = torch.empty((n, K), dtype=torch.int64, device="cuda")
    for c0 in range(0, n, slab):
        c1 = min(n, c0 + slab)
        idx, sc = index[c0:c1], score[c0:c1].to(si.dtype)
        live = idx >= 0
        g = si[idx.clamp(min=0)]                                            # [T, P, k]
        g = g / g.norm(dim=2, keepdim=True).clamp(min=1e-30)
        cos = torch.bmm(g, g.transpose(1, 2))                               # [T, P, P]
        hi = torch.where(live, sc, torch.full_like(sc, -float("inf"))).max(1, keepdim=True).values
        lo = torch.where(live, sc, torch.full_like(sc, float("inf"))).min(1, keepdim=True).values
        rel = (sc - lo) / (hi - lo).clamp(min=1e-30)
        pen = torch.zeros_like(rel)
        left = live.clone()
        ar = torch.arange(c1 - c0, device="cuda")
        for t in range(K):
            margin = torch.where(left, lam * rel - (1.0 - lam) * pen, torch.full_like(rel, -float("inf")))
            v = margin.argmax(1)
            out[c0:c1, t] = idx[ar, v]
            left[ar, v] = False
            sim = cos[ar, :, v]
            pen = sim if t == 0 else torch.maximum(pen, sim)
    return out


def run_shape(torch, name, prec, e, mc, mi, nc, ni, k, P, K, reps, only, si_t):
    from fmwr_amd import _lib as L, engine
    rng = np.random.default_rng(11)
    cand = rng.integers(0, ni, (nc, P), dtype=np.int64)
    ml = engine.Matrix.from_csr(np.arange(nc + 1, dtype=np.int64) * P, cand.astype(np.uint32).ravel(), np.ones(nc * P, np.float32), ni)
    d_pi = torch.empty((nc, P), dtype=torch.int64, device="cuda")
    d_ps = torch.empty((nc, P), dtype=torch.float64, device="cuda")
    e.topk_lists_device(mc, 0, nc, mi, ml, P, d_pi.data_ptr(), d_ps.data_ptr())   # warm-up
    e.sync()
    t0 = time.perf_counter()
    e.topk_lists_device(mc, 0, nc, mi, ml, P, d_pi.data_ptr(), d_ps.data_ptr())
    e.sync()
    pool_s = time.perf_counter() - t0
    d_oi = torch.empty((nc, K), dtype=torch.int64, device="cuda")
    d_os = torch.empty((nc, K), dtype=torch.float64, device="cuda")
    d_om = torch.empty((nc, K), dtype=torch.float64, device="cuda")
    esz, fb = (8, 8) if prec == "fp64" else (4, 16)
    row_bytes = (k + fb - 1) // fb * fb * esz
    lds_default = P * (row_bytes + 16) <= TILE_BYTES
    hook = L.lib().fmx_debug_diversify_limits

    def diversify():
        e.diversify_device(mi, nc, P, d_pi.data_ptr(), d_ps.data_ptr(), K, LAMBDA, L.DIV_REL_MINMAX, d_oi.data_ptr(), d_os.data_ptr(), d_om.data_ptr())
        e.sync()

    def global_():
        hook(ctypes.c_int32(-1), ctypes.c_int64(0))
        try:
            diversify()
        finally:
            hook(ctypes.c_int32(0), ctypes.c_int64(0))

    res = {}

    def torch_():
        res["t"] = torch_mmr(torch, si_t, d_pi, d_ps, K, LAMBDA, max(1, (1 << 28) // (P * P)))
        torch.cuda.synchronize()

    versions = {"diversify": diversify, "torch": torch_}
    if lds_default:
        versions["global"] = global_
    if only:
        versions = {v: versions[v] for v in only if v in versions}
    out = {"case": name, "precision": prec, "n_ctx": nc, "n_items": ni, "k": k, "pool": P, "top_k": K, "row_bytes": row_bytes,
           "default_form": "lds" if lds_default else "global", "pool_call_s": pool_s}
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for _ in range(reps):          # alternated: one call of each version per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    for v in versions:
        out[v] = _stats(ts[v])
    if "diversify" in out:
        out["diversify_over_pool_call"] = out["diversify"]["median_s"] / pool_s
    if "diversify" in out and "torch" in out:
        diversify()
        out["torch_rows_with_the_same_picks"] = float((res["t"] == d_oi).all(1).double().mean().item())   # near-ties and duplicates differ there
        gap = out["torch"]["median_s"] - out["diversify"]["median_s"]
        spread = max(out["torch"]["max_s"] - out["torch"]["min_s"], out["diversify"]["max_s"] - out["diversify"]["min_s"])
        out["gate_diversify_faster_than_torch"] = bool(gap > spread)
    print(json.dumps(out), flush=True)
    return out


def shape_a(torch, prec, P, K, reps, only, nctx):
    from fmwr_amd import engine
    nu, ni, k = nctx or 138_493, 26_744, 64
    p = nu + ni
    mc = engine.Matrix.from_csr(np.arange(nu + 1, dtype=np.int64), np.arange(nu, dtype=np.uint32), np.ones(nu, np.float32), p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64), np.arange(nu, nu + ni, dtype=np.uint32), np.ones(ni, np.float32), p)
    e = make_engine(prec, p, k)
    e.init_normal(7, 0.0, 0.1)
    _, s = e.project(mi)
    si_t = torch.tensor(s, device="cuda", dtype=torch.float64 if prec == "fp64" else torch.float32)
    return run_shape(torch, f"a_movielens20m_P{P}_K{K}", prec, e, mc, mi, nu, ni, k, P, K, reps, only, si_t)


def shape_b(torch, reps, only, nctx):
    from fmwr_amd import engine
    nc, ni, p, k, P, K = nctx or 100_000, 1_000_000, 1_000_000, 16, 500, 20
    rng = np.random.default_rng(2)
    ccol = np.sort(rng.integers(0, p, (nc, 25)), axis=1).astype(np.uint32).ravel()
    icol = np.sort(rng.integers(0, p, (ni, 5)), axis=1).astype(np.uint32).ravel()
    mc = engine.Matrix.from_csr(np.arange(nc + 1, dtype=np.int64) * 25, ccol, rng.uniform(0.5, 1.5, nc * 25).astype(np.float32), p)
    mi = engine.Matrix.from_csr(np.arange(ni + 1, dtype=np.int64) * 5, icol, rng.uniform(0.5, 1.5, ni * 5).astype(np.float32), p)
    e = make_engine("fp32", p, k)
    e.init_normal(7, 0.0, 0.1)
    _, s = e.project(mi)
    return run_shape(torch, f"b_100k_x_1m_P{P}_K{K}", "fp32", e, mc, mi, nc, ni, k, P, K, reps, only, torch.tensor(s, device="cuda", dtype=torch.float32))


def write_txt(rec, path):
    lines = ["fmx_diversify_device record (profiles/diversify_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        lines.append(f"{o['case']} {o['precision']}: {o['n_ctx']} contexts, pools of {o['pool']} of {o['n_items']} items, top_k {o['top_k']}, k {o['k']}, "
                     f"s rows of {o['row_bytes']} bytes, default form: {o['default_form']}")
        for v in ("diversify", "global", "torch"):
            if v in o:
                t = o[v]
                extra = f"   = {t['median_s'] / o['diversify']['median_s']:.2f}x diversify" if v != "diversify" and "diversify" in o else ""
                lines.append(f"  {v:9s} {t['median_s'] * 1e3:10.3f} ms [{t['min_s'] * 1e3:.3f}, {t['max_s'] * 1e3:.3f}]{extra}")
        lines.append(f"  the fmx_topk_lists_device(top_k = P) call that made the pools: {o['pool_call_s'] * 1e3:.3f} ms (one call)"
                     + (f"; diversify = {o['diversify_over_pool_call']:.2f}x that" if "diversify_over_pool_call" in o else ""))
        if "gate_diversify_faster_than_torch" in o:
            lines.append("  gate (faster than torch by more than the spread of either side): " + ("PASS" if o["gate_diversify_faster_than_torch"] else "FAIL"))
            lines.append(f"  rows where torch picks the same items in the same order: {o['torch_rows_with_the_same_picks'] * 100:.2f} %")
    if rec.get("kernel_stats"):
        lines += ["", "kernel shares (rocprofv3 --kernel-trace --stats, separate run): " + rec["kernel_stats"].get("run", "")]
        for row in rec["kernel_stats"]["rows"]:
            lines.append(f"  {row['share']:6.2f} %  {row['total_ms']:9.2f} ms  {row['name']}")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a1 (P 100, K 10), a2 (P 1 000, K 50), b; or all")
    ap.add_argument("--prec", default="both", choices=["both", "fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nctx", type=int, default=0, help="fewer context rows than the shape's (a shortened record says so in its case line)")
    ap.add_argument("--only", default="", help="comma list of versions to run (diversify, global, torch); default all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify.json"))
    ap.add_argument("--merge", nargs="+", metavar="RECORD_JSON", help="join the records of separate runs into --out")
    ap.add_argument("--fold", nargs=3, metavar=("RECORD_JSON", "STATS_CSV", "RUN"), help="add kernel shares to a record and rewrite its .txt")
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    if args.fold:
        rec = json.load(open(args.fold[0]))
        rec["kernel_stats"] = fold_stats(args.fold[1], args.fold[2])
        json.dump(rec, open(args.fold[0], "w"), indent=1)
        write_txt(rec, args.fold[0].replace(".json", ".txt"))
        return
    if args.merge:
        recs = [json.load(open(f)) for f in args.merge]
        rec = {"reps": recs[0]["reps"], "cases": [c for r in recs for c in r["cases"]], "notes": [n for r in recs for n in r.get("notes", [])] + args.note}
        json.dump(rec, open(args.out, "w"), indent=1)
        write_txt(rec, args.out.replace(".json", ".txt"))
        return
    import torch
    shapes = ["a1", "a2", "b"] if args.shape == "all" else args.shape.split(",")
    only = [v for v in args.only.split(",") if v]
    rec = {"reps": args.reps, "cases": [], "notes": args.note}
    for prec in (["fp32", "fp64"] if args.prec == "both" else [args.prec]):
        for sh, P, K in (("a1", 100, 10), ("a2", 1000, 50)):
            if sh in shapes:
                rec["cases"].append(shape_a(torch, prec, P, K, args.reps, only, args.nctx))
    if "b" in shapes:
        rec["cases"].append(shape_b(torch, args.reps, only, args.nctx))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
