"""fmx_neighbors_device measured against two yardsticks on the same device and the same rows (neither is a product path).  Writes
profiles/neighbors.json and a one-page profiles/neighbors.txt.

Shapes (the matrices and the untrained model of profiles/topk_bench.py):
  a  all items against all items at MovieLens-20M's item count: 26 744 one-hot items, k = 64, K = 10, skip_self, fp32 (mini-batch) and fp64
     (sequential) engines;
  b  100 000 queries (25 nnz) x 1 000 000 items (5 nnz), p = 1 M, k = 16, K = 100, fp32 -- profiles/topk_r07.txt's shape.
Per shape, in one process, after one warm-up call of every version, --reps rounds with the versions alternated (median, [min, max]):
  neighbors  fmx_neighbors_device, FMX_SIM_COSINE, all query rows, ended by a device synchronise
  dot        the same call with FMX_SIM_DOT (no norms, no fp64 products)
  topk       fmx_topk_device on the same two matrices and the same K: the same product and selection, the score base_c + base_i + dot
  torch      the projections (made beforehand, not timed) row-normalised, then per chunk of queries torch.mm and torch.topk in the engine's
             precision (a 2 GB score block per chunk; the own row masked where the shape skips it)
No threshold is set: the record states both ratios and the spread, and says where fmx_neighbors is the slower one.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from topk_bench import _stats, _synthetic  # noqa: E402


def run_shape(torch, name, prec, Q_csr, I_csr, p, k, K, skip_self, reps, only):
    from fmwr_amd import _lib as L, engine
    if prec == "fp64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, num_factor=k, task=L.TASK_REGRESSION)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    mi = engine.Matrix.from_csr(*I_csr, p)
    mq = mi if Q_csr is None else engine.Matrix.from_csr(*Q_csr, p)
    nq, ni = mq.n, mi.n
    dt = torch.float64 if prec == "fp64" else torch.float32
    si = torch.tensor(e.project(mi)[1], device="cuda", dtype=dt)
    sq = si if Q_csr is None else torch.tensor(e.project(mq)[1], device="cuda", dtype=dt)
    di = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    ds = torch.empty((nq, K), dtype=torch.float64, device="cuda")
    ti = torch.empty((nq, K), dtype=torch.int64, device="cuda")
    chunk = max(1, (1 << 31) // (ni * (8 if prec == "fp64" else 4)))

    def neighbors(metric=L.SIM_COSINE):
        e.neighbors_device(mq, 0, nq, mi, K, di.data_ptr(), ds.data_ptr(), metric=metric, skip_self=skip_self)
        e.sync()

    def dot():
        neighbors(L.SIM_DOT)

    def topk():
        e.topk_device(mq, 0, nq, mi, K, di.data_ptr(), ds.data_ptr())
        e.sync()

    def torch_():
        qn = sq / sq.norm(dim=1, keepdim=True).clamp(min=1e-30)
        itn = (si / si.norm(dim=1, keepdim=True).clamp(min=1e-30)).T.contiguous()
        for c0 in range(0, nq, chunk):
            c1 = min(nq, c0 + chunk)
            sc = torch.mm(qn[c0:c1], itn)
            if skip_self:
                ar = torch.arange(c1 - c0, device="cuda")
                sc[ar, c0 + ar] = -float("inf")
            ti[c0:c1] = torch.topk(sc, K, dim=1).indices
        torch.cuda.synchronize()

    versions = {"neighbors": neighbors, "dot": dot, "topk": topk, "torch": torch_}
    if only:
        versions = {v: versions[v] for v in only if v in versions}
    out = {"case": name, "precision": prec, "n_queries": nq, "n_items": ni, "k": k, "top_k": K, "skip_self": bool(skip_self), "torch_chunk_rows": chunk}
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for _ in range(reps):          # alternated: one call of each version per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    for v in versions:
        out[v] = _stats(ts[v])
    if "neighbors" in out:
        out["pairs_per_s"] = nq * ni / out["neighbors"]["median_s"]
        for v in ("dot", "topk", "torch"):
            if v in out:
                out[f"{v}_over_neighbors"] = out[v]["median_s"] / out["neighbors"]["median_s"]
                spread = max(out[v]["max_s"] - out[v]["min_s"], out["neighbors"]["max_s"] - out["neighbors"]["min_s"])
                gap = out[v]["median_s"] - out["neighbors"]["median_s"]
                out[f"neighbors_vs_{v}"] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"
        if "torch" in out:
            neighbors()
            rows = min(nq, 4096)   # near-ties differ between the two roundings
            out["torch_rows_with_the_same_neighbours"] = float((ti[:rows].sort(1).values == di[:rows].sort(1).values).all(1).double().mean().item())
    print(json.dumps(out), flush=True)
    return out


def write_txt(rec, path):
    lines = ["fmx_neighbors_device record (profiles/neighbors_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        lines.append(f"{o['case']} {o['precision']}: {o['n_queries']} queries x {o['n_items']} items, k {o['k']}, top_k {o['top_k']}"
                     + (", skip_self" if o["skip_self"] else ""))
        for v in ("neighbors", "dot", "topk", "torch"):
            if v in o:
                t = o[v]
                extra = ""
                if v != "neighbors" and "neighbors" in o:
                    extra = f"   = {o[v + '_over_neighbors']:.2f}x neighbors (the cosine call is {o['neighbors_vs_' + v]})"
                elif v == "neighbors":
                    extra = f"   {o['pairs_per_s'] / 1e9:.1f} G pairs/s"
                lines.append(f"  {v:9s} {t['median_s'] * 1e3:10.3f} ms [{t['min_s'] * 1e3:.3f}, {t['max_s'] * 1e3:.3f}]{extra}")
        if "torch_rows_with_the_same_neighbours" in o:
            lines.append(f"  first rows where torch ({o['torch_chunk_rows']} rows per chunk) finds the same set of neighbours: "
                         f"{o['torch_rows_with_the_same_neighbours'] * 100:.2f} %")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b; or all")
    ap.add_argument("--prec", default="both", choices=["both", "fp64", "fp32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="comma list of versions to run (neighbors, dot, topk, torch); default all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbors.json"))
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b"] if args.shape == "all" else args.shape.split(",")
    only = [v for v in args.only.split(",") if v]
    rec = {"script": "profiles/neighbors_bench.py", "reps": args.reps, "cases": [], "notes": args.note}
    if "a" in shapes:
        users, items = 138_493, 26_744
        p = users + items
        Im = _synthetic(items, users, p, 1, 0, one_hot=True)
        for prec in (["fp32", "fp64"] if args.prec == "both" else [args.prec]):
            rec["cases"].append(run_shape(torch, "a_movielens20m_items", prec, None, Im, p, 64, 10, True, args.reps, only))
    if "b" in shapes:
        p = 1_000_000
        Qm = _synthetic(100_000, 0, p, 25, 1)
        Im = _synthetic(1_000_000, 0, p, 5, 2)
        rec["cases"].append(run_shape(torch, "b_100k_x_1m", "fp32", Qm, Im, p, 16, 100, False, args.reps, only))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
