"""fmx_topk_index_device measured against fmx_topk_device on the same engine and matrices.  Writes profiles/index.json and a one-page
profiles/index.txt.

Items and contexts are one-hot rows (item i = feature i, context c = feature n_items + c), so a row's projection is a column of V and the
shapes differ only in how V is drawn:
  a  100 000 contexts x 1 000 000 items, k = 16, K = 100, fp32, CLUSTERED projections: 2 000 centres N(0, 0.5), an item = its centre +
     N(0, 0.1), a context = a centre + N(0, 0.1) -- what a trained model's items look like to an inverted-file index;
  b  the same with i.i.d. N(0, 0.3) projections, where clustering cannot help;
  c  1 and 64 contexts of shape a against the 1 M items -- the serving case -- with the share of the call that fmx_project_device of the
     items takes when timed alone.
Per shape: one index per n_lists (fmx_index_build, n_iter = 10; the build is timed once), then, after one warm-up call of everything, --reps
rounds in which the yardstick and every (n_lists, n_probe) point are called once each (median, [min, max]); recall@K against fmx_topk on the
first 2 000 contexts, and the mean scanned / n_items.  Every point is timed three times per round: under the rule's choice of the fine form
and with the context form and the list form forced (fmx_debug_index_limits); the record says whether the rule took the faster form.  The
gate (shape a), per n_lists: at the smallest measured n_probe whose recall@K is >= 0.9 the indexed call (the rule's choice) is faster than
fmx_topk by more than the spread of either side.
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

from topk_bench import _stats  # noqa: E402

K_FACTORS, TOP_K = 16, 100


def _model(kind, ni, nc, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        cen = rng.normal(0, 0.5, (2000, K_FACTORS))
        vi = cen[rng.integers(0, 2000, ni)] + rng.normal(0, 0.1, (ni, K_FACTORS))
        vc = cen[rng.integers(0, 2000, nc)] + rng.normal(0, 0.1, (nc, K_FACTORS))
    else:
        vi, vc = rng.normal(0, 0.3, (ni, K_FACTORS)), rng.normal(0, 0.3, (nc, K_FACTORS))
    return np.concatenate([vi, vc]).T.copy(), rng.normal(0, 0.1, ni + nc)


def _one_hot(engine, lo, n, p):
    return engine.Matrix.from_csr(np.arange(n + 1, dtype=np.int64), np.arange(lo, lo + n, dtype=np.uint32), np.ones(n, np.float32), p)


def run_shape(torch, name, kind, ni, ncs, lists, probes, reps):
    from fmwr_amd import _lib as L, engine
    nc_max = max(ncs)
    p = ni + nc_max
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=K_FACTORS, task=L.TASK_REGRESSION, batch_rows=4096)
    v, w = _model(kind, ni, nc_max)
    e.set_params(0.1, w, v)
    del v, w
    mi = _one_hot(engine, 0, ni, p)
    di = torch.empty((nc_max, TOP_K), dtype=torch.int64, device="cuda")
    ds = torch.empty((nc_max, TOP_K), dtype=torch.float64, device="cuda")
    gi = torch.empty((nc_max, TOP_K), dtype=torch.int64, device="cuda")
    gn = torch.empty(nc_max, dtype=torch.int64, device="cuda")
    pb = torch.empty(ni, dtype=torch.float64, device="cuda")
    ps = torch.empty((ni, K_FACTORS), dtype=torch.float64, device="cuda")
    out = {"shape": name, "projections": kind, "n_items": ni, "k": K_FACTORS, "top_k": TOP_K, "builds": [], "cases": []}
    index = {}
    for nl in lists:
        t = time.perf_counter()
        index[nl] = e.index_build(mi, nl, n_iter=10, seed=1)
        e.sync()
        out["builds"].append({"n_lists": nl, "build_s": time.perf_counter() - t, "non_empty": index[nl].non_empty})
        print(json.dumps(out["builds"][-1]), flush=True)
    for nc in ncs:
        mc = _one_hot(engine, ni, nc, p)

        def topk():
            e.topk_device(mc, 0, nc, mi, TOP_K, di.data_ptr(), ds.data_ptr())
            e.sync()

        def indexed(nl, q, form=0):
            L.check(L.lib().fmx_debug_index_limits(form, 0, 0))
            e.topk_index_device(index[nl], mc, 0, nc, mi, TOP_K, q, gi.data_ptr(), ds.data_ptr(), gn.data_ptr())
            e.sync()

        def project():
            e.project_device(mi, 0, ni, pb.data_ptr(), ps.data_ptr())
            e.sync()

        points = [(nl, q) for nl in lists for q in probes if q <= nl]
        rows = min(nc, 2000)
        topk()
        want = di[:rows].cpu().numpy()
        case = {"n_ctx": nc, "points": []}
        for nl, q in points:                       # warm-up, recall and scanned
            indexed(nl, q)
            got = gi[:rows].cpu().numpy()
            rec = float(np.mean([np.isin(a[a >= 0], b).mean() if (a >= 0).any() else 1.0 for a, b in zip(want, got)]))
            case["points"].append({"n_lists": nl, "n_probe": q, "recall": rec, "scanned_share": float(gn[:nc].double().mean().item()) / ni})
        project()
        for nl, q in points:                       # the forced forms' warm-up
            indexed(nl, q, 1); indexed(nl, q, 2)
        ts = {"topk": [], "project": [], **{pt: [] for pt in points}, **{(pt, f): [] for pt in points for f in (1, 2)}}
        for _ in range(reps):                      # alternated: one call of everything per round
            t = time.perf_counter(); topk(); ts["topk"].append(time.perf_counter() - t)
            t = time.perf_counter(); project(); ts["project"].append(time.perf_counter() - t)
            for nl, q in points:
                t = time.perf_counter(); indexed(nl, q); ts[nl, q].append(time.perf_counter() - t)
                for f in (1, 2):
                    t = time.perf_counter(); indexed(nl, q, f); ts[(nl, q), f].append(time.perf_counter() - t)
        L.check(L.lib().fmx_debug_index_limits(0, 0, 0))
        case["fmx_topk"], case["project_items"] = _stats(ts["topk"]), _stats(ts["project"])
        for pt, rec in zip(points, case["points"]):
            rec.update(_stats(ts[pt]))
            rec["context_form"], rec["list_form"] = _stats(ts[pt, 1]), _stats(ts[pt, 2])
            rec["rule_takes"] = "context"             # the rule as fm_index.hip states it
            fast = "list" if rec["list_form"]["median_s"] < rec["context_form"]["median_s"] else "context"
            gap = abs(rec["list_form"]["median_s"] - rec["context_form"]["median_s"])
            sp = max(rec["list_form"]["max_s"] - rec["list_form"]["min_s"], rec["context_form"]["max_s"] - rec["context_form"]["min_s"])
            rec["faster_form"] = fast if gap > sp else "within the spread"
            rec["rule_right"] = bool(rec["faster_form"] in (rec["rule_takes"], "within the spread"))
            rec["speedup"] = case["fmx_topk"]["median_s"] / rec["median_s"]
            rec["project_share"] = case["project_items"]["median_s"] / rec["median_s"]
            spread = max(rec["max_s"] - rec["min_s"], case["fmx_topk"]["max_s"] - case["fmx_topk"]["min_s"])
            rec["faster_beyond_spread"] = bool(case["fmx_topk"]["median_s"] - rec["median_s"] > spread)
        case["gate"] = []                          # per n_lists: the smallest measured n_probe whose recall is >= 0.9
        for nl in lists:
            good = [r for r in case["points"] if r["n_lists"] == nl and r["recall"] >= 0.9]
            if good:
                at = min(good, key=lambda r: r["n_probe"])
                case["gate"].append({"n_lists": nl, "n_probe": at["n_probe"], "recall": at["recall"], "speedup": at["speedup"], "met": at["faster_beyond_spread"]})
            else:
                case["gate"].append({"n_lists": nl, "met": False, "reason": "no measured n_probe reaches recall 0.9"})
        print(json.dumps(case), flush=True)
        out["cases"].append(case)
    return out


def write_txt(rec, path):
    lines = ["fmx_topk_index_device record (profiles/index_bench.py); times: median of %d alternated calls after one warm-up, [min, max];" % rec["reps"],
             "recall@100 against fmx_topk on the first 2 000 contexts; each point under the rule's choice of the fine form and with each form forced", ""]
    for o in rec["shapes"]:
        lines.append(f"{o['shape']}: {o['projections']} projections, {o['n_items']} items, k {o['k']}, top_k {o['top_k']}")
        lines.append("  fmx_index_build (n_iter 10): " + ", ".join(f"{b['n_lists']} lists {b['build_s']:.2f} s ({b['non_empty']} non-empty)" for b in o["builds"]))
        for c in o["cases"]:
            t, pj = c["fmx_topk"], c["project_items"]
            lines.append(f"  {c['n_ctx']} contexts: fmx_topk_device {t['median_s'] * 1e3:.2f} ms [{t['min_s'] * 1e3:.2f}, {t['max_s'] * 1e3:.2f}]; "
                         f"fmx_project_device of the items alone {pj['median_s'] * 1e3:.2f} ms")
            lines.append("    n_lists n_probe   recall  scanned   rule: ms [min, max]         x fmx_topk  proj. share   context form ms   list form ms   rule takes / faster")
            for r in c["points"]:
                cf, lf = r["context_form"], r["list_form"]
                lines.append(f"    {r['n_lists']:7d} {r['n_probe']:7d} {r['recall']:8.4f} {r['scanned_share']:8.5f} {r['median_s'] * 1e3:9.2f} "
                             f"[{r['min_s'] * 1e3:.2f}, {r['max_s'] * 1e3:.2f}]  {r['speedup']:8.2f}x  {r['project_share']:.2f}"
                             f"   {cf['median_s'] * 1e3:9.2f} [{cf['min_s'] * 1e3:.2f}, {cf['max_s'] * 1e3:.2f}]   {lf['median_s'] * 1e3:9.2f} [{lf['min_s'] * 1e3:.2f}, {lf['max_s'] * 1e3:.2f}]"
                             f"   {r['rule_takes']} / {r['faster_form']}" + ("" if r["rule_right"] else "  RULE WRONG")
                             + ("" if r["faster_beyond_spread"] else "   (not faster than fmx_topk beyond the spread)"))
            for g in c["gate"]:
                lines.append(f"    gate, n_lists {g['n_lists']}: " + (f"n_probe {g['n_probe']}: recall {g['recall']:.4f}, {g['speedup']:.2f}x fmx_topk -- "
                                                                    + ("MET" if g["met"] else "NOT MET") if "n_probe" in g else "NOT MET: " + g["reason"]))
        lines.append("")
    if rec.get("notes"):
        lines += rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b, c; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--contexts", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index.json"))
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b", "c"] if args.shape == "all" else args.shape.split(",")
    lists, probes = [256, 1024, 4096], [1, 4, 16, 64]
    rec = {"script": "profiles/index_bench.py", "reps": args.reps, "shapes": [], "notes": args.note}
    if "a" in shapes:
        rec["shapes"].append(run_shape(torch, "a_100k_x_1m_clustered", "clustered", args.items, [args.contexts], lists, probes, args.reps))
    if "b" in shapes:
        rec["shapes"].append(run_shape(torch, "b_100k_x_1m_iid", "iid", args.items, [args.contexts], lists, probes, args.reps))
    if "c" in shapes:
        rec["shapes"].append(run_shape(torch, "c_serving", "clustered", args.items, [1, 64], [1024], [1, 4, 16, 64], args.reps))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
