"""Value binning on the device (fmx_matrix_column_quantiles + fmx_matrix_bin_columns) measured against the only route the library offered before --
Matrix.export -> numpy (a sort and a searchsorted per column, no np.quantile) -> Matrix.from_csr -- and, beside it, against a torch formulation on
the same device (sort, bucketize) that is handed the arrays for free and leaves its result as tensors.  Writes profiles/bins.json and the
timing part of profiles/bins.txt (what that file holds from the line "---- end to end" on, the AUC series of tests/test_gpu_bins.py, is kept).

Shapes:
  a  synthetic_fields(10 M rows, 13 dense columns, the 26 Criteo-shaped fields): the 13 dense columns at 32 bins, fit then apply.
  b  configs[1]'s matrix (10 M rows x 1 M features, 30 entries per row) after synthetic_values: 8 columns at 256 bins.
Per shape, in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min, max]).  The gate: the
device route is faster than the host round trip by more than the spread of either side; the record says so in bold if not, and states the torch
comparison either way.  The apply call alone is timed too, for its bytes per second."""
import argparse
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


def _alternate(versions, reps):
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for r in range(reps):          # alternated: one call of each route per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
        print("round", r + 1, {v: round(t[-1], 4) for v, t in ts.items()}, file=sys.stderr, flush=True)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out):
    for other in ("host", "torch"):
        if other not in out:
            continue
        spread = max(out[other]["max_s"] - out[other]["min_s"], out["device"]["max_s"] - out["device"]["min_s"])
        gap = out[other]["median_s"] - out["device"]["median_s"]
        out[other + "_over_device"] = out[other]["median_s"] / out["device"]["median_s"]
        out["device_vs_" + other] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _host_edges(v, bins):
    """the definition on one column's stored values, with a sort and integer indexing"""
    v = np.sort(v[~np.isnan(v)] + np.float32(0))          # (-0 + 0 = +0)
    if not len(v):
        return np.zeros(0, np.float32)
    cand = np.unique(v[(np.arange(1, bins, dtype=np.int64) * len(v)) // bins])
    return cand[cand > v[0]]


def _host_route(engine, m, cols, bins):
    """the parent's route: everything exported, binned in numpy, one upload"""
    rp, col, val, y = m.export()
    slot = np.full(m.p, -1, np.int32)
    slot[cols] = np.arange(len(cols), dtype=np.int32)
    s_of = slot[col]
    sel = np.flatnonzero(s_of >= 0)
    s_sel, v_sel = s_of[sel], val[sel]
    edges = [_host_edges(v_sel[s_sel == s], bins) for s in range(len(cols))]
    width = np.ones(m.p, np.int64)
    width[cols] = np.array([len(e) for e in edges]) + 2
    base = np.zeros(m.p + 1, np.int64)
    np.cumsum(width, out=base[1:])
    ocol = base[col]
    for s, e in enumerate(edges):
        at = sel[s_sel == s]
        x = val[at]
        ocol[at] += np.where(np.isnan(x), len(e) + 1, np.searchsorted(e, x, side="right"))
    val[sel] = 1.0
    return engine.Matrix.from_csr(rp, ocol.astype(np.uint32), val, int(base[-1]), y)


def _shape(args, torch, which):
    from fmwr_amd import engine
    n = int(10_000_000 * args.n_scale)
    if which == "a":
        m = engine.Matrix.synthetic_fields(n, 13, engine.CRITEO_VOCAB, 3.0, 11)
        cols, bins, what = np.arange(13), 32, "synthetic_fields, 13 dense columns + 26 fields: the 13 dense columns at 32 bins"
    else:
        m = engine.Matrix.synthetic(n, 1_000_000, 30, 11).synthetic_values(5)
        cols, bins, what = np.sort(np.random.default_rng(3).choice(1_000_000, 8, replace=False)), 256, "configs[1]'s matrix after synthetic_values: 8 columns at 256 bins"

    def device():
        edges, _, _ = m.column_quantiles(cols, bins)
        out, _ = m.bin_columns(cols, edges)
        k = out.p
        out.close()
        return k

    def host():
        out = _host_route(engine, m, cols, bins)
        k = out.p
        out.close()
        return k
    routes = {"device": device, "host": host}
    edges, count, _ = m.column_quantiles(cols, bins)
    a, b = m.bin_columns(cols, edges)[0], _host_route(engine, m, cols, bins)
    ea, eb = a.export(), b.export()
    assert a.p == b.p and all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(ea, eb))
    a.close(); b.close()
    del ea, eb
    if torch is not None:
        rp, col, val, _ = m.export()
        t_col, t_val = torch.from_numpy(col.astype(np.int64)).cuda(), torch.from_numpy(val).cuda()
        t_cols = torch.from_numpy(np.asarray(cols, np.int64)).cuda()
        del rp, col, val

        def torch_route():
            slot = torch.full((m.p,), -1, dtype=torch.int64, device=t_col.device)
            slot[t_cols] = torch.arange(len(cols), device=t_col.device)
            s_of = slot[t_col]
            sel = torch.nonzero(s_of >= 0).squeeze(1)
            s_sel, v_sel = s_of[sel], t_val[sel]
            es = []
            for s in range(len(cols)):
                v = torch.sort(v_sel[s_sel == s])[0]
                v = v[~torch.isnan(v)]
                cand = torch.unique(v[(torch.arange(1, bins, device=v.device) * len(v)) // bins]) if len(v) else v
                es.append(cand[cand > v[0]] if len(v) else cand)
            width = torch.ones(m.p, dtype=torch.int64, device=t_col.device)
            width[t_cols] = torch.tensor([len(e) for e in es], device=t_col.device) + 2
            base = torch.cumsum(width, 0) - width
            ocol, oval = base[t_col], t_val.clone()
            for s, e in enumerate(es):
                at = sel[s_sel == s]
                x = t_val[at]
                ocol[at] += torch.where(torch.isnan(x), len(e) + 1, torch.bucketize(x, e, right=True))
            oval[sel] = 1.0
            torch.cuda.synchronize()
            return int(base[-1] + width[-1])
        assert torch_route() == device()
        routes["torch"] = torch_route
    out = _alternate(routes, args.reps)
    _verdict(out)

    def apply_only():
        o, _ = m.bin_columns(cols, edges)
        o.close()
    out["apply"] = _alternate({"apply": apply_only}, args.reps)["apply"]

    def fit_only():
        m.column_quantiles(cols, bins)
    out["fit"] = _alternate({"fit": fit_only}, args.reps)["fit"]
    # what the apply moves: every entry's column and value read and written, the row pointers and the labels copied
    out.update(rows=n, entries=m.nnz, features=m.p, binned_entries=int(count.sum()), apply_bytes=16 * m.nnz + 16 * (n + 1) + 8 * n, what=what)
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bins.json"))
    args = ap.parse_args()
    torch = None
    if not args.no_torch:
        import torch
        torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b"] if args.shape == "all" else args.shape.split(",")
    record = {"reps": args.reps, "n_scale": args.n_scale, "shapes": {}}
    for s in shapes:
        record["shapes"][s] = _shape(args, torch, s)
        print(s, json.dumps(record["shapes"][s]), flush=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    lines = ["value binning on the device against export -> numpy -> from_csr, and against torch on the same device (profiles/bins_bench.py; "
             "medians of %d alternated calls, [min, max]; rows scaled by %g)" % (args.reps, args.n_scale)]
    for s, o in record["shapes"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries ({o['binned_entries']:,} of them binned), {o['features']:,} features")
        for v in ("device", "host", "torch"):
            if v in o:
                lines.append(f"    {v:7s} {o[v]['median_s'] * 1e3:10.1f} ms  [{o[v]['min_s'] * 1e3:.1f}, {o[v]['max_s'] * 1e3:.1f}]")
        gate = "" if o["device_vs_host"] == "faster" else "  ** THE GATE IS MISSED **"
        lines.append(f"    host / device = {o['host_over_device']:.1f}x: the device route is {o['device_vs_host']}{gate}")
        if "torch" in o:
            lines.append(f"    torch / device = {o['torch_over_device']:.2f}x: the device route is {o['device_vs_torch']} (a comparison, not the gate)")
        lines.append(f"    the fit alone {o['fit']['median_s'] * 1e3:.1f} ms [{o['fit']['min_s'] * 1e3:.1f}, {o['fit']['max_s'] * 1e3:.1f}]; the apply alone "
                     f"{o['apply']['median_s'] * 1e3:.1f} ms [{o['apply']['min_s'] * 1e3:.1f}, {o['apply']['max_s'] * 1e3:.1f}]: it reads and writes "
                     f"{o['apply_bytes'] / 1e9:.2f} GB = {o['apply_bytes'] / o['apply']['median_s'] / 1e12:.2f} TB/s over the whole call (the allocation of the "
                     f"output, the slot table and the detector's pass included); profiles/take.txt's copy kernel moves 3.3 TB/s (a figure, not a gate)")
    txt = os.path.splitext(args.out)[0] + ".txt"
    kept = open(txt).read() if os.path.exists(txt) else ""
    kept = kept[kept.index("---- end to end"):] if "---- end to end" in kept else ""
    with open(txt, "w") as f:
        f.write("\n".join(lines) + "\n" + ("\n" + kept if kept else ""))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
