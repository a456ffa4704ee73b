"""The calibration calls measured against their own forward pass and against a torch formulation on the same device (the yardstick only, never a
product path) that is handed the raw scores for free.  Writes profiles/calibrate.json and a one-page profiles/calibrate.txt.

Shapes:
  a  pooled: configs[1]'s matrix, 10 M rows x 1 M features, 30 entries per row, k = 16, one group.
  b  grouped: MovieLens-20M-shaped one-hot rows, 20 M ratings of (user, item), 138 493 users as groups, k = 64.
Calls, per shape: fmx_reliability_device at 20 width bins, fmx_calibrate_isotonic_device at 1 024 mass bins, fmx_calibrate_platt_device with 8 steps.
Yardsticks (torch, no forward in their time):
  reliability  sigmoid, bucketize into the bins, index_add_ of the counts, the positives and p, the ECE from the table
  isotonic     argsort by score, stable argsort by group, run heads by cummax, the equal-mass bin, index_add_ of the counts and amin of the
               scores: the table only -- the pooling, which the library call includes, is left out in torch's favour
  platt        8 batched Newton steps: the five sums by index_add_ per step, the 2 x 2 solves vectorised over the groups
Per shape, in one process, after one warm-up call of every version, --reps rounds with the versions alternated (median, [min, max]).  A version
whose warm-up call takes more than 3 s is timed once, one that takes more than 20 s not again (its warm-up time stands, and the record says so).
Gate, as for the sibling entry points: faster than torch by more than the spread of either side; the record says so in bold if not.
--note adds a line to the record: the largest share of each test bar that tests/test_gpu_calibrate.py printed (-s) goes in that way."""
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


SLOW_S, STUCK_S = 3.0, 20.0   # a version whose warm-up call takes longer is timed once / not again (the record says which)


def _alternate(versions, reps):
    ts = {v: [] for v in versions}
    warm = {}
    for v, fn in versions.items():   # warm-up; its time is printed at once, so that a slow version shows
        t = time.perf_counter(); fn(); warm[v] = time.perf_counter() - t
        print(f"  warm-up {v}: {warm[v]:.3f} s", file=sys.stderr, flush=True)
    for r in range(reps):            # alternated: one call of each version per round
        for v, fn in versions.items():
            if warm[v] > STUCK_S or (warm[v] > SLOW_S and r > 0):
                continue
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    out = {}
    for v, t in ts.items():
        out[v] = _stats(t if t else [warm[v]])
        if not t:
            out[v]["warm_up_only"] = True
    return out


def _verdict(out, ours, other):
    spread = max(out[other]["max_s"] - out[other]["min_s"], out[ours]["max_s"] - out[ours]["min_s"])
    gap = out[other]["median_s"] - out[ours]["median_s"]
    out[f"{other}_over_{ours}"] = out[other]["median_s"] / out[ours]["median_s"]
    out[f"{ours}_vs_{other}"] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _torch_reliability(torch, z, pos, grp, G, B):
    p = torch.sigmoid(z)
    cell = grp * B + torch.clamp((p * B).floor().long(), 0, B - 1)
    rows = torch.zeros(G * B, dtype=torch.int64, device=z.device).index_add_(0, cell, torch.ones_like(cell))
    npos = torch.zeros(G * B, dtype=torch.int64, device=z.device).index_add_(0, cell, pos)
    sp = torch.zeros(G * B, dtype=torch.float64, device=z.device).index_add_(0, cell, p)
    r = rows.view(G, B).double()
    gap = ((sp.view(G, B) - npos.view(G, B).double()) / r.clamp(min=1)).abs()
    return rows, (r / r.sum(1, keepdim=True).clamp(min=1) * gap).sum(1)


def _torch_mass_table(torch, z, pos, grp, G, B):
    n = z.numel()
    o1 = torch.sort(z, stable=True).indices
    o2 = torch.sort(grp[o1], stable=True).indices
    o = o1[o2]
    zs, gs = z[o], grp[o]
    idx = torch.arange(n, device=z.device)
    head = torch.ones(n, dtype=torch.bool, device=z.device)
    head[1:] = (gs[1:] != gs[:-1]) | (zs[1:] != zs[:-1])
    rh = torch.cummax(torch.where(head, idx, torch.zeros_like(idx)), 0).values
    first = torch.searchsorted(gs, torch.arange(G + 1, device=z.device))
    s = (first[1:] - first[:-1])[gs]
    cell = gs * B + (rh - first[gs]) * B // s
    rows = torch.zeros(G * B, dtype=torch.int64, device=z.device).index_add_(0, cell, torch.ones_like(cell))
    npos = torch.zeros(G * B, dtype=torch.int64, device=z.device).index_add_(0, cell, pos[o])
    lo = torch.full((G * B,), float("inf"), dtype=torch.float64, device=z.device).scatter_reduce_(0, cell, zs, "amin")
    return rows, npos, lo


def _torch_platt(torch, z, y, grp, G, lam, steps):
    a = torch.ones(G, dtype=torch.float64, device=z.device)
    b = torch.zeros(G, dtype=torch.float64, device=z.device)

    def per_group(v):
        return torch.zeros(G, dtype=torch.float64, device=z.device).index_add_(0, grp, v)
    for _ in range(steps):
        m = y * (a[grp] * z + b[grp])
        ng = torch.sigmoid(-m)
        w, d = torch.sigmoid(m) * ng, -y * ng
        g0, g1 = per_group(d * z) + lam * (a - 1), per_group(d) + lam * b
        h00, h01, h11 = per_group(w * z * z) + lam, per_group(w * z), per_group(w) + lam
        det = h00 * h11 - h01 * h01
        a, b = a - (h11 * g0 - h01 * g1) / det, b - (h00 * g1 - h01 * g0) / det
    return a, b


def run_shape(torch, name, m, y, e, n, G, g32, iso_bins, reps):
    from fmwr_amd import _lib as L
    B, S = 20, iso_bins
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")   # noqa: E731
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device="cuda")     # noqa: E731
    count, sum_p, lo, hi, nan_rows, value = i64(G, B, 2), f64(G, B), f64(G, B), f64(G, B), i64(G), f64(G, 4)
    ab, rows, status = f64(G, 2), i64(G), torch.empty(G, dtype=torch.int32, device="cuda")
    n_steps, thr, val = torch.empty(G, dtype=torch.int32, device="cuda"), f64(G, S), f64(G, S)
    z = f64(n)
    import ctypes as C
    dg = None if g32 is None else g32.data_ptr()

    def forward():
        L.check(L.lib().fmx_predict_device(e.h, m.h, C.c_int64(0), C.c_int64(n), C.c_void_p(z.data_ptr()), C.c_int(L.LINK_NONE))); e.sync()

    forward()
    pos = torch.from_numpy((y > 0).astype(np.int64)).cuda()
    ypm = torch.from_numpy(np.where(y > 0, 1.0, -1.0)).cuda()
    g64 = torch.zeros(n, dtype=torch.int64, device="cuda") if g32 is None else g32.long()
    res = {}

    def reliability():
        e.reliability_device(m, 0, n, dg, G, B, L.BINS_WIDTH, count.data_ptr(), sum_p.data_ptr(), lo.data_ptr(), hi.data_ptr(), nan_rows.data_ptr(), value.data_ptr()); e.sync()

    def isotonic():
        e.calibrate_isotonic_device(m, 0, n, dg, G, S, n_steps.data_ptr(), thr.data_ptr(), val.data_ptr()); e.sync()

    def platt():
        e.calibrate_platt_device(m, 0, n, dg, G, 0.1, 8, ab.data_ptr(), rows.data_ptr(), status.data_ptr()); e.sync()

    def torch_reliability():
        res["rel"] = _torch_reliability(torch, z, pos, g64, G, B); torch.cuda.synchronize()

    def torch_isotonic():
        res["iso"] = _torch_mass_table(torch, z, pos, g64, G, S); torch.cuda.synchronize()

    def torch_platt():
        res["platt"] = _torch_platt(torch, z, ypm, g64, G, 0.1, 8); torch.cuda.synchronize()

    out = {"case": name, "rows": n, "p": int(e.p), "k": int(e.cfg.num_factor), "groups": G, "iso_bins": S}
    out.update(_alternate({"forward": forward, "reliability": reliability, "isotonic": isotonic, "platt": platt, "torch_reliability": torch_reliability,
                           "torch_isotonic": torch_isotonic, "torch_platt": torch_platt}, reps))
    for call in ("reliability", "isotonic", "platt"):
        _verdict(out, call, "torch_" + call)
    out["counts_equal_to_torch"] = bool((res["rel"][0].view(G, B) == count[:, :, 0]).all().item())
    out["ece_max_abs_diff_to_torch"] = float((res["rel"][1] - value[:, 0]).abs().nan_to_num(0.0).max().item())
    solved = status == 0
    out["platt_max_abs_diff_to_torch"] = float((res["platt"][0][solved] - ab[solved, 0]).abs().nan_to_num(0.0).max().item()) if bool(solved.any()) else None
    out["platt_unsolved_groups"] = int((~solved).sum().item())
    print(json.dumps(out), flush=True)
    return out


def _engine(p, k):
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_CLASSIFICATION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    return e


def _labels(m, seed):
    rng = np.random.default_rng(seed)
    y = np.where(rng.random(m.n) < 0.25, 1.0, -1.0)
    m.set_labels(y)
    return y


def write_txt(rec, path):
    ms = lambda s: (f"{1e3 * s['median_s']:10.3f} ms [{1e3 * s['min_s']:.3f}, {1e3 * s['max_s']:.3f}]" + (f" ({s['reps']} call(s))" if s["reps"] != rec["reps"] else "")  # noqa: E731
                    + (" (the warm-up call only)" if s.get("warm_up_only") else ""))
    lines = ["calibration record (profiles/calibrate_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        lines.append(f"{o['case']}: {o['rows']} rows, p {o['p']}, k {o['k']}, {o['groups']} group(s)")
        lines.append(f"  forward alone          {ms(o['forward'])}")
        for call, what in (("reliability", "20 width bins"), ("isotonic", f"{o['iso_bins']} mass bins"), ("platt", "8 Newton steps")):
            verdict = o[f"{call}_vs_torch_{call}"]
            lines.append(f"  {call:<12} ({what}) {ms(o[call])}   {o['rows'] / o[call]['median_s'] / 1e6:.1f} M rows/s")
            lines.append(f"    torch (no forward)   {ms(o['torch_' + call])}   = {o[f'torch_{call}_over_{call}']:.2f}x the call")
            lines.append("    gate: faster than torch by more than the spread" if verdict == "faster" else f"    **gate missed: the call is {verdict} against torch**")
        lines.append(f"  counts equal to torch's: {o['counts_equal_to_torch']}; ECE within {o['ece_max_abs_diff_to_torch']:.3g} of torch's; "
                     f"Platt a within {o['platt_max_abs_diff_to_torch']} of torch's ({o['platt_unsolved_groups']} unsolved group(s))")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b in the order to run them; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibrate.json"))
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    from fmwr_amd import engine
    shapes = ["a", "b"] if args.shape == "all" else args.shape.split(",")
    rec = {"script": "profiles/calibrate_bench.py", "reps": args.reps, "cases": [], "notes": args.note}

    def save():   # after every shape: a later shape that is cut short does not lose the earlier ones
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(rec, open(args.out, "w"), indent=1)
        write_txt(rec, args.out.replace(".json", ".txt"))

    for shape in shapes:
        if shape == "a":
            n, p = int(10_000_000 * args.n_scale), 1_000_000
            m = engine.Matrix.synthetic(n, p, 30, 11).synthetic_values(12)
            y = _labels(m, 5)
            rec["cases"].append(run_shape(torch, "a_pooled_configs1", m, y, _engine(p, 16), n, 1, None, 1024, args.reps))
        else:
            n, users, items = int(20_000_263 * args.n_scale), 138_493, 26_744
            rng = np.random.default_rng(3)
            user = rng.integers(0, users, n)
            col = np.stack([user, users + rng.integers(0, items, n)], 1).ravel().astype(np.uint32)
            m = engine.Matrix.from_csr(np.arange(0, 2 * n + 1, 2, dtype=np.int64), col, np.ones(2 * n, np.float32), users + items)
            y = _labels(m, 6)
            g32 = torch.from_numpy(user.astype(np.int32)).cuda()   # the same bits as uint32
            rec["cases"].append(run_shape(torch, "b_grouped_movielens20m", m, y, _engine(users + items, 64), n, users, g32, 1024, args.reps))
        m.close()
        save()


if __name__ == "__main__":
    main()
