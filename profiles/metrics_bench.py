"""fmx_metrics_device measured against fmx_evaluate (the reference's AUC and LL, one call each) and against a torch formulation of the grouped AUC on
the same device and the same scores (the yardstick only, never a product path).  Writes profiles/metrics.json and a one-page profiles/metrics.txt.

Shapes:
  a  pooled: configs[1]'s matrix, 10 M rows x 1 M features, 30 entries per row, k = 16, CLASSIFICATION, one group.  Against
     fmx_evaluate(FMX_EVAL_AUC) + fmx_evaluate(FMX_EVAL_LL): both sides run one forward pass per call (fmx_evaluate: two calls, two passes) and a
     64-bit sort of n keys.
  b  grouped: MovieLens-20M-shaped one-hot rows, 20 M ratings of (user, item), 138 493 users as groups, k = 64.  Against torch: a stable sort by
     score, a stable sort by group, segmented cumulative counts of the negatives with ties resolved by run heads (the global form's own algorithm,
     on torch tensors), from raw scores torch is handed for free (its time holds NO forward pass; the library call's does, and the forward alone is
     timed beside them).
  c  the wave form alone: Criteo-shaped rows (13 dense + 26 one-hot fields, vocabularies capped), 1 M rows in groups of about 8, k = 16.  Reports
     rows/s; the wave-form kernel's share of the wall comes from a separate `rocprofv3 --kernel-trace --stats` run of `--shape c` (kernel
     mt_pairs_wave_k), never from this script's clock.
Per shape, in one process, after one warm-up call of every version, --reps rounds with the versions alternated (median, [min, max]).
Gate of shape b, as for the sibling entry points: faster than torch by more than the spread of either side; the record says so in bold if not."""
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
    for _ in range(reps):          # alternated: one call of each version per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out, ours, other):
    spread = max(out[other]["max_s"] - out[other]["min_s"], out[ours]["max_s"] - out[ours]["min_s"])
    gap = out[other]["median_s"] - out[ours]["median_s"]
    out[f"{other}_over_{ours}"] = out[other]["median_s"] / out[ours]["median_s"]
    out[f"{ours}_vs_{other}"] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _engine(p, k):
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_CLASSIFICATION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    return e


def _forward(e, m, n, ptr):
    """the raw scores of rows [0, n) into a device buffer"""
    import ctypes as C
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_predict_device(e.h, m.h, C.c_int64(0), C.c_int64(n), C.c_void_p(ptr), C.c_int(L.LINK_NONE)))
    e.sync()


def _labels(m, seed):
    rng = np.random.default_rng(seed)
    m.set_labels(np.where(rng.random(m.n) < 0.25, 1.0, -1.0))


def _torch_grouped_pairs2(torch, z, neg, grp, G):
    """pairs2 per group from raw scores, negative flags (int64 0/1) and group ids (int64), all on the device"""
    n = z.numel()
    o1 = torch.sort(z, stable=True).indices
    o2 = torch.sort(grp[o1], stable=True).indices
    o = o1[o2]
    zs, ns, gs = z[o], neg[o], grp[o]
    idx = torch.arange(n, device=z.device)
    head = torch.ones(n, dtype=torch.bool, device=z.device)
    head[1:] = (gs[1:] != gs[:-1]) | (zs[1:] != zs[:-1])
    rh = torch.cummax(torch.where(head, idx, torch.zeros_like(idx)), 0).values
    before = torch.cumsum(ns, 0) - ns                                    # negatives before position i
    ghead = torch.searchsorted(gs, torch.arange(G, device=z.device))     # first position of every group
    gh = ghead[gs]
    c = torch.where(ns == 1, (idx - before) - (rh - before[rh]), 2 * (before[rh] - before[gh]) + (before - before[rh]))
    return torch.zeros(G, dtype=torch.int64, device=z.device).index_add_(0, gs, c)


def run_pooled(torch, n, reps):
    from fmwr_amd import _lib as L, engine
    p, k = 1_000_000, 16
    m = engine.Matrix.synthetic(n, p, 30, 11).synthetic_values(12)
    _labels(m, 5)
    e = _engine(p, k)
    val = torch.empty(6, dtype=torch.float64, device="cuda")
    cnt = torch.empty(4, dtype=torch.int64, device="cuda")
    zbuf = torch.empty(n, dtype=torch.float64, device="cuda")
    res = {}

    def metrics():
        e.metrics_device(m, 0, n, None, 1, val.data_ptr(), cnt.data_ptr(), L.LINK_LOGISTIC); e.sync()

    def evaluate_auc_ll():
        res["auc"] = e.evaluate(m, L.EVAL_AUC); res["ll"] = e.evaluate(m, L.EVAL_LL)

    def forward():
        _forward(e, m, n, zbuf.data_ptr())

    out = {"case": "a_pooled_configs1", "rows": n, "p": p, "k": k, "groups": 1}
    out.update(_alternate({"metrics": metrics, "evaluate_auc_ll": evaluate_auc_ll, "forward": forward}, reps))
    _verdict(out, "metrics", "evaluate_auc_ll")
    out["rows_per_s"] = n / out["metrics"]["median_s"]
    v = val.cpu().numpy()
    out["auc"], out["reference_auc"] = float(v[0]), res["auc"]
    out["logloss"], out["reference_ll_over_rows"] = float(v[1]), -res["ll"] / n   # LL = (sum of (1 + y) log p + (1 - y) log(1 - p)) / 2: the summed log-likelihood
    print(json.dumps(out), flush=True)
    m.close()
    return out


def run_grouped(torch, n, reps):
    from fmwr_amd import _lib as L, engine
    users, items, k = 138_493, 26_744, 64
    rng = np.random.default_rng(3)
    user = rng.integers(0, users, n)
    col = np.stack([user, users + rng.integers(0, items, n)], 1).ravel().astype(np.uint32)
    m = engine.Matrix.from_csr(np.arange(0, 2 * n + 1, 2, dtype=np.int64), col, np.ones(2 * n, np.float32), users + items)
    _labels(m, 6)
    e = _engine(users + items, k)
    g32 = torch.from_numpy(user.astype(np.int32)).cuda()   # the same bits as uint32
    g64 = g32.long()
    val = torch.empty((users, 6), dtype=torch.float64, device="cuda")
    cnt = torch.empty((users, 4), dtype=torch.int64, device="cuda")
    z = torch.empty(n, dtype=torch.float64, device="cuda")
    _forward(e, m, n, z.data_ptr())
    _, _, _, y = m.export()
    neg = torch.from_numpy((~(y > 0)).astype(np.int64)).cuda()
    res = {}

    def metrics():
        e.metrics_device(m, 0, n, g32.data_ptr(), users, val.data_ptr(), cnt.data_ptr(), L.LINK_LOGISTIC); e.sync()

    def forward():
        _forward(e, m, n, z.data_ptr())

    def torch_():
        res["pairs2"] = _torch_grouped_pairs2(torch, z, neg, g64, users); torch.cuda.synchronize()

    out = {"case": "b_grouped_movielens20m", "rows": n, "p": users + items, "k": k, "groups": users}
    out.update(_alternate({"metrics": metrics, "torch": torch_, "forward": forward}, reps))
    _verdict(out, "metrics", "torch")
    out["rows_per_s"] = n / out["metrics"]["median_s"]
    out["pairs2_equal_to_torch"] = bool((res["pairs2"] == cnt[:, 2]).all().item())
    print(json.dumps(out), flush=True)
    m.close()
    return out


def run_wave(torch, n, reps, vocab_cap):
    from fmwr_amd import _lib as L, engine
    vocab = [min(v, vocab_cap) for v in engine.CRITEO_VOCAB]
    p = 13 + int(sum(vocab))
    m = engine.Matrix.synthetic_fields(n, 13, vocab, 3.0, 77)
    _labels(m, 7)
    e = _engine(p, 16)
    G = n // 8
    g32 = torch.from_numpy(np.random.default_rng(8).integers(0, G, n).astype(np.int32)).cuda()
    val = torch.empty((G, 6), dtype=torch.float64, device="cuda")
    cnt = torch.empty((G, 4), dtype=torch.int64, device="cuda")
    zbuf = torch.empty(n, dtype=torch.float64, device="cuda")

    def metrics():
        e.metrics_device(m, 0, n, g32.data_ptr(), G, val.data_ptr(), cnt.data_ptr(), L.LINK_LOGISTIC); e.sync()

    def forward():
        _forward(e, m, n, zbuf.data_ptr())

    out = {"case": "c_wave_criteo", "rows": n, "p": p, "k": 16, "groups": G, "vocab_cap": vocab_cap}
    out.update(_alternate({"metrics": metrics, "forward": forward}, reps))
    out["rows_per_s"] = n / out["metrics"]["median_s"]
    out["largest_group"] = int(cnt[:, 0].max().item())
    print(json.dumps(out), flush=True)
    m.close()
    return out


def write_txt(rec, path):
    ms = lambda s: f"{1e3 * s['median_s']:10.3f} ms [{1e3 * s['min_s']:.3f}, {1e3 * s['max_s']:.3f}]"  # noqa: E731
    lines = ["fmx_metrics record (profiles/metrics_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        lines.append(f"{o['case']}: {o['rows']} rows, p {o['p']}, k {o['k']}, {o['groups']} group(s)")
        lines.append(f"  metrics          {ms(o['metrics'])}   {o['rows_per_s'] / 1e6:.1f} M rows/s")
        lines.append(f"  forward alone    {ms(o['forward'])}")
        if "evaluate_auc_ll" in o:
            lines.append(f"  evaluate AUC+LL  {ms(o['evaluate_auc_ll'])}   = {o['evaluate_auc_ll_over_metrics']:.2f}x metrics (metrics is {o['metrics_vs_evaluate_auc_ll']})")
            lines.append(f"  AUC {o['auc']:.6f} (reference's max(a, 1 - a): {o['reference_auc']:.6f}); log loss {o['logloss']:.6f} (from the reference's LL: {o['reference_ll_over_rows']:.6f})")
        if "torch" in o:
            verdict = o["metrics_vs_torch"]
            lines.append(f"  torch (no forward) {ms(o['torch'])}   = {o['torch_over_metrics']:.2f}x metrics; pairs2 equal to torch's: {o['pairs2_equal_to_torch']}")
            lines.append("  gate: metrics is faster than torch by more than the spread" if verdict == "faster" else f"  **gate missed: metrics is {verdict} against torch**")
        if "largest_group" in o:
            lines.append(f"  largest group {o['largest_group']} rows")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b, c; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--vocab-cap", type=int, default=400_000, help="shape c: no field holds more ids than this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics.json"))
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b", "c"] if args.shape == "all" else args.shape.split(",")
    rec = {"script": "profiles/metrics_bench.py", "reps": args.reps, "cases": [], "notes": args.note}
    if "a" in shapes:
        rec["cases"].append(run_pooled(torch, int(10_000_000 * args.n_scale), args.reps))
    if "b" in shapes:
        rec["cases"].append(run_grouped(torch, int(20_000_263 * args.n_scale), args.reps))
    if "c" in shapes:
        rec["cases"].append(run_wave(torch, int(1_000_000 * args.n_scale), args.reps, args.vocab_cap))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
