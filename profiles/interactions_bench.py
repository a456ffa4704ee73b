"""fmx_interactions_device and fmx_interactions_summary measured against a torch formulation on the same device and the same rows (the
yardstick only, never a product path) and against fmx_contrib_device on the same matrix (the cost of one gather pass over it).  Writes
profiles/interactions.json and a one-page profiles/interactions.txt.

Shapes:
  a  configs[1]'s matrix: 10 M rows x 1 M features, 30 entries per row (values in (0, 1)), k = 16, top_m = 5, fp32 tables; torch and the
     call it is compared with run on the first --torch-rows rows (the whole matrix is timed too)
  b  MovieLens-20M-shaped one-hot rows: 20 M ratings of (user, item), 138 493 users + 26 744 items, k = 64, top_m = 5 (one pair per row)
  c  the summary on Criteo-shaped rows: 13 dense + 26 one-hot fields (engine.CRITEO_VOCAB, every vocabulary capped at --vocab-cap ids),
     39 groups, k = 16, --summary-rows rows
Per shape, in one process, after one warm-up call of every version, --reps rounds with the versions alternated (median, [min, max]):
  interactions / summary   the library call, ended by a device synchronise (the summary includes its copy of the tables to the host)
  contrib                  fmx_contrib_device over the same rows
  torch                    per chunk of rows: T = V[col] * x (fp64), I = bmm(T, T^T), topk of |I| over the triangle a < b -- for the summary
                           index_add_ of I and |I| over the triangle into the G x G cells
No threshold is set: the record states the ratios and the spread, and says where the library is the slower one.
"""
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
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, task=L.TASK_REGRESSION, batch_rows=4096)
    e.init_normal(7, 0.0, 0.1)
    return e


def _torch_rows(torch, e, m, rows, fixed_len):
    """the device tensors of the first `rows` rows: V [p][k] fp64, col [rows][len] int64, x [rows][len] fp64"""
    _, _, v = e.get_params()
    V = torch.from_numpy(np.ascontiguousarray(v.T)).cuda()
    _, col, val, _ = m.export(0, rows)
    col_d = torch.from_numpy(col.astype(np.int64)).cuda().view(rows, fixed_len)
    val_d = torch.from_numpy(val).cuda().double().view(rows, fixed_len)
    return V, col_d, val_d


def run_top(torch, name, m, p, k, fixed_len, top_m, torch_rows, reps, chunk=1 << 17):
    e = _engine(p, k)
    n = m.n
    torch_rows = min(torch_rows, n)
    oa = torch.empty((n, top_m), dtype=torch.int64, device="cuda")
    ob = torch.empty((n, top_m), dtype=torch.int64, device="cuda")
    ov = torch.empty((n, top_m), dtype=torch.float64, device="cuda")
    phi = torch.empty(m.nnz, dtype=torch.float64, device="cuda")
    V, col_d, val_d = _torch_rows(torch, e, m, torch_rows, fixed_len)
    ia, ib = torch.triu_indices(fixed_len, fixed_len, 1, device="cuda")
    tv = torch.empty((torch_rows, min(top_m, len(ia))), dtype=torch.float64, device="cuda")

    def interactions(rows=n):
        e.interactions_device(m, 0, rows, top_m, oa.data_ptr(), ob.data_ptr(), ov.data_ptr()); e.sync()

    def contrib(rows=n):
        e.contrib_device(m, 0, rows, phi.data_ptr()); e.sync()

    def torch_():
        for r0 in range(0, torch_rows, chunk):
            r1 = min(torch_rows, r0 + chunk)
            T = V[col_d[r0:r1]] * val_d[r0:r1, :, None]
            I = torch.bmm(T, T.transpose(1, 2))[:, ia, ib]
            idx = torch.topk(I.abs(), tv.shape[1], dim=1).indices
            tv[r0:r1] = torch.gather(I, 1, idx)
        torch.cuda.synchronize()

    out = {"case": name, "rows": n, "entries_per_row": fixed_len, "p": p, "k": k, "top_m": top_m, "torch_rows": torch_rows}
    out.update(_alternate({"interactions": interactions, "contrib": contrib}, reps))
    _verdict(out, "interactions", "contrib")
    out["pairs_per_s"] = n * (fixed_len * (fixed_len - 1) // 2) / out["interactions"]["median_s"]
    sub = _alternate({"interactions": lambda: interactions(torch_rows), "contrib": lambda: contrib(torch_rows), "torch": torch_}, reps)
    _verdict(sub, "interactions", "torch")
    out["first_rows"] = sub
    interactions(torch_rows)
    out["rows_where_torch_finds_the_same_values"] = float(((tv.abs() - ov[:torch_rows, :tv.shape[1]].abs()).abs() <= 1e-9 * (1 + tv.abs())).all(1).double().mean().item())
    print(json.dumps(out), flush=True)
    return out


def run_summary(torch, rows, k, reps, vocab_cap, chunk=1 << 16):
    from fmwr_amd import engine
    vocab = [min(v, vocab_cap) for v in engine.CRITEO_VOCAB]   # the larger vocabularies capped: the torch side holds V in fp64
    n_dense, G = 13, 13 + len(vocab)
    p = n_dense + int(sum(vocab))
    m = engine.Matrix.synthetic_fields(rows, n_dense, vocab, 3.0, 77)
    groups = np.concatenate([np.arange(n_dense), np.repeat(n_dense + np.arange(len(vocab)), vocab)]).astype(np.uint32)
    e = _engine(p, k)
    phi = torch.empty(m.nnz, dtype=torch.float64, device="cuda")
    V, col_d, val_d = _torch_rows(torch, e, m, rows, G)
    grp_d = torch.from_numpy(groups.astype(np.int64)).cuda()
    ia, ib = torch.triu_indices(G, G, 1, device="cuda")
    res = {}

    def summary():
        res["ours"] = e.interactions_summary(m, groups, G)

    def contrib():
        e.contrib_device(m, 0, rows, phi.data_ptr()); e.sync()

    def torch_():
        s = torch.zeros(G * G, dtype=torch.float64, device="cuda")
        ab = torch.zeros(G * G, dtype=torch.float64, device="cuda")
        for r0 in range(0, rows, chunk):
            r1 = min(rows, r0 + chunk)
            T = V[col_d[r0:r1]] * val_d[r0:r1, :, None]
            I = torch.bmm(T, T.transpose(1, 2))[:, ia, ib].reshape(-1)
            g = grp_d[col_d[r0:r1]]
            cell = (g[:, ia] * G + g[:, ib]).reshape(-1)
            s.index_add_(0, cell, I)
            ab.index_add_(0, cell, I.abs())
        res["torch"] = (s.cpu().numpy().reshape(G, G), ab.cpu().numpy().reshape(G, G))

    out = {"case": "c_criteo_summary", "rows": rows, "entries_per_row": G, "p": p, "k": k, "groups": G, "vocab_cap": vocab_cap}
    out.update(_alternate({"summary": summary, "contrib": contrib, "torch": torch_}, reps))
    _verdict(out, "summary", "torch")
    _verdict(out, "summary", "contrib")
    out["pairs_per_s"] = rows * (G * (G - 1) // 2) / out["summary"]["median_s"]
    ts = res["torch"][0]
    out["max_rel_diff_vs_torch"] = float(np.max(np.abs(np.triu(res["ours"]["sum"], 1) - np.triu(ts + ts.T, 1)) / np.maximum(np.triu(res["ours"]["abs_sum"], 1), 1e-300)))
    print(json.dumps(out), flush=True)
    return out


def write_txt(rec, path):
    ms = lambda s: f"{1e3 * s['median_s']:10.3f} ms [{1e3 * s['min_s']:.3f}, {1e3 * s['max_s']:.3f}]"  # noqa: E731
    lines = ["fmx_interactions record (profiles/interactions_bench.py); times: median of %d alternated calls after one warm-up, [min, max]" % rec["reps"], ""]
    for o in rec["cases"]:
        if o["case"] == "c_criteo_summary":
            lines.append(f"{o['case']}: {o['rows']} rows x {o['entries_per_row']} entries, p {o['p']} (vocabularies capped at {o['vocab_cap']}), k {o['k']}, {o['groups']} groups")
            lines.append(f"  summary      {ms(o['summary'])}   {o['pairs_per_s'] / 1e9:.2f} G pairs/s")
            lines.append(f"  torch        {ms(o['torch'])}   = {o['torch_over_summary']:.2f}x summary (the summary is {o['summary_vs_torch']}); "
                         f"max |sum diff| / abs_sum {o['max_rel_diff_vs_torch']:.1e}")
            lines.append(f"  contrib      {ms(o['contrib'])}   = {o['contrib_over_summary']:.2f}x summary")
            continue
        lines.append(f"{o['case']}: {o['rows']} rows x {o['entries_per_row']} entries, p {o['p']}, k {o['k']}, top_m {o['top_m']}")
        lines.append(f"  interactions {ms(o['interactions'])}   {o['pairs_per_s'] / 1e9:.2f} G pairs/s")
        lines.append(f"  contrib      {ms(o['contrib'])}   = {o['contrib_over_interactions']:.2f}x interactions")
        f = o["first_rows"]
        lines.append(f"  first {o['torch_rows']} rows:")
        lines.append(f"    interactions {ms(f['interactions'])}")
        lines.append(f"    contrib      {ms(f['contrib'])}")
        lines.append(f"    torch        {ms(f['torch'])}   = {f['torch_over_interactions']:.2f}x interactions (interactions is {f['interactions_vs_torch']}); "
                     f"rows with the same |values| to 1e-9: {o['rows_where_torch_finds_the_same_values'] * 100:.2f} %")
    if rec.get("notes"):
        lines += [""] + rec["notes"]
    open(path, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b, c; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of a and b (quick checks)")
    ap.add_argument("--torch-rows", type=int, default=1_000_000)
    ap.add_argument("--summary-rows", type=int, default=1_000_000)
    ap.add_argument("--vocab-cap", type=int, default=400_000, help="shape c: no field holds more ids than this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interactions.json"))
    ap.add_argument("--note", action="append", default=[], help="a line for the record's notes")
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    from fmwr_amd import engine
    shapes = ["a", "b", "c"] if args.shape == "all" else args.shape.split(",")
    rec = {"script": "profiles/interactions_bench.py", "reps": args.reps, "cases": [], "notes": args.note}
    if "a" in shapes:
        n, p = int(10_000_000 * args.n_scale), 1_000_000
        m = engine.Matrix.synthetic(n, p, 30, 11).synthetic_values(12)
        rec["cases"].append(run_top(torch, "a_configs1", m, p, 16, 30, 5, args.torch_rows, args.reps))
        m.close()
    if "b" in shapes:
        users, items = 138_493, 26_744
        n = int(20_000_263 * args.n_scale)
        rng = np.random.default_rng(3)
        col = np.stack([rng.integers(0, users, n), users + rng.integers(0, items, n)], 1).ravel().astype(np.uint32)
        m = engine.Matrix.from_csr(np.arange(0, 2 * n + 1, 2, dtype=np.int64), col, np.ones(2 * n, np.float32), users + items)
        rec["cases"].append(run_top(torch, "b_movielens20m", m, users + items, 64, 2, 5, args.torch_rows, args.reps))
        m.close()
    if "c" in shapes:
        rec["cases"].append(run_summary(torch, args.summary_rows, 16, args.reps, args.vocab_cap))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(rec, open(args.out, "w"), indent=1)
    write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
