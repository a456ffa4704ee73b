"""fmx_fold_in_pairs measured against a torch formulation on the same device (the yardstick only, never the product path).  Writes
profiles/foldin_pairs.json and appends a section to profiles/foldin_pairs.txt.  Runs of one k per process are joined with --merge.

Shape: MovieLens-20M -- 138 493 one-hot user columns, 26 744 one-hot item columns, 20 M positives (user, item) with n_neg = 1: 20 M pairs,
40 M rows (user, positive) / (user, negative), item popularity and user activity drawn from a power law, negatives uniform.  EVERY user is
folded in one call against the items' rows of an untrained model (V ~ N(0, 0.1)), at k = 16 and k = 64, 8 Newton steps, fp32 tables.
Per case, alternated inside one process after one warm-up call each, --reps rounds (median, [min, max]):
  fold_in_pairs  Engine.fold_in_pairs(apply = False): find, pair keys, sort, pair pass, Gram, solve, results to the host
  torch          the same solve in fp64 torch on difference vectors: Z = (0, v_i - v_j), B = w_i - w_j, per-group Gram matrices by index_add_
                 of the pairs' outer products (chunked to bound memory), torch.linalg.cholesky + cholesky_solve, eight times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NU, NI, N = 138_493, 26_744, 20_000_000


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def make_pairs(n, seed=3):
    rng = np.random.default_rng(seed)
    pu = rng.pareto(1.2, NU) + 1.0
    pi = rng.pareto(1.0, NI) + 1.0
    users = rng.choice(NU, n, p=pu / pu.sum()).astype(np.uint32)
    pos = rng.choice(NI, n, p=pi / pi.sum()).astype(np.uint32)
    neg = rng.integers(0, NI, n).astype(np.uint32)
    return users, pos, neg


def torch_fold(torch, users, pos, neg, w_items, v_items, lam, steps, chunk):
    """theta [NU][1 + k] in fp64 from Z = (0, v_pos - v_neg), B = w_pos - w_neg; Gram by index_add_ of outer products"""
    k = v_items.shape[1]
    D = 1 + k
    theta = torch.zeros((NU, D), dtype=torch.float64, device="cuda")
    eye = torch.diag(torch.full((D,), lam, dtype=torch.float64, device="cuda"))
    for _ in range(steps):
        H = torch.zeros((NU, D, D), dtype=torch.float64, device="cuda")
        rhs = torch.zeros((NU, D), dtype=torch.float64, device="cuda")
        for c0 in range(0, len(users), chunk):
            u, i, j = users[c0:c0 + chunk], pos[c0:c0 + chunk], neg[c0:c0 + chunk]
            z = torch.cat([torch.zeros((len(u), 1), dtype=torch.float64, device="cuda"), v_items[i] - v_items[j]], dim=1)
            d = w_items[i] - w_items[j] + (z * theta[u]).sum(1)
            sg = torch.sigmoid(d)
            H.index_add_(0, u, (z * (sg * (1 - sg))[:, None]).unsqueeze(2) * z.unsqueeze(1))
            rhs.index_add_(0, u, z * (1 - sg)[:, None])
        rhs -= lam * theta
        L = torch.linalg.cholesky(H + eye)
        theta = theta + torch.cholesky_solve(rhs.unsqueeze(2), L).squeeze(2)
    return theta


def run_case(torch, k, reps, n, only=None):
    from fmwr_amd import _lib as L, engine
    p = NU + NI
    users, pos, neg = make_pairs(n)
    col = np.stack([users, pos + NU, users, neg + NU], 1).ravel().astype(np.uint32)
    m = engine.Matrix.from_csr(np.arange(2 * n + 1, dtype=np.int64) * 2, col, np.ones(4 * n, np.float32), p)
    del col
    e = engine.Engine(p, mode=L.MODE_MINIBATCH, num_factor=k, batch_rows=4096, task=L.TASK_RANKING)
    e.init_normal(7, 0.0, 0.1)
    w0, w, v = e.get_params()
    w = np.random.default_rng(11).normal(0, 0.1, p).astype(np.float32).astype(np.float64)   # (init_normal leaves w = 0: B would vanish)
    e.set_params(0.0, w, v)
    ids = np.arange(NU, dtype=np.uint32)
    res = {}

    def fold():
        res["f"] = e.fold_in_pairs(m, ids, 0.1, 0.1, newton_steps=8)

    versions = {"fold_in_pairs": fold}
    if only != "fold_in_pairs":
        t_users = torch.tensor(users.astype(np.int64), device="cuda")
        t_pos = torch.tensor(pos.astype(np.int64), device="cuda")
        t_neg = torch.tensor(neg.astype(np.int64), device="cuda")
        t_w = torch.tensor(w[NU:], device="cuda", dtype=torch.float64)
        t_v = torch.tensor(v[:, NU:].T.copy(), device="cuda", dtype=torch.float64)
        chunk = max(1, (1 << 28) // ((1 + k) * (1 + k)))   # 2 GiB of outer products at a time

        def torch_():
            res["t"] = torch_fold(torch, t_users, t_pos, t_neg, t_w, t_v, 0.1, 8, chunk)
            torch.cuda.synchronize()

        versions["torch"] = torch_
    if only:   # one version alone (a run under a kernel trace, or a quick look): no comparison, no record
        fn = versions[only]
        fn()
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
        print(json.dumps({"case": f"k={k} {only} only", only: _stats(ts)}), flush=True)
        return None
    ts = {name: [] for name in versions}
    for fn in versions.values():
        fn()
    for _ in range(reps):
        for name, fn in versions.items():
            t = time.perf_counter(); fn(); ts[name].append(time.perf_counter() - t)
    out = {"case": f"movielens20m pairs k={k} logistic x8", "reps": reps, "k": k, "pairs": n, "rows": 2 * n, "groups": NU,
           "fold_in_pairs": _stats(ts["fold_in_pairs"]), "torch": _stats(ts["torch"])}
    gw, gv, pairs, status = res["f"]
    th = res["t"].cpu().numpy()
    scale = np.maximum(np.abs(th).max(1), 1e-300)
    out["max_rel_diff_vs_torch"] = float((np.abs(np.concatenate([gw[:, None], gv.T], 1) - th).max(1) / scale).max())
    out["status_failed"] = int(status.sum())
    out["w_exactly_zero"] = bool(np.all(gw == 0.0))
    out["pairs_counted"] = int(pairs.sum())
    gap = out["torch"]["median_s"] - out["fold_in_pairs"]["median_s"]
    spread = max(out["torch"]["max_s"] - out["torch"]["min_s"], out["fold_in_pairs"]["max_s"] - out["fold_in_pairs"]["min_s"])
    out["ratio_torch_over_fold_in_pairs"] = out["torch"]["median_s"] / out["fold_in_pairs"]["median_s"]
    out["gate_faster_than_torch"] = bool(gap > spread)
    print(json.dumps(out), flush=True)
    return out


def write_txt(rec, path):
    lines = ["", "fmx_fold_in_pairs timing record (profiles/foldin_pairs_bench.py); medians of alternated calls after one warm-up, [min, max]"]
    for o in rec["cases"]:
        lines.append(f"{o['case']} ({o['reps']} rounds): {o['pairs']} pairs ({o['rows']} rows), {o['groups']} users folded in one call, fp32 tables")
        for name in ("fold_in_pairs", "torch"):
            t = o[name]
            lines.append(f"  {name:14s} {t['median_s'] * 1e3:10.1f} ms [{t['min_s'] * 1e3:.1f}, {t['max_s'] * 1e3:.1f}]")
        lines.append(f"  torch / fold_in_pairs = {o['ratio_torch_over_fold_in_pairs']:.2f}; faster by more than the spread of either side: "
                     f"{'yes' if o['gate_faster_than_torch'] else 'no'}")
        lines.append(f"  largest difference from the torch result relative to a user's max |theta|: {o['max_rel_diff_vs_torch']:.3g}; unsolved groups: "
                     f"{o['status_failed']}; every w exactly 0: {o['w_exactly_zero']}; pairs counted: {o['pairs_counted']}")
    open(path, "a").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=N)
    ap.add_argument("--k", default="16,64")
    ap.add_argument("--only", default="", help="fold_in_pairs or torch: time that version alone and write no record")
    ap.add_argument("--merge", nargs="+", metavar="RECORD_JSON", help="join the records of separate runs (one k per process) into --out and write its text")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "foldin_pairs.json"))
    args = ap.parse_args()
    if args.merge:
        rec = {"cases": [c for f in args.merge for c in json.load(open(f))["cases"]]}
        json.dump(rec, open(args.out, "w"), indent=1)
        write_txt(rec, args.out.replace(".json", ".txt"))
        return
    torch = None
    if args.only != "fold_in_pairs":
        import torch
    rec = {"cases": []}
    for k in [int(x) for x in args.k.split(",")]:
        out = run_case(torch, k, args.reps, args.pairs, args.only)
        if out is not None:
            rec["cases"].append(out)
            json.dump(rec, open(args.out, "w"), indent=1)
    if rec["cases"]:
        write_txt(rec, args.out.replace(".json", ".txt"))


if __name__ == "__main__":
    main()
