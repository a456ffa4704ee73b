"""Hard negatives (fmx_matrix_pairs_hard) measured on one MI355X, fp32 state, at profiles/rank_bench.py's shapes A and B.
Writes the record to --out (profiles/hardneg.json); profiles/hardneg.txt is the one-page summary of it.

Default run, every figure ending with a device synchronise, each shape warmed up first, --reps alternated repetitions:
  uniform    fmx_matrix_pairs (n_neg 1)
  hard       fmx_matrix_pairs_hard at n_cand 2, 8 and 32 on the same inputs
  epoch      fmx_num_batches (plan) and fmx_train (steps) over one pair matrix: the epoch the sampler feeds
  torch      the same choice in torch on the same candidate indices (the first --torch-pairs pre-shuffle pairs at n_cand 8): gather the
             candidates' item projections [T, n_cand, KS], a batched dot with the context projection, the bases, argmax; projections made
             beforehand (torch EmbeddingBag sums of the engine's x v and x w), the choice alone timed
  quality    fm_train_rank on test_gpu_rank.py's planted problem: recall@10 on the held-out items after 10 and 30 epochs, uniform against
             n_cand 8, and the wall time per epoch ((t30 - t10) / 20)
--trace: only the hard sampler calls (per shape and n_cand, --reps calls, in the order printed as the plan line), for a run under
  rocprofv3 --kernel-trace; --merge TRACE_CSV PLAN_JSON then splits every call's kernels into projection (fm_rows_forward_k, topk_pack_k),
  score + choose (hard_choose_k) and the rest, and adds the medians to --out.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "profiles")):
    if d not in sys.path:
        sys.path.insert(0, d)

N_CANDS = (2, 8, 32)
SEED = 77


def _shapes(names, scale):
    import rank_bench
    rng = np.random.default_rng(2026)
    for s in names.split(","):
        yield (rank_bench.shape_a if s == "A" else rank_bench.shape_b)(rng, scale)


def _engine(sh, batch_rows):
    import rank_bench
    from fmwr_amd import _lib as L
    return rank_bench._engine(L.TASK_RANKING, sh["p"], sh["k"], batch_rows)


def _timed(fn, e):
    t = time.perf_counter()
    pm = fn()
    e.sync()
    return time.perf_counter() - t, pm


def _stats(xs):
    xs = sorted(xs)
    return dict(runs_s=xs, median_s=xs[len(xs) // 2], min_s=xs[0], max_s=xs[-1])


# ------------------------------------------------------------------------------------------------ the numpy restatement of the draws (torch inputs)
def _mix64(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _pair_hash(seed, epoch, t, stream):
    with np.errstate(over="ignore"):
        h = _mix64(np.array([seed], np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        h = _mix64(h ^ (np.array([epoch], np.uint64) * np.uint64(0xD6E8FEB86659FD93) + np.uint64(stream)))
        return _mix64(h ^ (t + np.uint64(0x632BE59BD9B4E019)))


def _mulhi(a, b):
    m32, s32 = np.uint64(0xFFFFFFFF), np.uint64(32)
    al, ah, bl, bh = a & m32, a >> s32, b & m32, b >> s32
    with np.errstate(over="ignore"):
        p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
        mid = (p0 >> s32) + (p1 & m32) + (p2 & m32)
        return p3 + (p1 >> s32) + (p2 >> s32) + (mid >> s32)


def _candidates(X, n_items, n_pairs, n_neg, n_cand, seed, epoch):
    """(context, candidates [T, n_cand]) of the first n_pairs pre-shuffle pairs, as fm_pairs.hip draws them"""
    rp, col, _, _ = X.export()
    row = np.repeat(np.arange(len(rp) - 1, dtype=np.uint64), np.diff(rp))
    u = np.unique((row << np.uint64(32)) | col.astype(np.uint64))
    uc = (u >> np.uint64(32)).astype(np.int64)
    ui = (u & np.uint64(0xFFFFFFFF)).astype(np.int64)
    off = np.searchsorted(uc, np.arange(len(rp)))
    rank_in = np.arange(len(u)) - off[uc]
    key = (uc.astype(np.uint64) << np.uint64(32)) | (ui - rank_in).astype(np.uint64)   # (c, P[idx] - idx): ascending
    T = min(n_pairs, len(u) * n_neg)
    t = np.arange(T, dtype=np.uint64)
    c = uc[np.arange(T) // n_neg]
    m = off[c + 1] - off[c]
    cand = np.empty((T, n_cand), np.int64)
    for q in range(n_cand):
        r = _mulhi(_pair_hash(seed, epoch, t, 0 if q == 0 else q + 1), (n_items - m).astype(np.uint64))
        L = np.searchsorted(key, (c.astype(np.uint64) << np.uint64(32)) | r, side="right") - off[c]
        cand[:, q] = r.astype(np.int64) + L
    return c, cand


def torch_choice(sh, e, torch, n_pairs, n_cand, reps):
    """seconds per pair of the torch formulation of the choice (projections made beforehand, untimed)"""
    w0, w, v = e.get_params()
    dev = "cuda"
    F = torch.nn.functional
    V = torch.from_numpy(v.T.astype(np.float32)).to(dev)
    W = torch.from_numpy(w.astype(np.float32)[:, None]).to(dev)

    def project(m):
        rp, col, val, _ = m.export()
        idx = torch.from_numpy(col.astype(np.int64)).to(dev)
        offs = torch.from_numpy(rp[:-1].astype(np.int64)).to(dev)
        x = torch.from_numpy(val).to(dev)
        s = F.embedding_bag(idx, V, offs, mode="sum", per_sample_weights=x)
        q = F.embedding_bag(idx, V * V, offs, mode="sum", per_sample_weights=x * x)
        lin = F.embedding_bag(idx, W, offs, mode="sum", per_sample_weights=x).squeeze(1)
        return s, lin + 0.5 * (s * s - q).sum(1)
    sc, bc = project(sh["C"])
    si, bi = project(sh["I"])
    c, cand = _candidates(sh["X"], sh["n_items"], n_pairs, 1, n_cand, SEED, 0)
    ct = torch.from_numpy(c).to(dev)
    kt = torch.from_numpy(cand).to(dev)

    def choose():
        g = si[kt]                                                      # [T, n_cand, KS]
        d = torch.bmm(g, sc[ct].unsqueeze(2)).squeeze(2)                # [T, n_cand]
        s = d + bc[ct].unsqueeze(1) + bi[kt]
        return kt.gather(1, s.argmax(1, keepdim=True)).squeeze(1)
    choose(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); choose(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return dict(pairs=len(c), n_cand=n_cand, **_stats(ts), s_per_pair=min(ts) / len(c))


def run_shape(sh, args, torch):
    from fmwr_amd import engine
    e = _engine(sh, args.batch_rows)
    C, I, X = sh["C"], sh["I"], sh["X"]
    # warm-up: every call once, and one epoch of steps (schedule tuning of phase 1)
    _, pm = _timed(lambda: engine.Matrix.pairs(C, I, X, 1, SEED, 0), e)
    e.num_batches(pm); e.train(pm, pm.n); e.sync()
    n_pairs = pm.n // 2
    pm.close()
    for nc in N_CANDS:
        engine.Matrix.pairs_hard(e, C, I, X, 1, nc, SEED, 0).close()
    t_u, t_h = [], {nc: [] for nc in N_CANDS}
    for _ in range(args.reps):
        t, pm = _timed(lambda: engine.Matrix.pairs(C, I, X, 1, SEED, 0), e); t_u.append(t); pm.close()
        for nc in N_CANDS:
            t, pm = _timed(lambda: engine.Matrix.pairs_hard(e, C, I, X, 1, nc, SEED, 0), e); t_h[nc].append(t); pm.close()
    pm = engine.Matrix.pairs(C, I, X, 1, SEED, 1)
    plan, steps = [], []
    for _ in range(2):
        t = time.perf_counter(); e.num_batches(pm); e.sync(); plan.append(time.perf_counter() - t)
        t = time.perf_counter(); e.train(pm, pm.n); e.sync(); steps.append(time.perf_counter() - t)
        pm.close()
        pm = engine.Matrix.pairs(C, I, X, 1, SEED, 2)
    pm.close()
    out = dict(shape=sh["name"], n_ctx=sh["n_ctx"], n_items=sh["n_items"], p=sh["p"], k=sh["k"], pairs=n_pairs, batch_rows=args.batch_rows,
               uniform=_stats(t_u), hard={str(nc): _stats(t_h[nc]) for nc in N_CANDS}, epoch_plan=_stats(plan), epoch_steps=_stats(steps))
    if torch is not None:
        out["torch_choice"] = torch_choice(sh, e, torch, args.torch_pairs, 8, args.reps)
    print(json.dumps(out), flush=True)
    return out


def quality(args):
    """recall@10 after 10 and 30 epochs on the planted problem, uniform against n_cand 8, and the wall time per epoch"""
    import scipy.sparse as sp

    import fmwr_amd as fm
    rng = np.random.default_rng(11)
    n_users, n_items, k, top, held = 2000, 500, 8, 20, 2
    U = rng.normal(0, 1, (n_users, k)); W = rng.normal(0, 1, (n_items, k)); b = rng.normal(0, 1.0, n_items)
    best = np.argsort(-(U @ W.T + b[None, :]), axis=1)[:, :top]
    train, test = [], []
    for u in range(n_users):
        sel = rng.permutation(top)
        test.append(list(best[u, sel[:held]])); train.append(list(best[u, sel[held:]]))
    p = n_users + n_items
    ctx = fm.fm_matrix(sp.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, p)))
    its = fm.fm_matrix(sp.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, p)))
    ctl = [fm.model_control("RANK", **{"factor.number": 16, "v.init_stdev": 0.1}), fm.solver_control(solver=fm.SGD_solver(learn_rate=0.1))]
    fm.fm_train_rank(ctx, its, train, control=ctl, n_neg=2, epochs=2, seed=3, batch_rows=4096, n_candidates=8)   # warm-up
    out = {}
    for nc in (1, 8):
        row = {}
        for epochs in (10, 30):
            t = time.perf_counter()
            fit = fm.fm_train_rank(ctx, its, train, control=ctl, n_neg=2, epochs=epochs, seed=3, batch_rows=4096, n_candidates=nc)
            row[f"train_s_{epochs}"] = time.perf_counter() - t
            row[f"recall@10_{epochs}"] = fm.fm_recommend_metrics(fit, ctx, its, test, k=10, exclude=train, normalize=False)["recall@10"]
        row["s_per_epoch"] = (row["train_s_30"] - row["train_s_10"]) / 20
        out[str(nc)] = row
    print(json.dumps({"quality": out}), flush=True)
    return out


def trace(args):
    from fmwr_amd import engine
    plan = []
    for sh in _shapes(args.shapes, args.scale):
        e = _engine(sh, args.batch_rows)
        for nc in N_CANDS:
            engine.Matrix.pairs_hard(e, sh["C"], sh["I"], sh["X"], 1, nc, SEED, 0).close()   # warm-up calls are traced too: marked
            plan.append(dict(shape=sh["name"], n_cand=nc, warmup=True))
        for _ in range(args.reps):
            for nc in N_CANDS:
                engine.Matrix.pairs_hard(e, sh["C"], sh["I"], sh["X"], 1, nc, SEED, 0).close()
                plan.append(dict(shape=sh["name"], n_cand=nc, warmup=False))
        e.sync()
        for key in ("C", "I", "X"):
            sh[key].close()
    with open(args.plan, "w") as f:
        json.dump(plan, f)
    print(json.dumps({"plan_calls": len(plan)}), flush=True)


def merge(args):
    """split each traced call (from one draw_k to the next) into projection / score + choose / rest kernel time"""
    plan = json.load(open(args.plan))
    rows = list(csv.DictReader(open(args.trace)))
    name_k = next(k for k in rows[0] if k.lower() in ("kernel_name", "kernelname", "name"))
    start_k = "Start_Timestamp" if "Start_Timestamp" in rows[0] else next(k for k in rows[0] if "start" in k.lower())
    end_k = "End_Timestamp" if "End_Timestamp" in rows[0] else next(k for k in rows[0] if k.lower().startswith("end"))
    rows.sort(key=lambda r: int(r[start_k]))
    calls, cur = [], None
    for r in rows:
        name = r[name_k]
        if "draw_k" in name:
            cur = dict(proj=0, choose=0, rest=0)
            calls.append(cur)
        if cur is None:
            continue
        d = int(r[end_k]) - int(r[start_k])
        if "hard_choose_k" in name:
            cur["choose"] += d
        elif "fm_rows_forward" in name or "topk_pack_k" in name:
            cur["proj"] += d
        else:
            cur["rest"] += d
    assert len(calls) == len(plan), (len(calls), len(plan))
    split = {}
    for c, p in zip(calls, plan):
        if not p["warmup"]:
            split.setdefault(p["shape"], {}).setdefault(str(p["n_cand"]), []).append(c)
    res = json.load(open(args.out))
    for r in res["results"]:
        for nc, cs in split.get(r["shape"], {}).items():
            med = {key: sorted(x[key] for x in cs)[len(cs) // 2] / 1e9 for key in ("proj", "choose", "rest")}
            r["hard"][nc]["kernels_median_s"] = dict(projection=med["proj"], score_choose=med["choose"], other_kernels=med["rest"],
                                                    choose_runs_s=sorted(x["choose"] / 1e9 for x in cs))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(split))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-pairs", type=int, default=1 << 21)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--merge", nargs=2, metavar=("TRACE_CSV", "PLAN_JSON"))
    ap.add_argument("--plan", default="hardneg_trace_plan.json", help="--trace: where the call plan is written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hardneg.json"))
    args = ap.parse_args()
    if args.merge:
        args.trace, args.plan = args.merge
        return merge(args)
    if args.trace:
        return trace(args)
    torch = None
    if not args.no_torch:
        import torch  # noqa: F811
    res = []
    for sh in _shapes(args.shapes, args.scale):
        res.append(run_shape(sh, args, torch))
        for key in ("C", "I", "X"):
            sh[key].close()
    out = {"results": res, "scale": args.scale, "reps": args.reps}
    if not args.no_quality:
        out["quality"] = quality(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
