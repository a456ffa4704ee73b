"""FMX_TASK_RANKING measured at two shapes, fp32 state.  Writes the record to --out (profiles/rank.json);
profiles/rank.txt is the one-page summary of it.

  (A) MovieLens-20M-like implicit feedback: 138 493 one-hot users, 26 744 one-hot items, 20 M positives (users uniform, items Zipf(1.0) by
      popularity rank), k = 64, n_neg = 1
  (B) rich context: 1 M contexts of 28 one-hot entries over 1 M features, 100 000 items of 2 entries (id + one of 1 000 categories), 10 M
      positives, k = 16, n_neg = 1

Per epoch (epochs 0 and 1; epoch 0 includes first-use allocations), each figure ending with a device synchronise:
  sample   fmx_matrix_pairs (dedup sort, draws, shuffle sort, gather, flags)
  plan     fmx_num_batches on the new matrix (the per-tile inverted indices of its steps)
  steps    fmx_train over all of its pairs (one pass)
  pairs/s  pairs / (sample + plan + steps)
Then, on epoch 1's pair matrix: a CLASSIFICATION engine of the same configuration over the same rows (the pointwise step; labels are 1), and
a torch BPR-FM on the same pairs and precision (EmbeddingBag sums of x v, x^2 v^2 and x w, the BPR loss, autograd, SGD), timed over
--torch-steps steps and scaled per pair.  Both rates are steps only (plans built beforehand).
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


def _sync(e):
    e.sync()


def _zipf_items(rng, n, n_items, s=1.0):
    w = 1.0 / np.arange(1, n_items + 1) ** s
    cdf = np.cumsum(w) / w.sum()
    rank = np.searchsorted(cdf, rng.random(n))
    perm = rng.permutation(n_items)  # popularity rank -> item id
    return perm[np.minimum(rank, n_items - 1)]


def shape_a(rng, scale):
    from fmwr_amd import engine
    users, items = 138_493, 26_744
    n_pos = int(20_000_000 * scale)
    p = users + items
    C = engine.Matrix.from_csr(np.arange(users + 1, dtype=np.int64), np.arange(users, dtype=np.uint32), np.ones(users, np.float32), p)
    I = engine.Matrix.from_csr(np.arange(items + 1, dtype=np.int64), users + np.arange(items, dtype=np.uint32), np.ones(items, np.float32), p)
    u = np.sort(rng.integers(0, users, n_pos))
    it = _zipf_items(rng, n_pos, items)
    rp = np.searchsorted(u, np.arange(users + 1)).astype(np.int64)
    X = engine.Matrix.from_csr(rp, it.astype(np.uint32), np.ones(n_pos, np.float32), items)
    return dict(name="A_movielens_like", C=C, I=I, X=X, p=p, k=64, n_ctx=users, n_items=items, n_pos=n_pos)


def shape_b(rng, scale):
    from fmwr_amd import engine
    n_ctx, f_ctx, z = int(1_000_000 * scale), 1_000_000, 28
    items, cats = 100_000, 1_000
    n_pos = int(10_000_000 * scale)
    p = f_ctx + items + cats
    cc = np.sort(rng.integers(0, f_ctx, (n_ctx, z)), axis=1).astype(np.uint32).ravel()
    C = engine.Matrix.from_csr(np.arange(0, n_ctx * z + 1, z, dtype=np.int64), cc, np.ones(n_ctx * z, np.float32), p)
    ic = np.stack([f_ctx + np.arange(items), f_ctx + items + rng.integers(0, cats, items)], 1).astype(np.uint32).ravel()
    I = engine.Matrix.from_csr(np.arange(0, 2 * items + 1, 2, dtype=np.int64), ic, np.ones(2 * items, np.float32), p)
    c = np.sort(rng.integers(0, n_ctx, n_pos))
    it = _zipf_items(rng, n_pos, items)
    rp = np.searchsorted(c, np.arange(n_ctx + 1)).astype(np.int64)
    X = engine.Matrix.from_csr(rp, it.astype(np.uint32), np.ones(n_pos, np.float32), items)
    return dict(name="B_rich_context", C=C, I=I, X=X, p=p, k=16, n_ctx=n_ctx, n_items=items, n_pos=n_pos)


def _engine(task, p, k, batch_rows):
    from fmwr_amd import _lib as L, engine
    e = engine.Engine(p, task=task, solver=L.SOLVER_SGD, num_factor=k, mode=L.MODE_MINIBATCH, batch_rows=batch_rows, learn_rate=0.05, l2_v=1e-5)
    e.init_normal(5, 0.0, 0.1)
    return e


def torch_bpr(pm, k, p, batch_rows, steps, torch):
    """BPR-FM in torch on the first `steps` batches of pm (fp32 tables, the same pairs): EmbeddingBag sums of x v, x^2 v^2 and x w per row,
    the BPR loss, autograd, SGD.  Seconds per step."""
    r_end = min(pm.n, steps * batch_rows)
    rp, col, val, _ = pm.export(0, r_end)
    dev = "cuda"
    F = torch.nn.functional
    Vw = torch.nn.Parameter(torch.randn(p, k, device=dev) * 0.1)
    Ww = torch.nn.Parameter(torch.zeros(p, 1, device=dev))
    opt = torch.optim.SGD([Vw, Ww], lr=0.05)
    batches = []
    for r0 in range(0, r_end, batch_rows):
        r1 = min(r_end, r0 + batch_rows)
        e0, e1 = int(rp[r0]), int(rp[r1])
        batches.append((torch.from_numpy(col[e0:e1].astype(np.int64)).to(dev), torch.from_numpy((rp[r0:r1] - rp[r0]).astype(np.int64)).to(dev),
                        torch.from_numpy(val[e0:e1]).to(dev)))

    def step(b):
        idx, off, x = b
        s = F.embedding_bag(idx, Vw, off, mode="sum", per_sample_weights=x)
        q = F.embedding_bag(idx, Vw * Vw, off, mode="sum", per_sample_weights=x * x)
        lin = F.embedding_bag(idx, Ww, off, mode="sum", per_sample_weights=x).squeeze(1)
        y = lin + 0.5 * (s * s - q).sum(1)
        d = y[0::2] - y[1::2]
        loss = F.softplus(-d).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    step(batches[0]); torch.cuda.synchronize()
    t = time.perf_counter()
    for b in batches:
        step(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / len(batches), len(batches)


def run_shape(sh, args, torch):
    from fmwr_amd import _lib as L, engine
    B = args.batch_rows
    e = _engine(L.TASK_RANKING, sh["p"], sh["k"], B)
    epochs = []
    pm = None
    for epoch in range(2):
        if pm is not None:
            pm.close()
        t0 = time.perf_counter()
        pm = engine.Matrix.pairs(sh["C"], sh["I"], sh["X"], 1, 77, epoch)
        t1 = time.perf_counter()
        e.num_batches(pm); _sync(e)
        t2 = time.perf_counter()
        e.train(pm, pm.n); _sync(e)
        t3 = time.perf_counter()
        pairs = pm.n // 2
        epochs.append(dict(epoch=epoch, pairs=pairs, rows=pm.n, nnz=pm.nnz, sample_s=t1 - t0, plan_s=t2 - t1, steps_s=t3 - t2,
                           pairs_per_s=pairs / (t3 - t0), step_pairs_per_s=pairs / (t3 - t2)))
        print(sh["name"], epochs[-1], flush=True)
    # pointwise step on the same rows, same configuration (plans of this matrix already built for B)
    ec = _engine(L.TASK_CLASSIFICATION, sh["p"], sh["k"], B)
    ec.num_batches(pm); ec.train(pm, min(pm.n, 8 * B)); _sync(ec)   # warm-up (schedule tuning of phase 1)
    e.train(pm, min(pm.n, 8 * B)); _sync(e)
    reps = []
    for _ in range(args.reps):
        t = time.perf_counter(); ec.train(pm, pm.n); _sync(ec); tc = time.perf_counter() - t
        t = time.perf_counter(); e.train(pm, pm.n); _sync(e); tr = time.perf_counter() - t
        reps.append((tr, tc))
    ratios = sorted(tr / tc for tr, tc in reps)
    out = dict(shape=sh["name"], n_ctx=sh["n_ctx"], n_items=sh["n_items"], positives_drawn=sh["n_pos"], p=sh["p"], k=sh["k"], batch_rows=B, epochs=epochs,
               rank_vs_classification=dict(rank_s=[r[0] for r in reps], classification_s=[r[1] for r in reps], ratio_median=ratios[len(ratios) // 2],
                                           ratio_min=ratios[0], ratio_max=ratios[-1]))
    if torch is not None:
        per_step, n = torch_bpr(pm, sh["k"], sh["p"], B, args.torch_steps, torch)
        eng_per_step = min(r[0] for r in reps) / ((pm.n + B - 1) // B)
        out["torch"] = dict(steps=n, s_per_step=per_step, engine_s_per_step=eng_per_step, speedup=per_step / eng_per_step)
    print(json.dumps({k: v for k, v in out.items() if k != "epochs"}), flush=True)
    pm.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="A,B")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the contexts / positives (smoke runs)")
    ap.add_argument("--batch-rows", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=60)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank.json"))
    args = ap.parse_args()
    torch = None
    if not args.no_torch:
        import torch  # noqa: F811
    rng = np.random.default_rng(2026)
    res = []
    for s in args.shapes.split(","):
        sh = (shape_a if s == "A" else shape_b)(rng, args.scale)
        res.append(run_shape(sh, args, torch))
        for key in ("C", "I", "X"):
            sh[key].close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"results": res, "scale": args.scale}, f, indent=1)


if __name__ == "__main__":
    main()
