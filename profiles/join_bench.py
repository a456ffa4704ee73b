"""Matrix composition on the device (fmx_matrix_join_device, fmx_matrix_stack) measured against the only route the library offered before --
Matrix.export -> numpy (fancy indexing, np.repeat) -> Matrix.from_csr -- and, beside it, against a torch formulation on the same device that is
handed the arrays for free and leaves its result as tensors.  Writes profiles/join.json and a one-page profiles/join.txt.

Shapes:
  a  10 M interactions over 138 493 users and 26 744 items (MovieLens-20M-shaped), 8 user-side and 8 item-side one-hot fields, two indicator
     blocks: rows of 18 entries, every block of a fixed length (the fixed form).
  b  the same with ragged side rows, Poisson(8) clipped to [0, 64] (the lane-group form).
  c  fmx_matrix_stack of the 5 folds of configs[1]'s matrix (10 M rows x 1 M features, 30 entries per row).
Per shape, in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min, max]).  The gate: the
device route is faster than the host round trip by more than the spread of either side; the record says so in bold if not, and states the torch
comparison either way.  --device-only times the device route alone (for a kernel trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

USERS, ITEMS = 138_493, 26_744
VOCAB = [1000, 300, 120, 50, 21, 7, 4, 2]


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def _alternate(versions, reps):
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for _ in range(reps):          # alternated: one call of each route per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out):
    for other in ("host", "torch"):
        if other not in out:
            continue
        spread = max(out[other]["max_s"] - out[other]["min_s"], out["device"]["max_s"] - out["device"]["min_s"])
        gap = out[other]["median_s"] - out["device"]["median_s"]
        out[other + "_over_device"] = out[other]["median_s"] / out["device"]["median_s"]
        out["device_vs_" + other] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _spread(start, lens):
    first = np.cumsum(lens) - lens
    return np.repeat(start - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)


def _host_design(engine, mu, mi, user, item, bases, p):
    """the parent's route: the side tables exported, the joined CSR assembled in numpy, one upload"""
    n = len(user)
    sides = [(mu.export(), user, bases[2]), (mi.export(), item, bases[3])]
    lens = [np.ones(n, np.int64), np.ones(n, np.int64)] + [(h[0][1:] - h[0][:-1])[ids] for h, ids, _ in sides]
    orp = np.zeros(n + 1, np.int64)
    np.cumsum(lens[0] + lens[1] + lens[2] + lens[3], out=orp[1:])
    col, val = np.empty(int(orp[-1]), np.uint32), np.ones(int(orp[-1]), np.float32)
    col[orp[:-1]] = user + bases[0]
    col[orp[:-1] + 1] = item + bases[1]
    before = 2
    for (h, ids, base), ln in zip(sides, lens[2:]):
        dst, src = _spread(orp[:-1] + before, ln), _spread(h[0][ids], ln)
        col[dst] = h[1][src] + np.uint32(base)
        val[dst] = h[2][src]
        before = before + ln
    return engine.Matrix.from_csr(orp, col, val, p)


def _design_shape(args, torch, ragged):
    from fmwr_amd import engine
    from tests.util import DevBuf
    n = int(10_000_000 * args.n_scale)
    rng = np.random.default_rng(9)
    user, item = rng.integers(0, USERS, n), rng.integers(0, ITEMS, n)
    if ragged:
        mu = engine.Matrix.synthetic_ragged(USERS, 4000, 8.0, 3, min_nnz=0, max_nnz=64)
        mi = engine.Matrix.synthetic_ragged(ITEMS, 4000, 8.0, 4, min_nnz=0, max_nnz=64)
    else:
        mu = engine.Matrix.synthetic_fields(USERS, 0, VOCAB, 1.1, 3)
        mi = engine.Matrix.synthetic_fields(ITEMS, 0, VOCAB, 1.1, 4)
    bases = engine.join_bases([USERS, ITEMS, mu, mi])
    p = int(bases[4])
    du, di = DevBuf.from_numpy(user), DevBuf.from_numpy(item)
    blocks = [(USERS, du.ptr, int(bases[0])), (ITEMS, di.ptr, int(bases[1])), (mu, du.ptr, int(bases[2])), (mi, di.ptr, int(bases[3]))]

    def device():
        m = engine.Matrix.join_device(blocks, n, p)
        k = m.nnz
        m.close()
        return k

    def host():
        m = _host_design(engine, mu, mi, user, item, bases, p)
        k = m.nnz
        m.close()
        return k
    routes = {"device": device}
    if not args.device_only:
        routes["host"] = host
        assert device() == host()
        a, b = engine.Matrix.join_device(blocks, n, p), _host_design(engine, mu, mi, user, item, bases, p)
        ea, eb = a.export(), b.export()
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(ea[:3], eb[:3]))
        a.close(); b.close()
        del ea, eb
    if torch is not None and not args.device_only:
        hu, hi = mu.export(), mi.export()
        t_user, t_item = torch.from_numpy(user).cuda(), torch.from_numpy(item).cuda()
        tu = [torch.from_numpy(x.astype(np.int64) if x.dtype != np.float32 else x).cuda() for x in hu[:3]]
        ti = [torch.from_numpy(x.astype(np.int64) if x.dtype != np.float32 else x).cuda() for x in hi[:3]]

        def t_spread(start, lens):
            first = torch.cumsum(lens, 0) - lens
            return torch.repeat_interleave(start - first, lens) + torch.arange(int(lens.sum()), device=lens.device)

        def torch_route():
            lu, li = (tu[0][1:] - tu[0][:-1])[t_user], (ti[0][1:] - ti[0][:-1])[t_item]
            orp = torch.zeros(n + 1, dtype=torch.int64, device=lu.device)
            orp[1:] = torch.cumsum(lu + li + 2, 0)
            total = int(orp[-1])
            col, val = torch.empty(total, dtype=torch.int64, device=lu.device), torch.ones(total, dtype=torch.float32, device=lu.device)
            col[orp[:-1]] = t_user + int(bases[0])
            col[orp[:-1] + 1] = t_item + int(bases[1])
            for t, ids, ln, before, base in ((tu, t_user, lu, 2, int(bases[2])), (ti, t_item, li, lu + 2, int(bases[3]))):
                dst, src = t_spread(orp[:-1] + before, ln), t_spread(t[0][ids], ln)
                col[dst] = t[1][src] + base
                val[dst] = t[2][src]
            torch.cuda.synchronize()
            return total
        assert torch_route() == device()
        routes["torch"] = torch_route
    out = _alternate(routes, args.reps)
    _verdict(out)
    k = device()
    # what the copy itself moves: every block's ids once, the source columns (and values, unless they are filled), the output's columns and values
    import ctypes as C
    from fmwr_amd import _lib as L
    side = k - 2 * n
    unit = []
    for m in (mu, mi):
        f = np.zeros(5, np.int32)
        L.check(L.lib().fmx_debug_matrix_flags(m.h, f.ctypes.data_as(C.c_void_p)))
        unit.append(int(f[1]))
    moved = 4 * n * 8 + side * 4 * (1 if all(unit) else 2) + 2 * k * 4
    out.update(rows=n, entries=k, features=p, bytes_moved_by_the_copy=moved, what=("ragged side rows, Poisson(8) in [0, 64]" if ragged else "8 + 8 one-hot side fields") +
               ", two indicator blocks: join_device")
    return out


def shape_c(args, torch):
    from fmwr_amd import engine
    n, k = int(10_000_000 * args.n_scale), 5
    m = engine.Matrix.synthetic(n, 1_000_000, 30, 11)
    part = engine.split_assign(n, n_folds=k, seed=5)
    folds = [m.select(part, f) for f in range(k)]
    m.close()

    def device():
        s = engine.Matrix.stack(folds)
        e = s.nnz
        s.close()
        return e

    def host():
        ex = [f.export() for f in folds]
        first = np.cumsum([0] + [int(e[0][-1]) for e in ex])
        orp = np.concatenate([e[0][:-1] + first[i] for i, e in enumerate(ex)] + [first[-1:]])
        s = engine.Matrix.from_csr(orp, np.concatenate([e[1] for e in ex]), np.concatenate([e[2] for e in ex]), folds[0].p, np.concatenate([e[3] for e in ex]))
        e = s.nnz
        s.close()
        return e
    routes = {"device": device}
    if not args.device_only:
        routes["host"] = host
        assert device() == host() == 30 * n
    if torch is not None and not args.device_only:
        ex = [f.export() for f in folds]
        tf = [[torch.from_numpy(x).cuda() for x in e] for e in ex]
        del ex

        def torch_route():
            first = [0]
            for t in tf:
                first.append(first[-1] + int(t[0][-1]))
            orp = torch.cat([t[0][:-1] + first[i] for i, t in enumerate(tf)] + [torch.tensor([first[-1]], device=tf[0][0].device)])
            col, val, y = torch.cat([t[1] for t in tf]), torch.cat([t[2] for t in tf]), torch.cat([t[3] for t in tf])
            torch.cuda.synchronize()
            return int(col.numel())
        routes["torch"] = torch_route
    out = _alternate(routes, args.reps)
    _verdict(out)
    out.update(rows=n, entries=30 * n, features=folds[0].p, what=f"stack of the {k} folds of configs[1]'s matrix")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b, c; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--device-only", action="store_true", help="time the device route alone (a kernel trace of it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join.json"))
    args = ap.parse_args()
    torch = None
    if not args.no_torch and not args.device_only:
        import torch
        torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b", "c"] if args.shape == "all" else args.shape.split(",")
    record = {"reps": args.reps, "n_scale": args.n_scale, "shapes": {}}
    fns = {"a": lambda a, t: _design_shape(a, t, False), "b": lambda a, t: _design_shape(a, t, True), "c": shape_c}
    for s in shapes:
        record["shapes"][s] = fns[s](args, torch)
        print(s, json.dumps(record["shapes"][s]), flush=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    lines = ["matrix composition on the device against export -> numpy -> from_csr, and against torch on the same device (profiles/join_bench.py; "
             "medians of %d alternated calls, [min, max]; rows scaled by %g)" % (args.reps, args.n_scale)]
    for s, o in record["shapes"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries, {o['features']:,} features")
        for v in ("device", "host", "torch"):
            if v in o:
                lines.append(f"    {v:7s} {o[v]['median_s'] * 1e3:10.1f} ms  [{o[v]['min_s'] * 1e3:.1f}, {o[v]['max_s'] * 1e3:.1f}]")
        if "host" in o:
            gate = "" if o["device_vs_host"] == "faster" else "  ** THE GATE IS MISSED **"
            lines.append(f"    host / device = {o['host_over_device']:.1f}x: the device route is {o['device_vs_host']}{gate}")
        if "torch" in o:
            lines.append(f"    torch / device = {o['torch_over_device']:.2f}x: the device route is {o['device_vs_torch']} (a comparison, not the gate)")
        if "bytes_moved_by_the_copy" in o:
            lines.append(f"    the copy reads and writes {o['bytes_moved_by_the_copy'] / 1e9:.2f} GB: {o['bytes_moved_by_the_copy'] / o['device']['median_s'] / 1e12:.2f} TB/s "
                         f"over the whole call (its allocations, length pass and scan included)")
    with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
