"""Row selection on the device (fmx_split_assign, fmx_matrix_select, fmx_matrix_take) measured against the only route the library offered before:
Matrix.export -> numpy indexing -> Matrix.from_csr.  Writes profiles/take.json and a one-page profiles/take.txt.

Shapes:
  a  configs[1]'s matrix (10 M rows x 1 M features, 30 entries per row): an 80/20 split of the rows -- device: split_assign + two selects; host:
     export, the same mask (handed over for free), two fancy-indexed CSRs, two uploads.
  b  the same matrix: take of a full random permutation -- device: row_permutation_device + take_device; host: export, the permutation (handed over
     for free), one fancy-indexed CSR, one upload.  Also the ratio of the device call's rows/s to fmx_measure_gather's at 128-byte rows (a 30-entry
     row is 120 bytes of columns and 120 of values): a figure, not a gate.
  c  20 M MovieLens-20M-shaped 2-entry rows in 138 493 user groups: leave-one-out inside every user (WITHIN_GROUPS, one row held, one always
     kept) -- device: split_assign + two selects; host as in a.
  d  10 M ragged rows, Poisson(8) clipped to [0, 64] (join_bench.py's shape b law): take of a full random permutation, the take call alone,
     once under the default limits (the group form) and once under fmx_debug_take_limits(-1, -1, 0) (the flat form).  No host route: the
     shape is there for A/B runs of two builds of the library (FMX_LIB_PATH).
Per shape, in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min, max]).  The gate: the
device route is faster than the host round trip by more than the spread of either side; the record says so in bold if not.  --device-only
times the device routes alone (a kernel trace, or an A/B run of two builds) and writes no record unless --out names one."""
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
    for _ in range(reps):          # alternated: one call of each route per round
        for v, fn in versions.items():
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out):
    if "host" not in out:
        return
    spread = max(out["host"]["max_s"] - out["host"]["min_s"], out["device"]["max_s"] - out["device"]["min_s"])
    gap = out["host"]["median_s"] - out["device"]["median_s"]
    out["host_over_device"] = out["host"]["median_s"] / out["device"]["median_s"]
    out["device_vs_host"] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _host_take(engine, host, rows, p):
    """the parent's route for one derived matrix, from the exported arrays"""
    rp, col, val, y = host
    lens = (rp[1:] - rp[:-1])[rows]
    orp = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=orp[1:])
    src = np.repeat(rp[rows] - orp[:-1], lens) + np.arange(int(orp[-1]), dtype=np.int64)
    return engine.Matrix.from_csr(orp, col[src], val[src], p, y[rows])


def _split_routes(engine, m, part_fn, mask):
    def device():
        part = part_fn()
        a, b = m.select(part, 0), m.select(part, 1)
        na, nb = a.n, b.n
        a.close(); b.close()
        return na, nb

    def host():
        ex = m.export()
        a, b = _host_take(engine, ex, np.flatnonzero(~mask), m.p), _host_take(engine, ex, np.flatnonzero(mask), m.p)
        na, nb = a.n, b.n
        a.close(); b.close()
        return na, nb
    return {"device": device, "host": host}


def _routes(args, routes):
    if args.device_only:
        routes.pop("host")
    else:
        assert routes["device"]() == routes["host"]()
    return routes


def shape_a(args):
    from fmwr_amd import _lib as L, engine
    n = int(10_000_000 * args.n_scale)
    m = engine.Matrix.synthetic(n, 1_000_000, 30, 11)
    part_fn = lambda: engine.split_assign(n, scope=L.SPLIT_ROWS, hold_fraction=0.2, seed=5)
    mask = part_fn() == 1
    routes = _routes(args, _split_routes(engine, m, part_fn, mask))
    assert routes["device"]() == (n - int(mask.sum()), int(mask.sum()))
    out = _alternate(routes, args.reps)
    _verdict(out)
    out.update(rows=n, entries=m.nnz, held=int(mask.sum()), what="80/20 ROWS split: assign + two selects")
    return out


def shape_b(args):
    from fmwr_amd import engine
    from tests.util import DevBuf
    n = int(10_000_000 * args.n_scale)
    m = engine.Matrix.synthetic(n, 1_000_000, 30, 11)
    d = DevBuf(n, np.int64)
    perm = engine.row_permutation(n, 3, 0)

    def device():
        engine.row_permutation_device(n, 3, 0, d.ptr)
        t = m.take_device(d.ptr, n)
        k = t.nnz
        t.close()
        return k

    def host():
        t = _host_take(engine, m.export(), perm, m.p)
        k = t.nnz
        t.close()
        return k

    def take_only():
        t = m.take_device(d.ptr, n)
        t.close()
    assert device() == m.nnz
    out = _alternate(_routes(args, {"device": device, "host": host, "take_only": take_only}), args.reps)
    _verdict(out)
    probe = engine.measure_gather(m.nnz * 4, 128)
    out.update(rows=n, entries=m.nnz, what="take of a full random permutation", take_rows_per_s=n / out["take_only"]["median_s"],
               gather_probe_rows_per_s=probe, take_over_probe=n / out["take_only"]["median_s"] / probe)
    return out


def shape_c(args):
    from fmwr_amd import _lib as L, engine
    n, users, items = int(20_000_000 * args.n_scale), 138_493, 26_744
    rng = np.random.default_rng(9)
    user = np.sort(rng.integers(0, users, n)).astype(np.uint32)
    col = np.empty(2 * n, np.uint32)
    col[0::2] = user
    col[1::2] = users + rng.integers(0, items, n)
    m = engine.Matrix.from_csr(np.arange(n + 1, dtype=np.int64) * 2, col, np.ones(2 * n, np.float32), users + items, np.ones(n, np.float32))
    part_fn = lambda: engine.split_assign(n, user, users, scope=L.SPLIT_WITHIN_GROUPS, hold_count=1, min_keep=1, seed=5)
    mask = part_fn() == 1
    routes = _routes(args, _split_routes(engine, m, part_fn, mask))
    assert routes["device"]() == (n - int(mask.sum()), int(mask.sum()))
    out = _alternate(routes, args.reps)
    _verdict(out)
    out.update(rows=n, entries=m.nnz, groups=users, held=int(mask.sum()), what="leave-one-out WITHIN_GROUPS: assign + two selects")
    return out


def shape_d(args):
    from fmwr_amd import _lib as L, engine
    from tests.util import DevBuf
    n = int(10_000_000 * args.n_scale)
    m = engine.Matrix.synthetic_ragged(n, 4000, 8.0, 3, min_nnz=0, max_nnz=64)
    d = DevBuf(n, np.int64)
    engine.row_permutation_device(n, 3, 0, d.ptr)

    def take(fixed, group):
        def run():
            L.check(L.lib().fmx_debug_take_limits(fixed, group, 0))
            t = m.take_device(d.ptr, n)
            k = t.nnz
            t.close()
            L.check(L.lib().fmx_debug_take_limits(0, 0, 0))
            return k
        return run
    routes = {"group": take(0, 0), "flat": take(-1, -1)}
    assert routes["group"]() == routes["flat"]() == m.nnz
    out = _alternate(routes, args.reps)
    out.update(rows=n, entries=m.nnz, what="ragged rows, Poisson(8) in [0, 64]: take of a full random permutation, the call alone, in the group and the flat form")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b, c, d; or all (a, b, c)")
    ap.add_argument("--device-only", action="store_true", help="time the device routes alone")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--out", default=None, help="the record (default: profiles/take.json; none with --device-only)")
    args = ap.parse_args()
    if args.out is None and not args.device_only:
        args.out = os.path.join(ROOT, "profiles", "take.json")
    shapes = ["a", "b", "c"] if args.shape == "all" else args.shape.split(",")
    record = {"reps": args.reps, "n_scale": args.n_scale, "shapes": {}}
    for s in shapes:
        record["shapes"][s] = {"a": shape_a, "b": shape_b, "c": shape_c, "d": shape_d}[s](args)
        print(s, json.dumps(record["shapes"][s]), flush=True)
    if args.out is None:
        return
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    lines = ["row selection on the device against export -> numpy -> from_csr (profiles/take_bench.py; medians of %d alternated calls, [min, max])" % args.reps]
    for s, o in record["shapes"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries")
        for v in ("device", "host", "group", "flat"):
            if v in o:
                lines.append(f"    {v:7s} {o[v]['median_s'] * 1e3:10.1f} ms  [{o[v]['min_s'] * 1e3:.1f}, {o[v]['max_s'] * 1e3:.1f}]")
        if "host" not in o:
            continue
        gate = "" if o["device_vs_host"] == "faster" else "  ** THE GATE IS MISSED **"
        lines.append(f"    host / device = {o['host_over_device']:.1f}x: the device route is {o['device_vs_host']}{gate}")
        if "take_over_probe" in o:
            lines.append(f"    take alone {o['take_only']['median_s'] * 1e3:.1f} ms = {o['take_rows_per_s'] / 1e6:.0f} M rows/s; fmx_measure_gather at 128-byte rows "
                         f"{o['gather_probe_rows_per_s'] / 1e6:.0f} M rows/s; ratio {o['take_over_probe']:.2f} (a figure, not a gate)")
    with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
