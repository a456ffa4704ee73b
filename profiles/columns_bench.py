"""Column selection on the device (fmx_matrix_column_stats, fmx_column_map_select, fmx_column_map_hash, fmx_matrix_remap_columns) measured against
the only route the library offered before -- Matrix.export -> numpy (bincount, indexing, a stable argsort where entries merge) -> Matrix.from_csr --
and, beside it, against a torch formulation on the same device (bincount, boolean indexing, a stable sort) that is handed the arrays for free and
leaves its result as tensors.  Writes profiles/columns.json and a one-page profiles/columns.txt.

Shapes:
  a  configs[1]'s matrix (10 M rows x 1 M i.i.d. columns, 30 entries per row): stats -- the counts and the two sums alone; prune -- stats, a map at
     the min_rows that drops about half of the columns (read from the stats), the matrix under it with DROP and KEEP; hash -- a map into 2^18 buckets
     and the matrix under it with SUM.
  b  1 M Criteo-shaped rows (13 dense + 26 fields, 33 M features): prune with min_rows = 5, one bucket per field, FIRST.
Per task, in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min, max]).  The gate: the
device route is faster than the host round trip by more than the spread of either side; the record says so in bold if not, and states the torch
comparison either way."""
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
        print("  round", r + 1, {v: round(t[-1], 4) for v, t in ts.items()}, flush=True)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out):
    for other in ("host", "torch"):
        spread = max(out[other]["max_s"] - out[other]["min_s"], out["device"]["max_s"] - out["device"]["min_s"])
        gap = out[other]["median_s"] - out["device"]["median_s"]
        out[other + "_over_device"] = out[other]["median_s"] / out["device"]["median_s"]
        out["device_vs_" + other] = "faster" if gap > spread else "slower" if -gap > spread else "within the spread"


def _rows_of(rp):
    return np.repeat(np.arange(len(rp) - 1, dtype=np.int64), np.diff(rp))


def _host_counts(rp, col, p):
    """entries and rows of every column; the rows are sorted inside (both generators): a duplicate is a repeat of its left neighbour"""
    entries = np.bincount(col, minlength=p)
    dup = np.zeros(len(col), bool)
    dup[1:] = col[1:] == col[:-1]
    dup[rp[:-1][np.diff(rp) > 0]] = False
    return entries, entries - np.bincount(col[dup], minlength=p)


def _host_merge(engine, rp, nid, val, y, new_p, first):
    """drop, a stable sort by (row, new id), merge equal ids (fp64 sum rounded once, or the first), upload"""
    row = _rows_of(rp)
    keep = nid != 0xFFFFFFFF
    row, nid, val = row[keep], nid[keep].astype(np.int64), val[keep]
    order = np.argsort((row << 32) | nid, kind="stable")
    row, nid, val = row[order], nid[order], val[order]
    head = np.ones(len(nid), bool)
    head[1:] = (nid[1:] != nid[:-1]) | (row[1:] != row[:-1])
    starts = np.flatnonzero(head)
    oval = val[starts] if first else np.add.reduceat(val.astype(np.float64), starts).astype(np.float32) if len(starts) else val[:0]
    orp = np.zeros(len(rp), np.int64)
    np.cumsum(np.bincount(row[starts], minlength=len(rp) - 1), out=orp[1:])
    return engine.Matrix.from_csr(orp, nid[starts].astype(np.uint32), oval, new_p, y)


def _torch_merge(torch, row, nid, val, n, first):
    keep = nid != 0xFFFFFFFF
    row, nid, val = row[keep], nid[keep], val[keep]
    order = torch.sort((row << 32) | nid, stable=True).indices
    row, nid, val = row[order], nid[order], val[order]
    head = torch.ones_like(nid, dtype=torch.bool)
    head[1:] = (nid[1:] != nid[:-1]) | (row[1:] != row[:-1])
    if first:
        oval = val[head]
    else:
        run = torch.cumsum(head.long(), 0) - 1
        oval = torch.zeros(int(head.sum()), dtype=torch.float64, device=val.device).index_add_(0, run, val.double()).float()
    orp = torch.cumsum(torch.bincount(row[head], minlength=n), 0)
    torch.cuda.synchronize()
    return int(orp[-1]) if n else 0


def _closed(m):
    k = m.nnz
    m.close()
    return k


def shape_a(args, torch):
    from fmwr_amd import _lib as L, engine
    from tests.util import DevBuf
    n, p = int(10_000_000 * args.n_scale), 1_000_000
    m = engine.Matrix.synthetic_iid(n, p, 30, 11)
    rp, col, val, y = m.export()
    t_col, t_val = torch.from_numpy(col.astype(np.int64)).cuda(), torch.from_numpy(val).cuda()
    t_row = torch.from_numpy(_rows_of(rp)).cuda()
    dc, dv, dm = DevBuf(p * 3, np.int64), DevBuf(p * 2, np.float64), DevBuf(p, np.uint32)
    count, _ = m.column_stats(values=False)
    cut = int(np.median(count[:, 1])) + 1           # drops about half of the columns
    out = {}

    # ---- stats
    def device():
        m.column_stats_device(dc.ptr, dv.ptr)

    def host():
        r, c, v, _ = m.export()
        _host_counts(r, c, p)
        x = v.astype(np.float64)
        return np.bincount(c, weights=x, minlength=p), np.bincount(c, weights=x * x, minlength=p)

    def torch_route():
        x = t_val.double()
        torch.bincount(t_col, minlength=p), torch.bincount(t_col, weights=x, minlength=p), torch.bincount(t_col, weights=x * x, minlength=p)
        torch.cuda.synchronize()
    o = _alternate({"device": device, "host": host, "torch": torch_route}, args.reps)
    _verdict(o)
    o.update(rows=n, entries=m.nnz, features=p, what="column_stats: counts and the two sums")
    out["a.stats"] = o

    # ---- prune: DROP, KEEP
    def device():
        m.column_stats_device(dc.ptr, None)
        new_p, _ = engine.column_map_select_device(p, dc.ptr, dm.ptr, by=L.COLUMNS_BY_ROWS, min_count=cut, rare=L.RARE_DROP)
        return _closed(m.remap_columns_device(dm.ptr, new_p, L.COMBINE_KEEP))

    def host():
        r, c, v, yy = m.export()
        _, rows = _host_counts(r, c, p)
        keep = rows >= cut
        cmap = np.cumsum(keep) - 1
        ek = keep[c]
        orp = np.zeros(len(r), np.int64)
        np.cumsum(np.bincount(_rows_of(r)[ek], minlength=len(r) - 1), out=orp[1:])
        return _closed(engine.Matrix.from_csr(orp, cmap[c[ek]].astype(np.uint32), v[ek], int(keep.sum()), yy))

    def torch_route():
        keep = torch.bincount(t_col, minlength=p) >= cut
        cmap = torch.cumsum(keep.long(), 0) - 1
        ek = keep[t_col]
        orp = torch.cumsum(torch.bincount(t_row[ek], minlength=n), 0)
        ocol, oval = cmap[t_col[ek]], t_val[ek]
        torch.cuda.synchronize()
        return int(orp[-1])
    kd, kh = device(), host()
    assert kd == kh, (kd, kh)
    o = _alternate({"device": device, "host": host, "torch": torch_route}, args.reps)
    _verdict(o)
    o.update(rows=n, entries=m.nnz, entries_out=kd, min_rows=cut, what=f"prune: stats + map (min_rows = {cut}, DROP) + remap (KEEP)")
    out["a.prune"] = o

    # ---- hash into 2^18 buckets, SUM
    B = 1 << 18
    hmap, _ = engine.column_map_hash(p, B, seed=3)
    t_map = torch.from_numpy(hmap.astype(np.int64)).cuda()

    def device():
        new_p = engine.column_map_hash_device(p, B, dm.ptr, seed=3)
        return _closed(m.remap_columns_device(dm.ptr, new_p, L.COMBINE_SUM))

    def host():
        r, c, v, yy = m.export()
        return _closed(_host_merge(engine, r, hmap[c], v, yy, B, False))

    def torch_route():
        return _torch_merge(torch, t_row, t_map[t_col], t_val, n, False)
    kd, kh = device(), host()
    assert kd == kh, (kd, kh)
    o = _alternate({"device": device, "host": host, "torch": torch_route}, args.reps)
    _verdict(o)
    o.update(rows=n, entries=m.nnz, entries_out=kd, what="hash: map into 2^18 buckets + remap (SUM)")
    out["a.hash"] = o
    return out


def shape_b(args, torch):
    from fmwr_amd import _lib as L, engine
    from tests.util import DevBuf
    n = int(1_000_000 * args.n_scale)
    vocab = engine.CRITEO_VOCAB
    m = engine.Matrix.synthetic_fields(n, 13, vocab, 3.0, 11)
    p = m.p
    base = np.concatenate([[0], 13 + np.cumsum(vocab)]).astype(np.uint32)     # the dense columns ride in the first field's segment, kept by the prefix
    rp, col, val, y = m.export()
    t_col, t_val, t_row = torch.from_numpy(col.astype(np.int64)).cuda(), torch.from_numpy(val).cuda(), torch.from_numpy(_rows_of(rp)).cuda()
    t_base = torch.from_numpy(base.astype(np.int64)).cuda()
    dc, dm = DevBuf(p * 3, np.int64), DevBuf(p, np.uint32)
    rule = dict(by=L.COLUMNS_BY_ROWS, min_count=5, keep_prefix=13, rare=L.RARE_BUCKET, segment_base=base)
    S = len(base) - 1

    def device():
        m.column_stats_device(dc.ptr, None)
        new_p, _ = engine.column_map_select_device(p, dc.ptr, dm.ptr, **rule)
        return _closed(m.remap_columns_device(dm.ptr, new_p, L.COMBINE_FIRST))

    def host():
        r, c, v, yy = m.export()
        _, rows = _host_counts(r, c, p)
        keep = rows >= 5
        keep[:13] = True
        pos = np.concatenate([[0], np.cumsum(keep)])
        seg = np.searchsorted(base, np.arange(p), side="right") - 1
        cmap = np.where(keep, pos[:-1] + seg, pos[base[seg + 1]] + seg)
        return _closed(_host_merge(engine, r, cmap[c].astype(np.uint32), v, yy, int(pos[-1]) + S, True))

    def torch_route():
        keep = torch.bincount(t_col, minlength=p) >= 5
        keep[:13] = True
        pos = torch.cat([torch.zeros(1, dtype=torch.int64, device=keep.device), torch.cumsum(keep.long(), 0)])
        seg = torch.searchsorted(t_base, torch.arange(p, device=keep.device), right=True) - 1
        cmap = torch.where(keep, pos[:-1] + seg, pos[t_base[seg + 1]] + seg)
        return _torch_merge(torch, t_row, cmap[t_col], t_val, n, True)
    kd, kh = device(), host()
    assert kd == kh, (kd, kh)
    o = _alternate({"device": device, "host": host, "torch": torch_route}, args.reps)
    _verdict(o)
    o.update(rows=n, entries=m.nnz, features=p, entries_out=kd, what="prune: stats + map (min_rows = 5, one bucket per field) + remap (FIRST)")
    return {"b.prune": o}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "columns.json"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()  # before libfmx: the same process
    shapes = ["a", "b"] if args.shape == "all" else args.shape.split(",")
    record = {"reps": args.reps, "n_scale": args.n_scale, "tasks": {}}
    for s in shapes:
        for name, o in {"a": shape_a, "b": shape_b}[s](args, torch).items():
            record["tasks"][name] = o
            print(name, json.dumps(o), flush=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
    lines = ["column selection on the device against export -> numpy -> from_csr, and against torch on the same device (profiles/columns_bench.py; "
             "medians of %d alternated calls, [min, max]; rows scaled by %g)" % (args.reps, args.n_scale)]
    for s, o in record["tasks"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries" + (f" -> {o['entries_out']:,}" if "entries_out" in o else ""))
        for v in ("device", "host", "torch"):
            lines.append(f"    {v:7s} {o[v]['median_s'] * 1e3:10.1f} ms  [{o[v]['min_s'] * 1e3:.1f}, {o[v]['max_s'] * 1e3:.1f}]")
        gate = "" if o["device_vs_host"] == "faster" else "  ** THE GATE IS MISSED **"
        lines.append(f"    host / device = {o['host_over_device']:.1f}x: the device route is {o['device_vs_host']}{gate}")
        lines.append(f"    torch / device = {o['torch_over_device']:.2f}x: the device route is {o['device_vs_torch']} (a comparison, not the gate)")
    with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
