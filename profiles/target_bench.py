"""Target encoding on the device (fmx_target_stats, fmx_matrix_encode_targets) measured against the only route the library offered before --
Matrix.export -> numpy (bincount, indexing) -> TargetTable.from_arrays / Matrix.from_csr -- and beside a torch formulation on the same device
(bincount / index_add_ + gather) that is handed the arrays for free and leaves its result as tensors.  Neither yardstick is the code under test.
Writes profiles/target.json and profiles/target.txt.

Shapes:
  a  synthetic_fields(10 M rows, 13 dense columns, the 26 Criteo-shaped fields), all 26 fields, 5 folds, MEAN + COUNT, FMX_TARGET_POSITIVE: the sorted
     form of the fit (the dense columns carry real values) and the single form of the apply, timed separately.
  b  1 M ragged rows, Poisson(30) entries in [1, 64], the one bag segment, 5 folds, MEAN + COUNT: the unit form of the fit, the group form of the apply.
Per shape and step (fit, apply), in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min,
max]); every timed device call follows an untimed one of itself (profiles/cross_bench.py says why).  The gate: the device route is faster than
both yardsticks by more than the larger spread of either side.  Figures beside it: the call against its gather bound, the 128-byte lines it must
move at the measured 56.7 G lines/s -- the whole call, allocation, detector and waits included, not the kernel alone."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LINES_PER_S = 56.7e9
FOLDS = 5
PRIOR, STRENGTH = 0.25, 20.0


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def _alternate(versions, reps, settle=()):
    ts = {v: [] for v in versions}
    for fn in versions.values():   # warm-up
        fn()
    for r in range(reps):          # alternated: one call of each route per round
        for v, fn in versions.items():
            if v in settle:
                fn()
            t = time.perf_counter(); fn(); ts[v].append(time.perf_counter() - t)
        print("round", r + 1, {v: round(t[-1], 4) for v, t in ts.items()}, file=sys.stderr, flush=True)
    return {v: _stats(t) for v, t in ts.items()}


def _verdict(out, device, other):
    spread = max(out[other]["max_s"] - out[other]["min_s"], out[device]["max_s"] - out[device]["min_s"])
    gap = out[other]["median_s"] - out[device]["median_s"]
    return {"ratio": out[other]["median_s"] / out[device]["median_s"], "verdict": "faster" if gap > spread else "slower" if -gap > spread else "within the spread"}


def _values(n, a):
    """MEAN and COUNT of the definition for int64 n and a (FMX_TARGET_POSITIVE), numpy"""
    den = n.astype(np.float64) + STRENGTH
    with np.errstate(all="ignore"):
        mean = np.where(den == 0, np.float32(PRIOR), ((a.astype(np.float64) + PRIOR * STRENGTH) / den).astype(np.float32)).astype(np.float32)
    return mean, n.astype(np.float32)


def _host_fit(m, part, lo, W, single_entry):
    """export -> bincount -> from_arrays.  Columns [lo, lo + W) are the encoded ones, in slot order"""
    from fmwr_amd import engine
    rp, col, val, y = m.export()
    row = np.repeat(np.arange(m.n, dtype=np.int64), np.diff(rp))
    inside = (col >= lo) & (col < lo + W)
    key = (col[inside].astype(np.int64) - lo) * FOLDS + part[row[inside]]
    r = row[inside]
    if not single_entry:   # a column stored twice in a row counts once
        pairs = np.unique(key * m.n + r)
        key, r = pairs // m.n, pairs % m.n
    count = np.zeros((W * FOLDS, 2), np.int64)
    count[:, 0] = np.bincount(key, minlength=W * FOLDS)
    count[:, 1] = np.bincount(key[y[r] > 0], minlength=W * FOLDS)
    return count.reshape(W, FOLDS, 2), (rp, col, val, y, row, inside)


def _host_apply(m, count, part, lo, W, n_terms_fixed, exported=None):
    """export -> indexing -> from_csr; returns the Matrix.  n_terms_fixed > 0: every row holds exactly one entry of each of that many fields (shape
    a: the new entries are a dense block); 0: one bag term, per-row sums (shape b)"""
    from fmwr_amd import engine
    rp, col, val, y = m.export() if exported is None else exported
    lens = np.diff(rp)
    row = np.repeat(np.arange(m.n, dtype=np.int64), lens)
    inside = (col >= lo) & (col < lo + W)
    slot = col[inside].astype(np.int64) - lo
    f = part[row[inside]]
    tot = count.sum(axis=1)
    dn = tot[slot, 0] - count[slot, f, 0]
    da = tot[slot, 1] - count[slot, f, 1]
    if n_terms_fixed:
        T, L = n_terms_fixed, int(lens[0])
        mean, cnt = _values(dn, da)
        ocol = np.empty((m.n, L + 2 * T), np.uint32)
        oval = np.empty((m.n, L + 2 * T), np.float32)
        ocol[:, :L], oval[:, :L] = col.reshape(m.n, L), val.reshape(m.n, L)
        ocol[:, L:] = m.p + np.arange(2 * T, dtype=np.uint32)
        oval[:, L::2], oval[:, L + 1::2] = mean.reshape(m.n, T), cnt.reshape(m.n, T)
        orp = np.arange(m.n + 1, dtype=np.int64) * (L + 2 * T)
        return engine.Matrix.from_csr(orp, ocol.ravel(), oval.ravel(), m.p + 2 * T, y)
    r = row[inside]
    n_r = np.bincount(r, weights=dn.astype(np.float64), minlength=m.n).astype(np.int64)   # (exact: the sums stay far below 2^53)
    a_r = np.bincount(r, weights=da.astype(np.float64), minlength=m.n).astype(np.int64)
    has = np.bincount(r, minlength=m.n) > 0
    mean, cnt = _values(n_r, a_r)
    olen = lens + 2 * has
    orp = np.concatenate([[0], np.cumsum(olen)]).astype(np.int64)
    ocol = np.empty(int(orp[-1]), np.uint32)
    oval = np.empty(int(orp[-1]), np.float32)
    at = orp[row] + (np.arange(len(col), dtype=np.int64) - rp[row])
    ocol[at], oval[at] = col, val
    tail = orp[1:][has] - 2
    ocol[tail], oval[tail], ocol[tail + 1], oval[tail + 1] = m.p, mean[has], m.p + 1, cnt[has]
    return engine.Matrix.from_csr(orp, ocol, oval, m.p + 2, y)


def _torch_routes(torch, m, part, lo, W, n_terms_fixed):
    """(fit, apply) closures over tensors that are already on the device"""
    rp, col, val, y = m.export()
    lens = np.diff(rp)
    row = np.repeat(np.arange(m.n, dtype=np.int64), lens)
    t_col = torch.from_numpy(col.astype(np.int64)).cuda()
    t_val = torch.from_numpy(val).cuda()
    t_row = torch.from_numpy(row).cuda()
    t_part = torch.from_numpy(part.astype(np.int64)).cuda()
    t_pos = torch.from_numpy((y > 0).astype(np.int64)).cuda()
    t_rp, t_lens = torch.from_numpy(rp[:-1].copy()).cuda(), torch.from_numpy(lens).cuda()
    del rp, col, val, row
    state = {}

    def fit():
        inside = (t_col >= lo) & (t_col < lo + W)
        r = t_row[inside]
        key = (t_col[inside] - lo) * FOLDS + t_part[r]
        if not n_terms_fixed:
            pairs = torch.unique(key * m.n + r)
            key, r = pairs // m.n, pairs % m.n
        rows = torch.bincount(key, minlength=W * FOLDS)
        pos = torch.bincount(key, weights=t_pos[r].double(), minlength=W * FOLDS).long()
        state["count"] = torch.stack([rows, pos], dim=1).view(W, FOLDS, 2)
        torch.cuda.synchronize()
        return int(W)

    def apply():
        count = state["count"]
        tot = count.sum(dim=1)
        inside = (t_col >= lo) & (t_col < lo + W)
        r = t_row[inside]
        slot = t_col[inside] - lo
        own = count[slot, t_part[r]]
        dn, da = tot[slot, 0] - own[:, 0], tot[slot, 1] - own[:, 1]
        if not n_terms_fixed:
            dn = torch.zeros(m.n, dtype=torch.int64, device=dn.device).index_add_(0, r, dn)
            da = torch.zeros(m.n, dtype=torch.int64, device=da.device).index_add_(0, r, da)
        den = dn.double() + STRENGTH
        mean = torch.where(den == 0, torch.tensor(PRIOR, dtype=torch.float64, device=den.device), (da.double() + PRIOR * STRENGTH) / den).float()
        cnt = dn.float()
        if n_terms_fixed:
            T, L = n_terms_fixed, int(lens[0])
            oval = torch.empty((m.n, L + 2 * T), dtype=torch.float32, device=mean.device)
            ocol = torch.empty((m.n, L + 2 * T), dtype=torch.int64, device=mean.device)
            ocol[:, :L], oval[:, :L] = t_col.view(m.n, L), t_val.view(m.n, L)
            ocol[:, L:] = m.p + torch.arange(2 * T, device=mean.device)
            oval[:, L::2], oval[:, L + 1::2] = mean.view(m.n, T), cnt.view(m.n, T)
        else:   # the ragged merge: every row that holds the bag gets two entries behind its own
            has = torch.bincount(r, minlength=m.n) > 0
            olen = t_lens + 2 * has
            orp = torch.zeros(m.n + 1, dtype=torch.int64, device=mean.device)
            orp[1:] = torch.cumsum(olen, 0)
            total = int(orp[-1])
            ocol = torch.empty(total, dtype=torch.int64, device=mean.device)
            oval = torch.empty(total, dtype=torch.float32, device=mean.device)
            at = orp[t_row] + (torch.arange(t_col.shape[0], device=mean.device) - t_rp[t_row])
            ocol[at], oval[at] = t_col, t_val
            tail = orp[1:][has] - 2
            ocol[tail], oval[tail], ocol[tail + 1], oval[tail + 1] = m.p, mean[has], m.p + 1, cnt[has]
        torch.cuda.synchronize()
        return int(oval.shape[0])
    return fit, apply, state


class _DevU32:
    """a uint32 array on the device, through the HIP runtime the library is linked against"""

    def __init__(self, a):
        import ctypes as C
        from fmwr_amd import _lib
        _lib.lib()
        hip = C.CDLL("libamdhip64.so.7")
        a = np.ascontiguousarray(a, np.uint32)
        self.ptr = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.ptr), C.c_size_t(max(a.nbytes, 4))) == 0
        assert hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), C.c_int(1)) == 0


def _make(args, which):
    """(Matrix, segment_base, term_segment, lo, W, fixed terms, what)"""
    from fmwr_amd import engine
    if which == "a":
        n = int(10_000_000 * args.n_scale)
        m = engine.Matrix.synthetic_fields(n, 13, engine.CRITEO_VOCAB, 3.0, 11)
        base = np.concatenate([np.arange(13), 13 + np.concatenate([[0], np.cumsum(engine.CRITEO_VOCAB)])]).astype(np.uint32)
        terms = np.arange(13, 39, dtype=np.uint32)
        lo, W, fixed = 13, int(sum(engine.CRITEO_VOCAB)), 26
        what = "synthetic_fields, 13 dense columns + 26 fields, all 26 fields encoded, 5 folds, MEAN + COUNT (fit: the sorted form -- the dense columns' values keep the source from being one-hot --, apply: the single form)"
    else:
        n = int(1_000_000 * args.n_scale)
        m = engine.Matrix.synthetic_ragged(n, 100_000, 30.0, 11, 1, 64)
        base, terms = np.array([0, 100_000], np.uint32), np.array([0], np.uint32)
        lo, W, fixed = 0, 100_000, 0
        what = "ragged rows, Poisson(30) entries in [1, 64] over 100 000 columns, the one bag segment encoded, 5 folds, MEAN + COUNT (fit: the unit form, apply: the group form)"
    return m, base, terms, lo, W, fixed, what


def _trace(args, which):
    """the device route alone, one warm-up and --reps calls of the fit and of the apply: the run to put under a kernel trace"""
    from fmwr_amd import engine
    m, base, terms, lo, W, fixed, what = _make(args, which)
    dpart = _DevU32(engine.split_assign(m.n, n_folds=FOLDS, seed=3))
    kinds = np.full(len(terms), 3, np.uint32)
    for _ in range(args.reps + 1):
        t = m.target_stats_device(dpart.ptr, base, terms, n_parts=FOLDS)
        out, _ = m.encode_targets(t, kinds=kinds, prior=PRIOR, strength=STRENGTH, dev_part=dpart.ptr)
        out.close()
        t.free()
    print("traced", which, args.reps + 1, "calls of the fit and of the apply;", m.n, "rows,", m.nnz, "entries")
    m.close()


def _shape(args, torch, which):
    from fmwr_amd import engine
    m, base, terms, lo, W, fixed, what = _make(args, which)
    part = engine.split_assign(m.n, n_folds=FOLDS, seed=3)
    dpart = _DevU32(part)
    kinds = np.full(len(terms), 3, np.uint32)
    held = {}

    def dev_fit():
        t = m.target_stats_device(dpart.ptr, base, terms, n_parts=FOLDS)
        w = t.width
        t.free()
        return w

    def dev_apply():
        out, _ = m.encode_targets(held["table"], kinds=kinds, prior=PRIOR, strength=STRENGTH, dev_part=dpart.ptr)
        k = out.nnz
        out.close()
        return k

    def host_fit():
        count, _ = _host_fit(m, part, lo, W, bool(fixed))
        t = engine.TargetTable.from_arrays(base, terms, count)
        t.free()
        return W

    def host_apply():
        out = _host_apply(m, held["count"], part, lo, W, fixed)
        k = out.nnz
        out.close()
        return k
    # the routes agree before anything is timed
    held["table"] = m.target_stats_device(dpart.ptr, base, terms, n_parts=FOLDS)
    held["count"], exported = _host_fit(m, part, lo, W, bool(fixed))
    assert np.array_equal(held["table"].export()[0], held["count"])
    ref = _host_apply(m, held["count"], part, lo, W, fixed, exported[:4])
    got, _ = m.encode_targets(held["table"], kinds=kinds, prior=PRIOR, strength=STRENGTH, dev_part=dpart.ptr)
    k = min(m.n, 2000)
    a, b = got.export(0, k), ref.export(0, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))
    out_nnz, in_nnz, encoded = got.nnz, m.nnz, int(exported[5].sum())
    got.close(); ref.close()
    del exported, a, b
    fit_routes, apply_routes = {"device": dev_fit, "host": host_fit}, {"device": dev_apply, "host": host_apply}
    if torch is not None:
        tf, ta, tstate = _torch_routes(torch, m, part, lo, W, fixed)
        tf()
        assert np.array_equal(tstate["count"].cpu().numpy(), held["count"])     # the same table as the library's
        fit_routes["torch"], apply_routes["torch"] = tf, ta
    out = {"what": what, "rows": m.n, "entries": in_nnz, "encoded_entries": encoded, "out_entries": out_nnz, "slots": W, "table_bytes": held["table"].device_bytes}
    for step, routes in (("fit", fit_routes), ("apply", apply_routes)):
        res = _alternate(routes, args.reps, settle=("device",))
        res["device_vs_host"] = _verdict(res, "device", "host")
        if "torch" in routes:
            res["device_vs_torch"] = _verdict(res, "device", "torch")
        res["device"]["bound_s"] = encoded / LINES_PER_S
        out[step] = res
    held["table"].free()
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of a, b; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--trace", action="store_true", help="run the device route alone (for rocprofv3 --kernel-trace --stats); writes nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "target.json"))
    args = ap.parse_args()
    shapes = ["a", "b"] if args.shape == "all" else args.shape.split(",")
    if args.trace:
        for s in shapes:
            _trace(args, s)
        return
    torch = None
    if not args.no_torch:
        import torch
        torch.cuda.init()  # before libfmx: the same process
    record = {"reps": args.reps, "n_scale": args.n_scale, "shapes": {}}
    if os.path.exists(args.out):   # shapes measured by an earlier call of this script stay
        old = json.load(open(args.out))
        if old.get("reps") == args.reps and old.get("n_scale") == args.n_scale:
            record["shapes"] = old["shapes"]
    for s in shapes:
        record["shapes"][s] = _shape(args, torch, s)
        print(s, json.dumps(record["shapes"][s]), flush=True)
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
    ms = lambda o: f"{o['median_s'] * 1e3:10.1f} ms  [{o['min_s'] * 1e3:.1f}, {o['max_s'] * 1e3:.1f}]"
    lines = ["target encoding on the device against export -> numpy -> from_arrays / from_csr, and against torch on the same device (profiles/target_bench.py; "
             "medians of %d alternated calls, [min, max]; rows scaled by %g; every timed device call follows an untimed one of itself)" % (args.reps, args.n_scale)]
    for s, o in record["shapes"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries in, {o['encoded_entries']:,} of them encoded, {o['out_entries']:,} out, "
                     f"{o['slots']:,} slots, a table of {o['table_bytes'] / 1e9:.2f} GB")
        for step in ("fit", "apply"):
            r = o[step]
            lines.append(f"  {step}")
            for v in ("device", "host", "torch"):
                if v in r:
                    lines.append(f"    {v:7s} {ms(r[v])}")
            for other in ("host", "torch"):
                g = r.get("device_vs_" + other)
                if g:
                    gate = "" if g["verdict"] == "faster" else "  ** THE GATE IS MISSED **"
                    lines.append(f"    {other} / device = {g['ratio']:.2f}x: the device route is {g['verdict']}{gate}")
            lines.append(f"    the gather bound ({o['encoded_entries']:,} lines of 128 bytes at 56.7 G lines/s) is {r['device']['bound_s'] * 1e3:.2f} ms, the call takes "
                         f"{r['device']['median_s'] / r['device']['bound_s']:.1f}x that -- the whole call, not the kernel alone (a figure, not a gate)")
    with open(os.path.splitext(args.out)[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
