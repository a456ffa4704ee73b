"""Feature crosses on the device (fmx_matrix_cross) measured against the only route the library offered before -- Matrix.export ->
tests/cross_model.py (numpy) -> Matrix.from_csr -- and, on shape (a), beside a torch gather-and-multiply formulation on the same device that is
handed the arrays for free and leaves its result as tensors.  Writes profiles/cross.json and the timing part of profiles/cross.txt (what that
file holds from the line "---- end to end" on, the accuracies of tests/test_gpu_cross.py, is kept).

Shapes:
  a  synthetic_fields(10 M rows, 13 dense columns, the 26 Criteo-shaped fields), 8 field pairs hashed into 2^20 buckets each: the single form.
  b  the same with fmx_debug_cross_limits(single = -1): the group form.  (a and b are timed in one alternation with one host route.)
  c  1 M ragged rows, Poisson(30) entries in [1, 64], one self-cross of the bag hashed into 2^22 buckets: the group form's pair enumeration.
Per shape, in one process, after one warm-up call of each route, --reps rounds with the routes alternated (median, [min, max]).  The gate: the
device route is faster than the host round trip by more than the spread of either side.  Figures beside it: the call against its byte bound
(entries read plus written x 8 B at 8 TB/s), and hipMalloc + hipFree of the output's arrays alone, which is the allocation's share of the call."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_BPS = 8e12


def _stats(ts):
    ts = sorted(ts)
    return {"median_s": ts[len(ts) // 2], "min_s": ts[0], "max_s": ts[-1], "reps": len(ts)}


def _alternate(versions, reps, settle=()):
    """settle: the routes that get one untimed call of themselves directly before every timed one.  The first device call behind the host route
    or the torch route took 1.2 .. 1.7 s where the same call repeated takes 6.5 ms (supposed, not measured: the allocator's state after gigabytes
    were released; the kernels are the same): whichever device route stood first in a round paid it, so the device routes are timed in their
    steady state"""
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


def _limits(single=0, group=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_cross_limits(single, group, rows))


def _alloc_only(sizes, reps):
    """hipMalloc + hipFree of the output's arrays, the way alloc_matrix and free_matrix make and release them"""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]

    def once():
        ps = []
        for b in sizes:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), b) == 0
            ps.append(p)
        for p in ps:
            assert hip.hipFree(p) == 0
    return _alternate({"alloc": once}, reps)["alloc"]


def _mix64(torch, x):
    """splitmix64's finaliser on int64 tensors: the multiplications wrap as uint64's do, the shifts are made logical by a mask"""
    x = x ^ ((x >> 30) & ((1 << 34) - 1)); x = x * torch.tensor(0xBF58476D1CE4E5B9 - (1 << 64), dtype=torch.int64, device=x.device)
    x = x ^ ((x >> 27) & ((1 << 37) - 1)); x = x * torch.tensor(0x94D049BB133111EB - (1 << 64), dtype=torch.int64, device=x.device)
    return x ^ ((x >> 31) & ((1 << 33) - 1))


def _torch_cross(torch, t_col, t_val, L, pos, bases, n_buckets, p, seed):
    """shape (a) in torch: a gather of the two positions, the hash in int64 arithmetic, the product; (col [n, L + T], val [n, L + T])"""
    from tests.split_model import mix64
    n = t_col.shape[0] // L
    c2, v2 = t_col.view(n, L), t_val.view(n, L)
    ocol = torch.empty((n, L + len(pos)), dtype=torch.int64, device=t_col.device)
    oval = torch.empty((n, L + len(pos)), dtype=torch.float32, device=t_col.device)
    ocol[:, :L], oval[:, :L] = c2, v2
    with np.errstate(over="ignore"):
        h0 = mix64(np.array([seed], np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    for t, ((pa, pb), (ba, bb)) in enumerate(zip(pos, bases)):
        with np.errstate(over="ignore"):
            h1 = int(mix64(h0 ^ (np.uint64(0) * np.uint64(0xD6E8FEB86659FD93) + np.uint64(128 + t)))[0])
        key = ((c2[:, pa] - ba) << 32) | (c2[:, pb] - bb)
        k = key + torch.tensor(0x632BE59BD9B4E019, dtype=torch.int64, device=key.device)
        h = _mix64(torch, torch.tensor(h1 - (1 << 64) if h1 >= 1 << 63 else h1, dtype=torch.int64, device=key.device) ^ k)
        hi, lo = (h >> 32) & 0xFFFFFFFF, h & 0xFFFFFFFF
        ocol[:, L + t] = p + t * n_buckets + ((hi * n_buckets + ((lo * n_buckets) >> 32)) >> 32)
        oval[:, L + t] = v2[:, pa] * v2[:, pb]
    torch.cuda.synchronize()
    return ocol, oval


def _run(m, base, terms, reps, forms, torch_route=None):
    from fmwr_amd import engine
    from tests import cross_model as cm

    def device(single):
        def f():
            _limits(single)
            out, cb = m.cross(base, terms, seed=7)
            k = out.nnz
            out.close()
            _limits()
            return k
        return f

    def host():
        rp, col, val, y = m.export()
        orp, ocol, oval, cb = cm.cross(rp, col, val, m.p, base, terms, 7)
        out = engine.Matrix.from_csr(orp, ocol, oval, int(cb[-1]), y)
        k = out.nnz
        out.close()
        return k
    # the routes agree before anything is timed
    a, cb = m.cross(base, terms, seed=7)
    rp, col, val, y = m.export()
    ref = cm.cross(rp, col, val, m.p, base, terms, 7)
    got = a.export()
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
    out_nnz, out_p = a.nnz, a.p
    a.close()
    del rp, col, val, y, ref, got
    routes = {name: device(single) for name, single in forms.items()}
    routes["host"] = host
    if torch_route is not None:
        routes["torch"] = torch_route
    out = _alternate(routes, reps, settle=tuple(forms))
    for name in forms:
        out[name + "_vs_host"] = _verdict(out, name, "host")
        if torch_route is not None:
            out[name + "_vs_torch"] = _verdict(out, name, "torch")
        out[name]["bound_s"] = 8.0 * (m.nnz + out_nnz) / PEAK_BPS
    out["alloc"] = _alloc_only([8 * (m.n + 1), 4 * out_nnz, 4 * out_nnz, 4 * m.n], reps)
    out.update(rows=m.n, entries=m.nnz, out_entries=out_nnz, out_features=out_p)
    return out


def _shape(args, torch, which):
    from fmwr_amd import engine
    if which == "ab":
        n = int(10_000_000 * args.n_scale)
        m = engine.Matrix.synthetic_fields(n, 13, engine.CRITEO_VOCAB, 3.0, 11)
        base = np.concatenate([np.arange(13), 13 + np.concatenate([[0], np.cumsum(engine.CRITEO_VOCAB)])]).astype(np.uint32)
        pairs = [(13 + 2 * i, 13 + 2 * i + 1) for i in range(8)]
        terms = [(a, b, 1 << 20) for a, b in pairs]
        torch_route = None
        if torch is not None:
            rp, col, val, _ = m.export()
            t_col, t_val = torch.from_numpy(col.astype(np.int64)).cuda(), torch.from_numpy(val).cuda()
            del rp, col, val
            bases = [(int(base[a]), int(base[b])) for a, b in pairs]

            def torch_route():
                return _torch_cross(torch, t_col, t_val, 39, pairs, bases, 1 << 20, m.p, 7)[0].shape[0]
            oc, _ = _torch_cross(torch, t_col, t_val, 39, pairs, bases, 1 << 20, m.p, 7)
            chk, _ = m.cross(base, terms, seed=7)
            assert np.array_equal(oc[:1000].cpu().numpy().ravel(), chk.export(0, 1000)[1].astype(np.int64))     # the same ids as the library's
            chk.close()
            del oc
        out = _run(m, base, terms, args.reps, {"single": 0, "group": -1}, torch_route)
        out["what"] = "synthetic_fields, 13 dense columns + 26 fields, 8 field pairs hashed into 2^20 buckets each; single: the default, group: single = -1"
    else:
        n = int(1_000_000 * args.n_scale)
        m = engine.Matrix.synthetic_ragged(n, 100_000, 30.0, 11, 1, 64)
        out = _run(m, np.array([0, 100_000], np.uint32), [(0, 0, 1 << 22)], args.reps, {"group": 0})
        out["what"] = "ragged rows, Poisson(30) entries in [1, 64] over 100 000 columns, the bag crossed with itself into 2^22 buckets (the group form)"
    m.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", help="comma list of ab, c; or all")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-scale", type=float, default=1.0, help="fraction of the rows of every shape (quick checks)")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross.json"))
    args = ap.parse_args()
    torch = None
    if not args.no_torch:
        import torch
        torch.cuda.init()  # before libfmx: the same process
    shapes = ["ab", "c"] if args.shape == "all" else args.shape.split(",")
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
    lines = ["feature crosses on the device against export -> tests/cross_model.py -> from_csr, and against torch on the same device (profiles/cross_bench.py; "
             "medians of %d alternated calls, [min, max]; rows scaled by %g; every timed device call follows an untimed one of itself: the first "
             "device call of a round, behind the host and the torch route, took 1.2 .. 1.7 s on shape (a) where the same call repeated takes 6.5 ms)" % (args.reps, args.n_scale)]
    for s, o in record["shapes"].items():
        lines.append(f"({s}) {o['what']}: {o['rows']:,} rows, {o['entries']:,} entries in, {o['out_entries']:,} out, {o['out_features']:,} features out")
        forms = [v for v in ("single", "group") if v in o]
        for v in forms + ["host"] + (["torch"] if "torch" in o else []):
            lines.append(f"    {v:7s} {ms(o[v])}")
        for v in forms:
            g = o[v + "_vs_host"]
            gate = "" if g["verdict"] == "faster" else "  ** THE GATE IS MISSED **"
            lines.append(f"    host / {v} = {g['ratio']:.1f}x: the device route is {g['verdict']}{gate}")
            if v + "_vs_torch" in o:
                lines.append(f"    torch / {v} = {o[v + '_vs_torch']['ratio']:.2f}x: the device route is {o[v + '_vs_torch']['verdict']} (a comparison, not the gate)")
            lines.append(f"    {v}: the byte bound ({8 * (o['entries'] + o['out_entries']) / 1e9:.2f} GB at 8 TB/s) is {o[v]['bound_s'] * 1e3:.2f} ms, the call takes "
                         f"{o[v]['median_s'] / o[v]['bound_s']:.1f}x that -- the whole call: the allocation, the detector's pass over the output and the waits included")
        lines.append(f"    hipMalloc + hipFree of the output's four arrays alone {ms(o['alloc'])}: " +
                     ", ".join(f"{o['alloc']['median_s'] / o[v]['median_s']:.0%} of the {v} call" for v in forms) + " (a figure, not a gate)")
    txt = os.path.splitext(args.out)[0] + ".txt"
    kept = open(txt).read() if os.path.exists(txt) else ""
    kept = kept[kept.index("---- end to end"):] if "---- end to end" in kept else ""
    with open(txt, "w") as f:
        f.write("\n".join(lines) + "\n" + ("\n" + kept if kept else ""))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
