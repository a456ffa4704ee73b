"""Why the TDAP cases of tests/step_cases.py's ladder take l2 = 0.3: the fp64 ORACLE with float32 inputs, no engine and no GPU involved.

Per step the oracle's exact gradient sums get the error the engine's number formats alone would cause -- every S row entry rounded to float32
(four times coarser at k = 16, where EMBED_BITS takes two mantissa bits of each factor), the multiplier rounded to float32 -- and after the
update w, V and the TDAP state are stored as float32; the arithmetic stays fp64.  Printed: max |V - V_pure| / max |V_pure| against the pure fp64
oracle, per (alpha, l2) and noise seed.  TDAP's first update of a coordinate jumps by alpha * sign(G), smoothed only over |G| ~ l1, alpha * l2:
small l2 turns rounding of the sums into errors of 1e-5 .. 1e-4 of max |V| on tiles with many once-touched coordinates.

    python profiles/tdap_fp32_amplification.py single_k32_onehot_tdap,single_k6_val_tdap 0.1:1e-3,0.1:0.1,0.1:0.3

Recorded output: profiles/step_forms_parity.txt."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402
from oracle import _ptr  # noqa: E402
from tests import step_cases as sc, util  # noqa: E402


def run(case, prob, start, alpha, l2, noisy, rng):
    P = sc.oracle_params(case); P.alpha_w = alpha; P.alpha_v = alpha; P.l2_regw = l2; P.l2_regv = l2
    p, k = prob["p"], case["k"]
    X = oracle.Matrix(prob["rp"], prob["col"], prob["val"], p)
    mb = oracle.TdapMinibatch(P, X, prob["y"], start[0], start[1], start[2].ravel())
    rp, col, val, y = prob["rp"], prob["col"].astype(np.int64), prob["val"].astype(np.float64), prob["y"]
    for b0, b1 in prob["oracle_steps"]:
        acc = oracle.batch_sums(P, X, y, mb.w0.value, mb.w, mb.v, b0, b1)
        if noisy:
            e0, e1 = rp[b0], rp[b1]
            c, x = col[e0:e1], val[e0:e1]
            row_of = np.repeat(np.arange(b1 - b0), np.diff(rp[b0:b1 + 1]))
            V = mb.v.reshape(k, p)
            s = np.zeros((b1 - b0, k)); np.add.at(s, row_of, x[:, None] * V[:, c].T)
            yh = oracle.predict_batch(P, X, mb.w0.value, mb.w, mb.v)[b0:b1]
            mult = np.array([oracle.grad_mult(P, float(a), float(b))[0] for a, b in zip(yh, y[b0:b1])])
            ulp = 2.0 ** -24 * (4.0 if k == 16 else 1.0)
            ds = np.abs(s) * ulp * rng.uniform(-1, 1, s.shape)
            dm = mult * 2.0 ** -24 * rng.uniform(-1, 1, mult.shape)
            dg = (mult[row_of] * x)[:, None] * ds[row_of] + (dm[row_of] * x)[:, None] * (s[row_of] - x[:, None] * V[:, c].T)
            Gv = acc["Gv"].reshape(k, p); np.add.at(Gv.T, c, dg)
            np.add.at(acc["Gw"], c, dm[row_of] * x)
        oracle.lib().fmo_tdap_apply_sums(C.byref(P), C.c_uint32(p), C.byref(mb.w0), _ptr(mb.w), _ptr(mb.v), C.c_double(b1 - b0), C.c_double(acc["G0"]), C.c_double(acc["Q0"]),
                                         _ptr(acc["Gw"]), _ptr(acc["Qw"]), _ptr(acc["cw"]), _ptr(acc["Gv"]), _ptr(acc["Qv"]), _ptr(mb.s0), _ptr(mb.sw), _ptr(mb.sv))
        if noisy:
            for name in ("w", "v", "sw", "sv"):
                a = getattr(mb, name); a[:] = a.astype(np.float32)
    return mb.w.copy(), mb.v.copy()

names = sys.argv[1].split(",")
combos = [tuple(map(float, c.split(":"))) for c in sys.argv[2].split(",")]
for case in sc.LADDER_CASES:
    if case["name"] not in names: continue
    prob = sc.ladder_problem(case["regime"], case["values"], case["seed"])
    start = sc.start_params(prob["p"], case["k"], case["seed"])
    out = []
    for alpha, l2 in combos:
        w, v = run(case, prob, start, alpha, l2, False, None)
        errs = []
        for trial in range(3):
            w2, v2 = run(case, prob, start, alpha, l2, True, np.random.default_rng(trial))
            errs.append(util.rel_err(v2, v))
        out.append("a=%g l2=%g: %s" % (alpha, l2, " ".join("%.1e" % e for e in errs)))
    print(case["name"], " | ".join(out), flush=True)
