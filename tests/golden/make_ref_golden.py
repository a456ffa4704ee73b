"""Regenerates tests/golden/ref_v1.npz / ref_v1.json: vectors produced by the REFERENCE's own classes.

Run by hand from the repo root, where the reference tree is present and `make -C oracle ref` has built
oracle/_ref/ref_harness (the reference's unmodified FM.h behind the project's stand-in oracle/ref/Rcpp.h):

    python tests/golden/make_ref_golden.py [--harness PATH] [--check | --sanitizer-report]

Every case is a dict of plain arrays (the INPUTS), handed to one fresh harness process (libc rand() is then in the state
of srand(1)); what the harness writes back are the reference's OUTPUTS.  Both are stored, so no test needs this file's
random streams.  A case may name a "_base" case whose inputs it inherits; those are stored once.

Before anything is written the generator asserts that the harness (a) gives the Appendix-B literals of tests/kat.py
exactly and (b) gives tests/golden/oracle_v1.npz bit for bit on the six problems of make_golden.py.  It then runs the
oracle (oracle/fm_oracle.c) on every case, and records per case whether the restatement was bit-equal and the largest
absolute disagreement: ref_v1.json holds the settings and those measurements.
"""
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from tests import kat, util  # noqa: E402
from tests.golden import make_golden as mg  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
NPZ, META = os.path.join(HERE, "ref_v1.npz"), os.path.join(HERE, "ref_v1.json")

OP_LEARN, OP_FORWARD, OP_EVALUATE, OP_MATRIX, OP_ALS_V, OP_ORDER = 1, 2, 3, 4, 5, 6
MCMC, ALS, SGD, FTRL, TDAP = 100, 200, 300, 500, 600  # util/Macros.h solver ids
SOLVER_ID = {"sgd": SGD, "ftrl": FTRL, "tdap": TDAP, "als": ALS, "mcmc": MCMC}
CLS, REG = oracle.CLASSIFICATION, oracle.REGRESSION
ALL_METRICS = [oracle.LL, oracle.AUC, oracle.ACC, oracle.RMSE, oracle.MSE, oracle.MAE]

_TYPES = {np.dtype(np.float64): b"d", np.dtype(np.float32): b"f", np.dtype(np.int32): b"i", np.dtype(np.uint32): b"u", np.dtype(np.int64): b"l"}
_DTYPES = {v: k for k, v in _TYPES.items()}


# ---------------------------------------------------------------------------------------------- the harness's container
def write_pack(path, arrays):
    with open(path, "wb") as f:
        for name, a in arrays.items():
            a = np.ascontiguousarray(np.atleast_1d(a))
            if a.dtype not in _TYPES:
                a = a.astype(np.float64)
            nb = name.encode()
            f.write(struct.pack("<I", len(nb)) + nb + _TYPES[a.dtype] + struct.pack("<Q", a.size) + a.ravel().tobytes())


def read_pack(path):
    out, b, i = {}, open(path, "rb").read(), 0
    while i < len(b):
        (nl,) = struct.unpack_from("<I", b, i); i += 4
        name = b[i:i + nl].decode(); i += nl
        dt = _DTYPES[b[i:i + 1]]; i += 1
        (cnt,) = struct.unpack_from("<Q", b, i); i += 8
        out[name] = np.frombuffer(b, dt, cnt, i).copy(); i += cnt * dt.itemsize
    return out


def run_harness(inputs, harness=HARNESS):
    """One case through one fresh process of the reference harness -> dict of its outputs."""
    with tempfile.TemporaryDirectory() as d:
        write_pack(os.path.join(d, "case"), inputs)
        r = subprocess.run([harness, os.path.join(d, "case"), os.path.join(d, "result")], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{harness} ended with {r.returncode}:\n{r.stderr[-3000:]}")
        return read_pack(os.path.join(d, "result"))


# ---------------------------------------------------------------------------------------------- the cases
def _learn_case(solver, rp, col, val, y, p, w0, w, v, iters, Pm, **extra):
    c = dict(op=OP_LEARN, solver=SOLVER_ID[solver], task=Pm.task, k=Pm.k, k0=Pm.k0, k1=Pm.k1, p=p, row_ptr=np.asarray(rp, np.int64),
             col=np.asarray(col, np.uint32), val=np.asarray(val, np.float32), y=np.asarray(y, np.float32), w0_in=float(w0), w_in=np.asarray(w, np.float64),
             v_in=np.asarray(v, np.float64).reshape(Pm.k, p), l1_regw=Pm.l1_regw, l1_regv=Pm.l1_regv, l2_reg0=Pm.l2_reg0, l2_regw=Pm.l2_regw,
             l2_regv=Pm.l2_regv, min_target=Pm.min_target, max_target=Pm.max_target, learn_rate=Pm.learn_rate, alpha_w=Pm.alpha_w,
             beta_w=Pm.beta_w, alpha_v=Pm.alpha_v, beta_v=Pm.beta_v, gamma=Pm.gamma, random_step=Pm.random_step, max_iter=iters,
             trace_step=Pm.trace_step, eval_type=Pm.eval_type, conv_condition=Pm.conv_condition)
    c.update(extra)
    return c


def params_of(c):
    """oracle.Params of a stored learner / forward case."""
    g = lambda k, d=0.0: float(np.ravel(c[k])[0]) if k in c else d
    return oracle.params(task=int(g("task")), k=int(g("k")), k0=bool(g("k0", 1)), k1=bool(g("k1", 1)), l1_regw=g("l1_regw"), l1_regv=g("l1_regv"),
                         l2_reg0=g("l2_reg0"), l2_regw=g("l2_regw"), l2_regv=g("l2_regv"), min_target=g("min_target", -1.0), max_target=g("max_target", 1.0),
                         learn_rate=g("learn_rate", 0.01), alpha_w=g("alpha_w", 0.1), beta_w=g("beta_w", 1.0), alpha_v=g("alpha_v", 0.1),
                         beta_v=g("beta_v", 1.0), random_step=int(g("random_step", 1)), eval_type=int(g("eval_type", 0)),
                         trace_step=int(g("trace_step", -1)), conv_condition=g("conv_condition", 1e-4), gamma=g("gamma", 1e-4))


def odd_rows_matrix(seed, n=48, p=20):
    """Rows the generators elsewhere never make: an empty row, single-entry rows, one row that stores a column twice
    (SURVEY A-11) and one whose columns are not ascending."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        m = int(rng.integers(2, 6))
        rows.append(sorted(rng.choice(p, m, replace=False).tolist()))
    rows[3] = []
    rows[7] = [int(rng.integers(0, p))]
    rows[20] = [5]
    rows[11] = [2, 9, 9, 14]          # column 9 stored twice
    rows[12] = [2, 9, 2]              # and twice, not adjacent
    rows[17] = [15, 4, 11, 0]         # not ascending
    rows[n - 1] = []                  # the last row empty: the Iterator's read one past the end is at the arrays' end
    rp = np.zeros(n + 1, np.int64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([c for r in rows for c in r], np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    return rp, col, val


def learner_cases():
    cases = {}
    for name, c in mg.CASES.items():
        rp, col, val, y, w0, w, v, Pm = mg.problem(name, c)
        cases[name] = _learn_case(c["solver"], rp, col, val, y, mg.P, w0, w, v, mg.ITERS, Pm, with_pred=1)
    more = {
        "sgd_no_w0": ("sgd_l2_cls", dict(solver="sgd", task=CLS, k=4, k0=False, l2_regw=1e-3, l2_regv=2e-3, learn_rate=0.05)),
        "sgd_no_w1": ("sgd_l2_cls", dict(solver="sgd", task=CLS, k=4, k1=False, l2_regw=1e-3, l2_regv=2e-3, learn_rate=0.05)),
        "sgd_k0": ("sgd_l2_cls", dict(solver="sgd", task=CLS, k=0, l2_reg0=1e-3, l2_regw=1e-3, learn_rate=0.05)),
        "ftrl_k0": ("sgd_l2_cls", dict(solver="ftrl", task=CLS, k=0, l1_regw=1e-3, l2_regw=1e-2)),
        "tdap_no_w0": ("sgd_l2_cls", dict(solver="tdap", task=CLS, k=2, k0=False, l1_regw=1e-3, l2_regw=1e-2, l2_regv=1e-2, gamma=3e-4)),
        "sgd_l1_and_l2": ("sgd_l2_cls", dict(solver="sgd", task=CLS, k=4, l1_regw=1e-3, l1_regv=5e-4, l2_regw=5e-2, l2_regv=5e-2, learn_rate=0.05)),
        "sgd_l1_reg": ("sgd_l2_reg", dict(solver="sgd", task=REG, k=4, l1_regw=2e-3, l1_regv=1e-3, l2_regw=5e-2, l2_regv=5e-2, learn_rate=0.02)),
        "sgd_reg_clamps": ("sgd_l2_reg", dict(solver="sgd", task=REG, k=4, l2_regw=1e-3, l2_regv=1e-3, learn_rate=0.02, min_target=-0.75, max_target=0.5)),
        "ftrl_reg_clamps": ("sgd_l2_reg", dict(solver="ftrl", task=REG, k=2, l1_regw=1e-3, l2_regw=1e-2, l2_regv=1e-2, min_target=-0.75, max_target=0.5)),
        "sgd_reg_nan_forward": ("sgd_l2_reg", dict(solver="sgd", task=REG, k=2, l2_regw=1e-3, l2_regv=1e-3, learn_rate=0.02, min_target=-0.75, max_target=0.5)),
        "sgd_reg_nan_finite": ("sgd_l2_reg", dict(solver="sgd", task=REG, k=2, l2_regw=1e-3, l2_regv=1e-3, learn_rate=0.02, min_target=-0.75, max_target=0.5)),
        "ftrl_rs3": ("sgd_l2_cls", dict(solver="ftrl", task=CLS, k=4, l1_regw=1e-3, l1_regv=1e-3, l2_regw=1e-2, l2_regv=1e-2, random_step=3)),
        "tdap_rs2": ("sgd_l2_cls", dict(solver="tdap", task=CLS, k=4, l1_regw=1e-3, l1_regv=5e-4, l2_regw=1e-2, l2_regv=1e-2, gamma=3e-4, alpha_v=0.05, random_step=2)),
    }
    for name, (base, c) in more.items():
        b = cases[base]
        seed = sum(map(ord, name))
        w0, w, v = util.params(mg.P, c["k"], seed, fp32=False)
        kw = {k: v_ for k, v_ in c.items() if k != "solver"}
        kw.setdefault("min_target", float(b["y"].min())); kw.setdefault("max_target", float(b["y"].max()))
        Pm = oracle.params(**kw)
        if name == "sgd_reg_nan_forward":   # inf - inf in the pairwise term: every row holding feature 7 predicts NaN, and std::min / std::max
            v[0, 7] = np.inf                # then leave max_target (their FIRST argument wherever the comparison is false)
        if name == "sgd_reg_nan_finite":    # the same NaN from FINITE parameters: s^2 and q overflow to inf, inf - inf
            v[0, 7] = 1e200
        full = _learn_case(c["solver"], b["row_ptr"], b["col"], b["val"], b["y"], mg.P, w0, w, v, mg.ITERS, Pm, with_pred=1)
        cases[name] = dict({k: v_ for k, v_ in full.items() if k not in ("row_ptr", "col", "val", "y", "p")}, _base=base)
    rp, col, val = odd_rows_matrix(4242)
    n, p = len(rp) - 1, 20
    for solver, kw in dict(sgd=dict(l2_regw=1e-3, l2_regv=2e-3, l2_reg0=1e-3, learn_rate=0.05), sgdl1=dict(l1_regw=1e-3, l1_regv=5e-4, learn_rate=0.05),
                           ftrl=dict(l1_regw=1e-3, l1_regv=1e-3, l2_regw=1e-2, l2_regv=1e-2),
                           tdap=dict(l1_regw=1e-3, l1_regv=5e-4, l2_regw=1e-2, l2_regv=1e-2, gamma=3e-4, alpha_v=0.05)).items():
        name = f"{solver}_odd_rows"
        y = util.labels(n, 4242)
        w0, w, v = util.params(p, 3, 4242 + len(solver), stdev=0.3, fp32=False)
        Pm = oracle.params(task=CLS, k=3, **kw)
        full = _learn_case(solver.replace("sgdl1", "sgd"), rp, col, val, y, p, w0, w, v, 150, Pm, with_pred=1)
        cases[name] = full if solver == "sgd" else dict({k: v_ for k, v_ in full.items() if k not in ("row_ptr", "col", "val", "y", "p")}, _base="sgd_odd_rows")
    return cases


def tracker_cases(learners):
    """The learners with the tracker on: every metric id, conv_condition 0 (never stops) and one large enough to stop."""
    cases = {}
    n, p = 60, 24
    rp, col, val = util.random_csr(n, p, 5, seed=909, empty_rows=False)   # no empty rows: two of them with unlike labels tie in AUC
    ycls, yreg = util.labels(n, 909), util.labels(n, 909, "regression")
    spec = {
        "trk_sgd_ll": ("sgd", CLS, oracle.LL, 0.0, dict(l2_regw=1e-3, l2_regv=2e-3, learn_rate=0.05)),
        "trk_sgd_ll_stops": ("sgd", CLS, oracle.LL, 10.0, dict(l2_regw=1e-3, l2_regv=2e-3, learn_rate=0.05)),
        "trk_sgd_acc_stops": ("sgd", CLS, oracle.ACC, 10.0, dict(l1_regw=1e-3, l1_regv=5e-4, learn_rate=0.05)),
        "trk_ftrl_auc": ("ftrl", CLS, oracle.AUC, 0.0, dict(l1_regw=1e-3, l1_regv=1e-3, l2_regw=1e-2, l2_regv=1e-2)),
        "trk_tdap_acc": ("tdap", CLS, oracle.ACC, 0.0, dict(l1_regw=1e-3, l2_regw=1e-2, l2_regv=1e-2, gamma=3e-4)),
        "trk_sgd_rmse": ("sgd", REG, oracle.RMSE, 0.0, dict(l2_regw=1e-3, l2_regv=1e-3, learn_rate=0.02)),
        "trk_sgd_mse_stops": ("sgd", REG, oracle.MSE, 10.0, dict(l2_regw=1e-3, l2_regv=1e-3, learn_rate=0.02)),
        "trk_ftrl_mae": ("ftrl", REG, oracle.MAE, 0.0, dict(l1_regw=1e-3, l2_regw=1e-2, l2_regv=1e-2)),
        "trk_tdap_rmse_clamped": ("tdap", REG, oracle.RMSE, 0.0, dict(l2_regw=1e-2, l2_regv=1e-2, gamma=3e-4, min_target=-0.75, max_target=0.5)),
    }
    first = None
    for name, (solver, task, metric, conv, kw) in spec.items():
        y = ycls if task == CLS else yreg
        w0, w, v = util.params(p, 2, sum(map(ord, name)), stdev=0.3, fp32=False)
        kw = dict(kw)
        kw.setdefault("min_target", float(y.min())); kw.setdefault("max_target", float(y.max()))
        Pm = oracle.params(task=task, k=2, eval_type=metric, trace_step=25, conv_condition=conv, **kw)
        full = _learn_case(solver, rp, col, val, y, p, w0, w, v, 130, Pm)
        if first is None:
            first, cases[name] = name, full
        else:
            cases[name] = dict({k: v_ for k, v_ in full.items() if k not in ("row_ptr", "col", "val", "p")}, _base=first)
    return cases


FORWARD_K = [0, 1, 3, 16, 64]


def forward_cases():
    """Model::predict / predict_batch / predict_prob with raw scores from about -40 to +40: both ends of the probit table
    (|x| > 5.2) and the logistic where 1 + exp(-x) rounds to 1 or overflows."""
    cases = {}
    n, p = 64, 32
    rp, col, val = util.random_csr(n, p, 6, seed=313, empty_rows=True)
    rng = np.random.default_rng(313)
    val = (val * np.repeat(np.linspace(0.02, 5.0, n), np.diff(rp))).astype(np.float32)   # small rows first, large rows last
    y = util.labels(n, 313)
    w = rng.normal(0, 2.5, p)
    first = None
    for k in FORWARD_K:
        v = rng.normal(0, 0.9 / np.sqrt(max(k, 1)), (k, p))
        for solver, task in (("sgd", CLS), ("als", CLS), ("sgd", REG)):
            if task == REG and k not in (0, 3):
                continue
            name = f"fwd_k{k}_{solver}" + ("_reg" if task == REG else "")
            yy = y if task == CLS else util.labels(n, 313, "regression")
            c = dict(op=OP_FORWARD, solver=SOLVER_ID[solver], task=task, k=k, p=p, row_ptr=rp, col=col, val=val, y=yy, w0_in=0.3, w_in=w, v_in=v,
                     min_target=-1.5, max_target=2.25, eval_types=np.array([oracle.LL, oracle.ACC] if task == CLS else [oracle.RMSE, oracle.MAE], np.int32))
            if first is None:
                first, cases[name] = name, c
            else:
                drop = ("row_ptr", "col", "val", "p", "w_in", "w0_in") + (("y",) if task == CLS else ()) + (("v_in",) if solver != "sgd" or task == REG else ())
                cases[name] = dict({k_: v_ for k_, v_ in c.items() if k_ not in drop}, _base=first if solver == "sgd" and task == CLS else f"fwd_k{k}_sgd")
    return cases


def evaluation_cases():
    """evaluates() on hand-made vectors.  Equal |score| ACROSS the two classes is left out on purpose: the reference orders
    with std::sort, which is not stable, so it does not define AUC there."""
    rng = np.random.default_rng(5150)
    n = 41
    y = np.where(rng.random(n) < 0.45, -1.0, 1.0).astype(np.float32)
    yh = np.round(rng.random(n), 3) * 0.98 + 0.01
    pos, neg = np.flatnonzero(y > 0), np.flatnonzero(y < 0)
    yh[pos] = np.round(yh[pos], 2) + 0.001          # the classes' score sets are disjoint ...
    yh[neg] = np.round(yh[neg], 2) + 0.002
    yh[pos[:3]] = yh[pos[3]]                        # ... and ties exist inside each class
    yh[neg[:2]] = yh[neg[2]]
    edges = yh.copy()
    edges[pos[4]] = 0.5; edges[pos[5]] = 1.0; edges[neg[3]] = 0.0; edges[neg[4]] = 0.0   # one side each: no |score| shared by the classes
    zero_pos = yh.copy(); zero_pos[pos[4]] = 0.0; zero_pos[pos[5]] = 0.5   # log(0 + 1e-20) counts, and LL stays finite (no 1.0)
    one_class = edges.copy(); one_class[[1, 2]] = 0.5; one_class[[8, 9]] = 0.0
    both = dict(tasks=np.array([CLS] * 6 + [REG] * 6, np.int32), types=np.array(ALL_METRICS * 2, np.int32))
    yreg = rng.normal(0, 2, n).astype(np.float32)
    return {
        "eval_probabilities": dict(op=OP_EVALUATE, y_hat=yh, y=y, **both),
        "eval_exact_0_half_1": dict(op=OP_EVALUATE, y_hat=edges, y=y, **both),
        "eval_exact_0_on_positive": dict(op=OP_EVALUATE, y_hat=zero_pos, y=y, **both),
        "eval_single_class": dict(op=OP_EVALUATE, y_hat=one_class, y=np.ones(n, np.float32), **both),
        "eval_single_class_neg": dict(op=OP_EVALUATE, y_hat=one_class, y=-np.ones(n, np.float32), **both),
        "eval_real_valued": dict(op=OP_EVALUATE, y_hat=yreg + rng.normal(0, 0.5, n), y=yreg, **both),
    }


def matrix_cases():
    rng = np.random.default_rng(77)
    n, p = 30, 12
    dense = np.where(rng.random((n, p)) < 0.4, rng.normal(1.0, 2.0, (n, p)), 0.0)
    dense[:, 3] = 2.0                 # constant and fully stored: variance exactly 0, the 1e-30 guard divides
    dense[:, 5] = 0.0; dense[9, 5] = 1.75   # one stored entry
    dense[:, 8] = 0.0                 # no stored entry
    dense[np.flatnonzero((dense != 0).sum(1) == 0), 0] = 1.0   # SMatrix::transpose has no defined result with an empty row
    rows, cols = np.nonzero(dense)
    rp = np.zeros(n + 1, np.int64); np.add.at(rp, rows + 1, 1); rp = np.cumsum(rp)
    val = dense[rows, cols].astype(np.float32)
    mean = rng.normal(0, 1, p); std = rng.uniform(0.5, 2.0, p); std[[2, 5]] = 0.0
    base = dict(op=OP_MATRIX, p=p, row_ptr=rp, col=cols.astype(np.uint32), val=val, norm_mean=mean, norm_std=std)
    return {
        "mat_partial_columns": dict(base, norm_columns=np.array([0, 3, 5, 8, 10], np.int32)),
        "mat_all_columns": dict(_base="mat_partial_columns", op=OP_MATRIX, norm_columns=np.arange(p, dtype=np.int32), norm_mean=mean, norm_std=std, do_transpose=0),
        "mat_no_columns": dict(_base="mat_partial_columns", op=OP_MATRIX, norm_columns=np.array([-1], np.int32), norm_mean=mean, norm_std=std, do_transpose=0),
    }


ALS_N, ALS_P, ALS_K, ALS_ITERS = 120, 30, 3, 4


def als_cases():
    cases = {}
    n, p, k = ALS_N, ALS_P, ALS_K
    rp, col, val = util.random_csr(n, p, 5, seed=61, empty_rows=False)   # SMatrix::transpose needs every row non-empty
    ycls, yreg = util.labels(n, 61), util.labels(n, 61, "regression")
    w0, w, v = util.params(p, k, 61, stdev=0.3, fp32=False)
    first = None
    for name, solver, task, trace, scale in (("als_reg", "als", REG, -1, 1.0), ("als_cls", "als", CLS, -1, 20.0), ("als_reg_tracked", "als", REG, 2, 1.0),
                                             ("als_cls_tracked", "als", CLS, 3, 20.0), ("mcmc_reg", "mcmc", REG, -1, 1.0), ("mcmc_cls", "mcmc", CLS, -1, 8.0),
                                             ("mcmc_reg_tracked", "mcmc", REG, 3, 1.0), ("mcmc_cls_tracked", "mcmc", CLS, 2, 8.0)):
        y = ycls if task == CLS else yreg
        Pm = oracle.params(task=task, k=k, l2_reg0=0.05, min_target=float(y.min()), max_target=float(y.max()), trace_step=trace,
                           eval_type=oracle.LL if task == CLS else oracle.RMSE)
        full = _learn_case(solver, rp, col, val, y, p, w0, w * scale, v, ALS_ITERS, Pm)   # scale: scores beyond +-3 and +-5.2, the tables' saturated ends
        if first is None:
            first, cases[name] = name, full
        else:
            cases[name] = dict({k_: v_ for k_, v_ in full.items() if k_ not in ("row_ptr", "col", "val", "p", "v_in")}, _base=first)
    # the V sweep and the V hyper-parameter updates, which update_all keeps commented out (SURVEY A-1): through a subclass
    e0 = oracle.predict_batch(oracle.params(task=REG, k=k), oracle.Matrix(rp, col, val, p), w0, w, v.ravel()) - yreg
    lam, mu = np.array([0.0, 0.1, 0.5]), np.array([0.0, 0.05, -0.05])
    sweep = dict(_base=first, op=OP_ALS_V, solver=ALS, task=REG, k=k, y=yreg, w0_in=w0, w_in=w, max_iter=1, err_in=e0, alpha=1.3, v_lambda=lam, v_mu=mu, do_sweep=1, do_hyper=0)
    cases["als_vsweep"] = sweep
    bad = e0.copy(); bad[5] = np.inf; bad[40] = np.nan       # CHECK_PARAM: every column that meets row 5 or 40 keeps its old value
    vbig = v.copy(); vbig[1, 7] = 1e200                      # and a V entry whose square overflows
    cases["als_vsweep_guards"] = dict(sweep, err_in=bad, v_in=vbig)
    cases["mcmc_vsweep"] = dict(sweep, solver=MCMC)
    cases["mcmc_vhyper"] = dict(sweep, solver=MCMC, do_sweep=0, do_hyper=1, v_lambda=np.array([0.7, 0.1, 0.5]))
    cases["als_vhyper"] = dict(sweep, do_sweep=0, do_hyper=1)
    del cases["mcmc_vhyper"]["err_in"], cases["als_vhyper"]["err_in"]
    return cases


def order_cases():
    return {f"order_rs{rs}": dict(op=OP_ORDER, n=mg.N, random_step=rs, max_iter=mg.ITERS) for rs in (1, 2, 3)}


FAMILIES = dict(learners=learner_cases, tracker=None, forward=forward_cases, evaluation=evaluation_cases, matrix=matrix_cases, als_mcmc=als_cases, order=order_cases)


def all_cases():
    """{family: {case: inputs}}."""
    out = {}
    for fam, fn in FAMILIES.items():
        out[fam] = tracker_cases(out["learners"]) if fam == "tracker" else fn()
    return out


def resolve(cases, name):
    """Inputs of a case with everything it inherits from its _base chain."""
    c = cases[name]
    if "_base" in c:
        full = dict(resolve(cases, c["_base"]))
        full.update({k: v for k, v in c.items() if k != "_base"})
        return full
    return dict(c)


# ---------------------------------------------------------------------------------------------- the restatement, case by case
def _order_of(c):
    return oracle.visit_order(len(c["row_ptr"]) - 1, int(np.ravel(c["random_step"])[0]), int(np.ravel(c["max_iter"])[0]), seed=1)


def oracle_outputs(c, ref):
    """What oracle/fm_oracle.c gives for the resolved inputs `c`: {key: array}, keys a subset of the reference's outputs.
    `ref` supplies only what the reference LOGGED for the caller (the standard variates it drew) -- never an expected value."""
    one = lambda k, d=None: np.ravel(c[k])[0] if k in c else d
    op = int(one("op"))
    out = {}
    if op == OP_ORDER:
        return dict(order=oracle.visit_order(int(one("n")), int(one("random_step")), int(one("max_iter")), seed=1))
    if op == OP_EVALUATE:
        return dict(eval=np.array([oracle.evaluate(int(t), int(m), c["y_hat"], c["y"]) for t, m in zip(c["tasks"], c["types"])]))
    p = int(one("p"))
    if op == OP_MATRIX:
        n = len(c["row_ptr"]) - 1
        nc = np.asarray(c["norm_columns"], np.int32)
        sv, mean, std = oracle.scales(n, p, c["col"], c["val"], nc[nc >= 0])
        out.update(scaled_val=sv.astype(np.float64), mean=mean, std=std,
                   normalized_val=oracle.normalize(c["col"], c["val"], c["norm_mean"], c["norm_std"]).astype(np.float64))
        if int(one("do_transpose", 1)):
            cp, ri, vt = oracle.Matrix(c["row_ptr"], c["col"], c["val"], p).transpose()
            out.update(t_row_ptr=cp, t_col=ri.astype(np.int64), t_val=vt.astype(np.float64))
        return out
    P = params_of(c)
    X = oracle.Matrix(c["row_ptr"], c["col"], c["val"], p)
    k, solver = P.k, int(one("solver"))
    w0, w, v = float(one("w0_in")), np.asarray(c["w_in"], np.float64), np.asarray(c["v_in"], np.float64).ravel()
    if op == OP_FORWARD:
        n = X.n
        out["pred_row"] = np.array([oracle.predict(P, X, w0, w, v, i)[0] for i in range(n)])
        out["pred_batch"] = oracle.predict_batch(P, X, w0, w, v)
        out["prob"] = oracle.predict_batch(P, X, w0, w, v, prob="probit" if solver in (ALS, MCMC) else True)
        yh = np.clip(out["pred_batch"], P.min_target, P.max_target) if P.task == REG else out["prob"]
        out["report_eval"] = np.array([oracle.evaluate(P.task, int(t), yh, c["y"]) for t in c["eval_types"]])
        return out
    if op == OP_ALS_V:
        if int(one("do_hyper")):
            zg, zn = (ref["gamma_z"], ref["norm_z"]) if solver == MCMC else (np.zeros(k), np.zeros(k))
            if solver == MCMC:
                lam, mu = oracle.mcmc_v_hyper(k, p, v, zg, zn, c["v_lambda"], c["v_mu"], sample=True)
            else:   # the ALS learner: do_multilevel is off, so lambda stays and mu is reset to mu_0 = 0 (:448-452, :482-484)
                lam, mu = np.asarray(c["v_lambda"], np.float64), np.zeros(k)
            out.update(v_lambda_out=lam, v_mu_out=mu)
        if int(one("do_sweep")):
            zn = ref["norm_z"].reshape(k, p) if solver == MCMC else None
            v1, _, _ = oracle.als_update_v(k, X, v, c["err_in"], alpha=float(one("alpha")), v_lambda=c["v_lambda"], v_mu=c["v_mu"], znorm=zn)
            out["v"] = v1
        return out
    assert op == OP_LEARN
    iters = int(one("max_iter"))
    if solver in (SGD, FTRL, TDAP):
        fn = {SGD: oracle.sgd_learn, FTRL: oracle.ftrl_learn, TDAP: oracle.tdap_learn}[solver]
        order = oracle.visit_order(X.n, P.random_step, iters, seed=1)
        r = fn(P, X, c["y"], w0, w, v, iters, order=order, trace_cap=iters + 2 if P.trace_step > 0 else 0)
        out.update(w0=np.array([r["w0"]]), w=r["w"], v=r["v"], convergent=np.array([float(r["convergent"])]))
        if int(one("with_pred", 0)):
            out["pred"] = oracle.predict_batch(P, X, r["w0"], r["w"], r["v"])
        if P.trace_step > 0:
            out.update(rec_index=r["trace_iters"], rec_eval=r["trace_vals"])
            P0 = params_of(dict(c, trace_step=-1))
            snaps = [fn(P0, X, c["y"], w0, w, v, int(i) + 1, order=order[: int(i) + 1]) for i in r["trace_iters"]]   # a snapshot is the model after that example
            out.update(snap_w0=np.array([s["w0"] if P.k0 else 0.0 for s in snaps]), snap_w=np.concatenate([s["w"] for s in snaps]) if P.k1 else np.zeros(0),
                       snap_v=np.concatenate([s["v"] for s in snaps]) if k > 0 else np.zeros(0))
        return out
    y = c["y"]

    def recorded(it):   # MCMC_ALS_Learner.h:96-125: the START of iterations 0, step, 2 step, ... and of the last one
        return P.trace_step > 0 and (it % P.trace_step == 0 or it == iters - 1)

    def score(a0, aw, av):
        raw = oracle.predict_batch(P, X, a0, aw, av)
        yh = np.clip(raw, P.min_target, P.max_target) if P.task == REG else oracle.fast_pnorm(raw)
        return oracle.evaluate(P.task, P.eval_type, yh, y)

    snaps, evals = [], []
    if solver == ALS:
        if P.trace_step > 0:
            r0, rw, rv, it, ev = oracle.als_learn_traced(P, X, y, w0, w, v, iters)
            out.update(rec_index=it, rec_eval=ev)
            snaps = [oracle.als_learn(P, X, y, w0, w, v, int(i)) for i in it]   # a snapshot is the model after i iterations
        else:
            r0, rw, rv = oracle.als_learn(P, X, y, w0, w, v, iters)
    else:
        gz, nz = ref["gamma_z"].reshape(iters, 2), ref["norm_z"].reshape(iters, 2 + p)
        r0, rw, rv, st = w0, w, v, None
        for it in range(iters):   # the chain one iteration at a time, so that the tracker can look at the start of each
            if recorded(it):
                snaps.append((r0, rw.copy(), rv.copy())); evals.append(score(r0, rw, rv))
            r0, rw, rv, st = oracle.mcmc_learn(P, X, y, r0, rw, rv, 1, gz[it:it + 1], nz[it:it + 1], seed=1 if it == 0 else None, state=st)
        out.update(alpha=np.array([st[0]]), w_lambda=np.array([st[1]]), w_mu=np.array([st[2]]))
        if P.trace_step > 0:
            out.update(rec_index=np.array([it for it in range(iters) if recorded(it)], np.int64), rec_eval=np.array(evals))
    out.update(w0=np.array([r0]), w=rw, v=rv, convergent=np.array([0.0]))   # neither learner has a stopping rule
    if P.trace_step > 0:
        out.update(snap_w0=np.array([s_[0] for s_ in snaps]), snap_w=np.concatenate([s_[1] for s_ in snaps]), snap_v=np.concatenate([np.ravel(s_[2]) for s_ in snaps]))
    return out


# ---------------------------------------------------------------------------------------------- self-checks
def check_kat(harness):
    base = dict(op=OP_LEARN, task=CLS, k=kat.K, p=kat.P_FEAT, row_ptr=kat.ROW_PTR, col=kat.COL, val=kat.VAL, y=kat.Y, draw_v=1, init_stdev=kat.INIT_STDEV,
                l2_regw=kat.L2_REGW, l2_regv=kat.L2_REGV, min_target=-1.0, max_target=1.0, max_iter=kat.MAX_ITER, trace_step=kat.TRACE_STEP, eval_type=oracle.LL, conv_condition=0.0)
    r = run_harness(dict(base, solver=SGD, learn_rate=0.05, random_step=1), harness)
    assert r["w0"][0] == kat.SGD_W0 and r["w"].tolist() == kat.SGD_W and r["v"][: kat.P_FEAT].tolist() == kat.SGD_V0, "SGD known answers"
    assert np.array_equal(r["v_init"], kat.harness_v0()) and r["rec_index"].tolist() == kat.TRACE_ITERS
    assert [float(f"{x:.10g}") for x in r["rec_eval"]] == kat.SGD_LL, "SGD LL trace"
    r = run_harness(dict(base, solver=FTRL, l1_regw=0.001, l1_regv=0.001), harness)
    assert r["w0"][0] == kat.FTRL_W0 and [float(f"{x:.10g}") for x in r["rec_eval"]] == kat.FTRL_LL, "FTRL known answers"
    r = run_harness(dict(base, solver=TDAP, gamma=kat.TDAP_GAMMA), harness)
    assert r["w0"][0] == kat.TDAP_W0 and [float(f"{x:.10g}") for x in r["rec_eval"]] == kat.TDAP_LL, "TDAP known answers"


def check_oracle_v1(results):
    g = np.load(os.path.join(HERE, "oracle_v1.npz"))
    for name, c in mg.CASES.items():
        r = results[name]
        assert np.array_equal(oracle.visit_order(mg.N, c.get("random_step", 1), mg.ITERS, seed=1), g[f"{name}/order"]), name
        assert r["w0"][0] == float(g[f"{name}/w0"]) and np.array_equal(r["w"], g[f"{name}/w"]) and np.array_equal(r["v"].reshape(c["k"], mg.P), g[f"{name}/v"]), name


# ---------------------------------------------------------------------------------------------- the fixture
OUTPUT_DROP = ("step_size_used",)
ORACLE_V1_KEYS = ("row_ptr", "col", "val", "y", "w0_in", "w_in", "v_in")   # the six make_golden.py problems: inputs already in oracle_v1.npz
# Outputs that pass through the probit tables.  The oracle REGENERATES util/RandomData.h / RandomData_.h from their defining
# formulas (fm_oracle.c, "probit tables"); the shipped literals are those values rounded to 15 significant digits / 12
# decimals, so a table read differs by up to ~7e-16 / ~2e-12 and LL, which takes log of 1 - Phi near 1e-7, magnifies it.
TABLE_CAUSE = "probit grids regenerated from their formulas; bit-equal once the oracle reads the shipped grids (DESIGN.md section 2)"
BLANKET_ATOL = 1e-14


def shipped_tables():
    g = np.load(os.path.join(HERE, "probit_tables_full.npz"))
    return oracle.shipped_probit_tables(g["pnorm_x"], g["pnorm_y"], g["dpnorm_y"])


def _same(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if a.shape != b.shape:
        return False, float("inf")
    bit = bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin], b[~fin], equal_nan=True):
        return False, float("inf")
    return bit, float(np.max(np.abs(a[fin] - b[fin]))) if fin.any() else 0.0


def build(harness=HARNESS):
    """(cases, outputs, meta) in the form load() returns: every case through the harness, and the oracle measured against it."""
    meta, outs = dict(format=1, blanket_atol=BLANKET_ATOL, families={}, cases={}), {}
    fams = all_cases()
    flat = {name: c for cs in fams.values() for name, c in cs.items()}
    for fam, cs in fams.items():
        meta["families"][fam] = list(cs)
        for name in cs:
            full = resolve(flat, name)
            ref = run_harness(full, harness)
            want = oracle_outputs(full, ref)
            cmp = {}
            for key, val in want.items():
                bit, worst = _same(val, ref[key])
                cmp[key] = dict(bit_equal=bit, max_abs_diff=worst)
                if not bit:   # a bar of its own: four times what was measured, and the cause shown: the shipped grids remove it
                    with shipped_tables():
                        bit2, worst2 = _same(oracle_outputs(full, ref)[key], ref[key])
                    assert bit2, f"{name}/{key}: differs by {worst} and the probit tables do not explain it ({worst2} with the shipped ones)"
                    cmp[key].update(atol=4.0 * worst, cause=TABLE_CAUSE, bit_equal_with_shipped_tables=bit2)
            outs[name] = {key: val for key, val in ref.items() if key not in OUTPUT_DROP and (val.size or key in want)}
            meta["cases"][name] = dict(family=fam, base=flat[name].get("_base"), outputs=cmp)
    cases = {name: {k: np.asarray(v) for k, v in c.items() if k != "_base"} for name, c in flat.items()}
    for name, c in flat.items():
        if "_base" in c:
            cases[name]["_base"] = c["_base"]
    return cases, outs, meta


def save(cases, outs, meta):
    """Arrays to ref_v1.npz; settings (every 0-d input, exact through repr) and the measurements to ref_v1.json."""
    g1 = np.load(os.path.join(HERE, "oracle_v1.npz"))
    arrays = {}
    for name, c in cases.items():
        m = meta["cases"][name]
        m["settings"] = {}
        if name in mg.CASES:
            assert all(np.array_equal(np.asarray(c[k]).ravel(), g1[f"{name}/{k}"].ravel()) for k in ORACLE_V1_KEYS), name
            m["inputs_from_oracle_v1"] = True
        for key, val in c.items():
            if key == "_base" or (name in mg.CASES and key in ORACLE_V1_KEYS):
                continue
            if val.ndim == 0:
                m["settings"][key] = val.item()
            else:
                arrays[f"{name}/in/{key}"] = val
        for key, val in outs[name].items():
            arrays[f"{name}/out/{key}"] = val
    np.savez_compressed(NPZ, **arrays)
    json.dump(meta, open(META, "w"), sort_keys=True, separators=(",", ":"))
    return len(arrays)


def load():
    """(cases, outputs, meta) from the committed fixture: cases[name] = its own inputs (+ "_base"), outputs[name] = what the
    reference wrote.  resolve(cases, name) gives a case's full inputs."""
    g = np.load(NPZ)
    meta = json.load(open(META))
    cases, outs = {}, {n: {} for n in meta["cases"]}
    for n, m in meta["cases"].items():
        cases[n] = {k: np.asarray(v) for k, v in m["settings"].items()}
        if m["base"]:
            cases[n]["_base"] = m["base"]
        if m.get("inputs_from_oracle_v1"):
            g1 = np.load(os.path.join(HERE, "oracle_v1.npz"))
            cases[n].update({k: g1[f"{n}/{k}"] for k in ORACLE_V1_KEYS})
    for key in g.files:
        name, kind, field = key.split("/", 2)
        (cases if kind == "in" else outs)[name][field] = g[key]
    return cases, outs, meta


def differences(a, b):
    """Names of the arrays that are not bit for bit the same in two (cases, outputs) pairs."""
    bad = []
    for kind, x, y in (("in", a[0], b[0]), ("out", a[1], b[1])):
        for name in sorted(set(x) | set(y)):
            for key in sorted(set(x.get(name, {})) | set(y.get(name, {}))):
                u, v = x.get(name, {}).get(key), y.get(name, {}).get(key)
                if key == "_base":
                    ok = u == v
                else:
                    ok = u is not None and v is not None and np.asarray(u).dtype == np.asarray(v).dtype and np.asarray(u).tobytes() == np.asarray(v).tobytes()
                if not ok:
                    bad.append(f"{name}/{kind}/{key}")
    return bad


def summary(meta):
    lines = []
    for fam, names in meta["families"].items():
        outs = [(n, k, v) for n in names for k, v in meta["cases"][n]["outputs"].items()]
        worst = max(outs, key=lambda t: t[2]["max_abs_diff"])
        lines.append(f"{fam:11s} cases {len(names):3d}  vectors {len(outs):3d}  bit-equal {sum(v['bit_equal'] for _, _, v in outs):3d}  "
                     f"largest |diff| {worst[2]['max_abs_diff']:.3g} ({worst[0]}/{worst[1]})")
    return lines


def sanitizer_report(harness):
    """Every committed case through an instrumented build of the harness (make -C oracle ref-asan; a stand-alone program, on
    the CPU): what the sanitizers say per case, and whether the cases they let through still give the committed outputs."""
    cases, outs, _ = load()
    clean = 0
    for name in cases:
        try:
            ref = run_harness(resolve(cases, name), harness)
        except RuntimeError as e:
            what = [ln for ln in str(e).splitlines() if "SUMMARY" in ln or "runtime error" in ln]
            print(f"{name}: {what[:2] or str(e)[-400:]}")
            continue
        bad = [k for k, v in outs[name].items() if ref[k].tobytes() != v.tobytes()]
        assert not bad, f"{name}: the instrumented build gives other values in {bad}"
        clean += 1
    print(f"{clean} of {len(cases)} cases ran clean and bit-equal to the committed fixture")


def main(argv):
    harness = argv[argv.index("--harness") + 1] if "--harness" in argv else HARNESS
    if "--sanitizer-report" in argv:
        return sanitizer_report(harness)
    check_kat(harness)
    cases, outs, meta = build(harness)
    check_oracle_v1(outs)
    print("self-checks passed: Appendix-B known answers exact, oracle_v1.npz bit for bit")
    print("\n".join(summary(meta)))
    if "--check" in argv:
        old = load()
        bad = differences((cases, outs), old[:2])
        assert not bad, f"the committed fixture differs in {bad[:8]}"
        print("committed fixture reproduced bit for bit")
        return
    n = save(cases, outs, meta)
    print("wrote", n, "arrays,", os.path.getsize(NPZ), "+", os.path.getsize(META), "bytes")


if __name__ == "__main__":
    main(sys.argv[1:])
