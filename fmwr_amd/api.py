"""Python mirror of the reference's user-facing operator interface for the hot path.

The reference's host side for this path is R + Rcpp (R/fm_train.R, R/fm_update.R, R/fm_predict.R, R/fm_control.R,
R/fm_solver_control.R, R/fm_track_control.R, R/fm_matrix.R -> src/FM.cpp).  R is not available in this image, so the
same surface is mirrored here with the same names (dots -> underscores), argument meaning, defaults and error
messages, on top of the C ABI (include/fmx.h).  The Rcpp glue a maintainer would add is in INTEGRATION.md.

ALS runs for REGRESSION and CLASSIFICATION (probit tables regenerated, csrc/fm_probit.h); the MCMC solver runs with its
Gibbs draws taken from the numpy generator of fm_train(seed=...) instead of R's (same call order, include/fmx.h).  The tracker (track.control(step_size > 0), fm.track, fm.select: row f-1) runs on the device.
"""
import warnings

import numpy as np

from . import _lib as L
from .engine import Engine, Matrix, column_map_hash, column_map_select, join_bases, split_assign

_TASKS = {"CLASSIFICATION": L.TASK_CLASSIFICATION, "REGRESSION": L.TASK_REGRESSION, "RANK": L.TASK_RANKING}
_SOLVERS = {"SGD": L.SOLVER_SGD, "FTRL": L.SOLVER_FTRL, "ALS": L.SOLVER_ALS, "TDAP": L.SOLVER_TDAP, "MCMC": L.SOLVER_MCMC}

# R/fm_control.R:52-66
MODEL_CONTROL_DEFAULT = {
    "keep.w0": True, "L2.w0": 0.0, "keep.w1": True, "L1.w1": 0.0, "L2.w1": 0.0,
    "factor.number": 2, "v.init_mean": 0.0, "v.init_stdev": 0.01, "L1.v": 0.0, "L2.v": 0.0,
}
SGD_SOLVER_DEFAULT = {"learn_rate": 0.01, "random_step": 1}                                        # R/fm_solver_control.R:91-94
FTRL_SOLVER_DEFAULT = {"alpha_w": 0.1, "alpha_v": 0.1, "beta_w": 1.0, "beta_v": 1.0, "random_step": 1}  # :109-115
ALS_SOLVER_DEFAULT = {"alpha_0": 1.0, "gamma_0": 1.0, "beta_0": 1.0, "mu_0": 0.0, "alpha": 1.0, "w0_mean_0": 1.0,  # :64-71
                      "update_v": False}  # not in the reference: also run the V sweep its update_all leaves out


def _control_assign(default, given):
    """R/control_tools.R:1-37: overlay named arguments on the defaults, coerce integers, warn on unknown names."""
    out = dict(default)
    unknown = 0
    for name, value in given.items():
        key = name.replace("_", ".") if name.replace("_", ".") in default else name
        if key not in default:
            unknown += 1
            continue
        d = default[key]
        if isinstance(d, bool):
            if not isinstance(value, (bool, np.bool_)):
                raise TypeError(f"{key} must be logical")
        elif isinstance(d, int):
            iv = int(value)
            if iv != value:
                iv = max(d, iv)
                warnings.warn(f"{key} is not integer, it will be set as {iv}")
            value = iv
        out[key] = value
    if unknown:
        warnings.warn("some arguments are unknown...")
    return out


def model_control(task="CLASSIFICATION", **hyper):
    """model.control() -- R/fm_control.R:43-50."""
    if task not in ("CLASSIFICATION", "REGRESSION", "RANK"):
        raise ValueError("'arg' should be one of 'CLASSIFICATION', 'REGRESSION', 'RANK'")
    return {"class": "model.control", "task": task, "hyper.params": _control_assign(MODEL_CONTROL_DEFAULT, hyper)}


def SGD_solver(**kw):
    """SGD.solver() -- R/fm_solver_control.R:96-107."""
    return {"solver": "SGD", **_control_assign(SGD_SOLVER_DEFAULT, kw)}


def FTRL_solver(**kw):
    """FTRL.solver() -- R/fm_solver_control.R:117-130."""
    return {"solver": "FTRL", **_control_assign(FTRL_SOLVER_DEFAULT, kw)}


def ALS_solver(**kw):
    """ALS.solver() -- R/fm_solver_control.R:73-87 (its parameters are ignored by the reference too: SURVEY A-7)."""
    return {"solver": "ALS", **_control_assign(ALS_SOLVER_DEFAULT, kw)}


TDAP_SOLVER_DEFAULT = {"gamma": 1e-4, "alpha_w": 0.1, "alpha_v": 0.1, "random_step": 1}  # R/fm_solver_control.R:134-139


def TDAP_solver(**kw):
    """TDAP.solver() -- R/fm_solver_control.R:141-155 (row f-3; sequential mode = the shipped algorithm; mode="minibatch" = the mini-batch form defined in DESIGN.md section 4)."""
    return {"solver": "TDAP", **_control_assign(TDAP_SOLVER_DEFAULT, kw)}


def MCMC_solver(**kw):
    """MCMC.solver() -- R/fm_solver_control.R:36-62 (its parameters are ignored by the reference too: SURVEY A-7).
    The chain's Gamma / normal variates, which the reference takes from R's generator, are drawn here from the numpy
    generator seeded by fm_train(seed=...), in the reference's call order (include/fmx.h: fmx_mcmc_train)."""
    return {"solver": "MCMC", **_control_assign(ALS_SOLVER_DEFAULT, kw)}


def solver_control(max_iter=10000, solver=None):
    """solver.control() -- R/fm_solver_control.R:22-33 (default solver TDAP.solver(), as in the reference)."""
    solver = TDAP_solver() if solver is None else solver
    if solver["solver"] in ("MCMC", "ALS") and max_iter > 100:
        warnings.warn("the maximum number of iteratorions for MCMC/ALS solver is 100, so max_iter will be set to 100")
        max_iter = min(max_iter, 100)
    return {"class": "solver.control", "max_iter": int(max_iter), "solver": solver}


def track_control(step_size=-1, evaluate_metric="LL", convergence=1e-4):
    """track.control() -- R/fm_track_control.R:20-26."""
    if evaluate_metric not in ("AUC", "ACC", "LL", "RMSE", "MAE"):
        raise ValueError('evaluate.metric %in% c("AUC", "ACC", "LL", "RMSE", "MAE") is not TRUE')
    return {"class": "track.control", "max_iter": 1, "step_size": int(step_size), "evaluate.metric": evaluate_metric,
            "convergence": convergence}


class FmMatrix:
    """fm.matrix -- R/fm_matrix.R:6-43: features = list(value, col_idx, row_size, dim, size), labels."""

    def __init__(self, features, labels, feature_names):
        self.features, self.labels, self.feature_names = features, labels, feature_names

    @property
    def dim(self):
        return self.features["dim"]


def fm_matrix(data, labels=None, feature_names=None):
    """fm.matrix(): accepts a scipy.sparse matrix or a dense 2-D array (rows = cases, columns = features)."""
    import scipy.sparse as sp
    if labels is not None:
        labels = np.asarray(labels, np.float64)
        if labels.ndim != 1:
            raise ValueError("is.numeric(labels) is not TRUE")
        if np.any(np.isnan(labels)):
            raise ValueError("!any(is.na(labels)) is not TRUE")
    if sp.issparse(data) and data.format == "csc":
        # a dgCMatrix's own slots: R/fm_matrix.R:26-33 transposes on the host (Matrix::t); the slots go over as they are and the device transposes
        # (fmx_matrix_from_dgc; examples/FM_glue.cpp takes the same branch on the "col_ptr" element)
        n, p = data.shape
        if labels is not None and len(labels) != n:
            raise ValueError("length(labels) == nrow(data) is not TRUE")
        if feature_names is None:
            feature_names = [f"V{j + 1}" for j in range(p)]
        elif len(feature_names) != p:
            raise ValueError("ncol(data) == length(feature_names) is not TRUE")
        if data.nnz > np.iinfo(np.int32).max or n > np.iinfo(np.int32).max:
            raise ValueError("a dgCMatrix's slots are 32-bit: more stored entries or rows than 2^31 - 1 (pass the rows as CSR instead)")   # (astype would wrap silently)
        features = {"value": data.data.astype(np.float64), "col_idx": data.indices.astype(np.int32), "col_ptr": data.indptr.astype(np.int32),
                    "dim": (n, p), "size": int(data.nnz)}
        return FmMatrix(features, labels, list(feature_names))
    X = data.tocsr() if sp.issparse(data) else sp.csr_matrix(np.asarray(data, np.float64))
    X.sort_indices()
    n, p = X.shape
    if labels is not None and len(labels) != n:
        raise ValueError("length(labels) == nrow(data) is not TRUE")
    if feature_names is None:
        feature_names = [f"V{j + 1}" for j in range(p)]  # numpy has no colnames; R would stop("there's no feature_names")
    elif len(feature_names) != p:
        raise ValueError("ncol(data) == length(feature_names) is not TRUE")
    if p > np.iinfo(np.int32).max:
        raise ValueError("fm.matrix keeps col_idx as 32-bit integers: more columns than 2^31 - 1")   # (astype would wrap silently)
    features = {"value": X.data.astype(np.float64), "col_idx": X.indices.astype(np.int32),
                "row_size": np.diff(X.indptr).astype(np.int32), "dim": (n, p), "size": int(X.nnz)}
    return FmMatrix(features, labels, list(feature_names))


def _device_matrix(data, labels, device):
    f = data.features
    if "col_ptr" in f:
        return Matrix.from_dgc(f["value"], f["col_idx"], f["col_ptr"], f["dim"][0], f["dim"][1], labels, device=device)
    return Matrix.from_rlist(f["value"], f["col_idx"], f["row_size"], f["dim"][1], labels, device=device)


def _engine_for(controls, p, target_range, mode, batch_rows, device):
    model, solver_ctl = controls["model"], controls["solver"]
    hp, sol = model["hyper.params"], solver_ctl["solver"]
    if model["task"] == "RANK" and mode in ("sequential", "sequential_bitwise"):
        mode, batch_rows = "minibatch_fp64", 2  # scoring a RANK model (predict, fm_recommend, fm_explain): the fp64 tables of the sequential engine
    return Engine(p, task=_TASKS[model["task"]], solver=_SOLVERS[sol["solver"]], num_factor=int(hp["factor.number"]),
                  keep_w0=int(hp["keep.w0"]), keep_w1=int(hp["keep.w1"]), l2_w0=hp["L2.w0"], l1_w1=hp["L1.w1"], l2_w1=hp["L2.w1"],
                  l1_v=hp["L1.v"], l2_v=hp["L2.v"], learn_rate=sol.get("learn_rate", 0.01), alpha_w=sol.get("alpha_w", 0.1),
                  alpha_v=sol.get("alpha_v", 0.1), beta_w=sol.get("beta_w", 1.0), beta_v=sol.get("beta_v", 1.0),
                  gamma=sol.get("gamma", 1e-4), random_step=int(sol.get("random_step", 1)), mode=L.MODE_SEQUENTIAL if mode in ("sequential", "sequential_bitwise") else L.MODE_MINIBATCH,
                  seq_reassociate=int(mode == "sequential"), state_fp64=int(mode == "minibatch_fp64"), batch_rows=int(batch_rows), min_target=target_range[0], max_target=target_range[1], device=device)


def _merge_controls(data, control):
    n = data.dim[0]
    merged = {"model": model_control(), "solver": solver_control(max_iter=max(10000, 2 * n)), "track": track_control()}  # R/fm_train.R:90-93
    for c in (control or []):
        cls = c.get("class", "")
        if not cls.endswith(".control"):
            raise ValueError("control list is wrong")
        merged[cls.split(".")[0]] = c
    merged["track"]["max_iter"] = merged["solver"]["max_iter"]  # R/fm_train.R:106
    return merged


def _check_labels(data, task):
    if data.labels is None:
        raise ValueError("there are no labels in data")  # R/fm_train.R:72-74
    y = np.asarray(data.labels, np.float64)
    if task == "CLASSIFICATION":  # R/fm_train.R:112-122
        u = np.unique(y)
        if len(u) != 2:
            raise ValueError("target should have two levels")
        if np.array_equal(u, [0.0, 1.0]):
            y = np.where(y < 1, -1.0, 1.0)
        elif not np.array_equal(u, [-1.0, 1.0]):
            raise ValueError("target should be c(0, 1) or c(-1, 1)")
    return y


def _normalize_columns(normalize, p):
    """R/fm_train.R:75-87: TRUE -> every column, FALSE -> none, or an integer vector of columns (0-based here, R is 1-based)."""
    if isinstance(normalize, (bool, np.bool_)):
        return np.arange(p, dtype=np.int32) if normalize else None
    cols = np.asarray(normalize)
    if cols.dtype.kind not in "iu":
        raise TypeError("normalize should be a logical value or an integer vector")
    if cols.size and (cols.min() < 0 or cols.max() >= p):
        raise ValueError("the columns to be normalized is out of range")
    return np.sort(cols).astype(np.int32)


def _mcmc_draws(rng, n, p, iters, k0, k1):
    """Standard variates of one MCMC run in the reference's call order: per iteration the Gamma of update_alpha, the
    normal of update_w0, the Gamma of update_w_lambda, the normals of update_w_mu and update_w (fmx.h: fmx_mcmc_train)."""
    g = np.ones((iters, 2)); z = np.zeros((iters, 2 + p))
    for it in range(iters):
        g[it, 0] = rng.gamma((1.0 + n) / 2.0)
        if k0:
            z[it, 0] = rng.normal()
        if k1:
            g[it, 1] = rng.gamma((2.0 + p) / 2.0)
            z[it, 1] = rng.normal()
            z[it, 2:] = rng.normal(size=p)
    return g, z


def _train(data, controls, w0, w, v, target_range, mode, batch_rows, device, norm_cols=None, rng=None):
    p = data.dim[1]
    y = _check_labels(data, controls["model"]["task"])
    lo, hi = float(y.min()), float(y.max())  # src/FM.cpp:89-90
    if target_range is not None:               # src/FM.cpp:91-96 (fm.update widens the range)
        lo, hi = min(lo, target_range[0]), max(hi, target_range[1])
    if controls["solver"]["solver"]["solver"] in ("ALS", "MCMC"):
        mode = "sequential"  # ALS / MCMC work on the fp64 tables
    eng = _engine_for(controls, p, (lo, hi), mode, batch_rows, device)
    eng.set_params(w0, w, v)
    m = _device_matrix(data, y, device)
    mean = std = None
    if norm_cols is not None:  # src/FM.cpp:36-38: scales = m.scales(normalize)
        mean, std = m.scales(norm_cols)
    sol = controls["solver"]["solver"]["solver"]
    track = controls["track"]
    trace, convergent = None, False
    if sol == "MCMC":
        hp = controls["model"]["hyper.params"]
        iters = int(controls["solver"]["max_iter"])
        g, z = _mcmc_draws(rng if rng is not None else np.random.default_rng(), data.dim[0], p, iters, bool(hp["keep.w0"]), bool(hp["keep.w1"]))
        if track["step_size"] > 0 and iters > 0:
            # the tracker block of MCMC_ALS_Learner::learn (:96-125): the model at the START of iterations 0, step, 2 step, ... and of
            # the last one is scored (clamped predictions / fast_pnorm) and snapshotted; the chain continues call by call
            metric = getattr(L, "EVAL_" + track["evaluate.metric"])
            idx, evals, snaps, state, ii = [], [], [], None, -1
            for it in range(iters):
                ii = 0 if ii + 1 == track["step_size"] else ii + 1
                if ii == 0 or it == iters - 1:
                    idx.append(it); evals.append(eng.evaluate(m, metric))
                    a, b, c = eng.get_params(); snaps.append({"w0": a, "w": b, "v": c})
                state = eng.mcmc_train(m, 1, g[it:it + 1], z[it:it + 1]) if state is None else eng.mcmc_train_from(m, 1, g[it:it + 1], z[it:it + 1], state)
            trace = {"trace": [np.asarray(idx)] + snaps, "evaluation.train": np.asarray(evals)}
        else:
            eng.mcmc_train(m, iters, g, z)
    elif track["step_size"] > 0:  # learner->tracker.step_size > 0: Learner::learn evaluates, snapshots and may stop early
        metric = getattr(L, "EVAL_" + track["evaluate.metric"])
        r = eng.train_tracked(m, controls["solver"]["max_iter"], track["step_size"], metric, track["convergence"], keep_params=True)
        convergent = r["convergent"]
        # Tracker::save (core/Tracker.h:96-119): trace = list(record_index, {w0,w,v}...), evaluation.train
        trace = {"trace": [r["iters"]] + [{"w0": a, "w": b, "v": c} for (a, b, c) in r["params"]], "evaluation.train": r["evals"]}
    elif sol == "ALS":  # MCMC_ALS_Learner::learn; as shipped it never sweeps V (SURVEY A-1) unless als_update_v is asked for
        eng.als_train(m, controls["solver"]["max_iter"], with_v=bool(controls["solver"]["solver"].get("update_v", False)))
    else:
        eng.train(m, controls["solver"]["max_iter"])
    w0, w, v = eng.get_params()
    model = {"w0": w0, "w": w, "v": v, "model.control": controls["model"], "solver.control": controls["solver"],
             "track.control": controls["track"], "convergence": convergent}
    scales = {"mean": mean, "std": std, "model.vars": data.feature_names, "target.range": (lo, hi)}
    fit = {"class": "FM", "Model": model, "Scales": scales, "engine": {"mode": mode, "batch_rows": batch_rows, "device": device}}
    if trace is not None:
        fit["Trace"] = trace
    return fit


def fm_train(data, normalize=True, control=None, seed=None, mode="sequential", batch_rows=65536, device=0):
    """fm.train() -- R/fm_train.R:70-127.  `control` is a list of *.control objects.  V0 ~ N(v.init_mean, v.init_stdev)
    is drawn here (the reference draws it from R's RNG inside Model::init, core/Model.h:63-72); `seed` makes it repeatable.
    mode="sequential" is the reference's algorithm (its visiting order, one update per example, fp64; for SGD the forward's sum is reassociated so that only
    w0 chains the examples -- cfg.seq_reassociate: <= 1e-10 on V against the CPU restatement, 4.0 M examples/s); mode="sequential_bitwise" keeps the reference's association
    (<= 1e-11, 1.65 M examples/s); mode="minibatch" the synchronous mini-batch engine (fp32 state),
    mode="minibatch_fp64" the same engine on fp64 state."""
    if not isinstance(data, FmMatrix):
        raise TypeError("data must be a fm.matrix object")
    norm_cols = _normalize_columns(normalize, data.dim[1])
    controls = _merge_controls(data, control)
    if controls["model"]["task"] == "RANK":
        raise ValueError("task RANK trains on sampled preference pairs: use fm_train_rank(context, items, positives, control)")
    hp = controls["model"]["hyper.params"]
    k, p = int(hp["factor.number"]), data.dim[1]
    rng = np.random.default_rng(seed)
    v0 = rng.normal(hp["v.init_mean"], hp["v.init_stdev"], (k, p)) if k > 0 else np.zeros((0, p))
    return _train(data, controls, 0.0, np.zeros(p), v0, None, mode, batch_rows, device, norm_cols, rng=rng)


def fm_update(object, data, normalize=True, max_iter=None, mode=None, batch_rows=None, device=None, rng=None):
    """fm.update() -- R/fm_update.R:18-135: continue training from a fitted FM with the controls stored on it.
    Optimizer state (FTRL z/n, SGD q/u) is NOT carried over, exactly as in the reference.
    rng: a numpy Generator standing in for R's global stream.  The reference calls fm.init() -- k*p normal draws -- BEFORE the
    warm start overwrites them (src/FM.cpp:64 precedes :66-72), so an update consumes k*p normals too: they are drawn from
    `rng` and discarded here, which leaves the stream where the reference leaves it (examples/FM_glue.cpp does the same in R)."""
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    if not isinstance(data, FmMatrix):
        raise TypeError("data must be a fm.matrix object")
    if list(data.feature_names) != list(object["Scales"]["model.vars"]):  # R/fm_update.R:27-37
        raise ValueError("the features in data are not the same as those in FM model")
    mdl = object["Model"]
    if mdl["model.control"]["task"] == "RANK":
        raise ValueError("fm_update does not continue a RANK model (it trains pointwise on labels): train a new one with fm_train_rank, or pass the model's "
                         "parameters as the start of your own pairwise loop")
    # normalisation settings, R/fm_update.R:39-83 (its interactive readline() branches become errors here)
    p = data.dim[1]
    sc = object["Scales"]
    model_normalized = sc["mean"] is not None
    model_cols = np.where((np.asarray(sc["mean"]) != 0) | (np.asarray(sc["std"]) != 1))[0].astype(np.int32) if model_normalized else None
    if isinstance(normalize, (bool, np.bool_)):
        if normalize:
            if not model_normalized:
                raise ValueError("all the features are not normalized in the previously saved model; pass normalize=False or the columns explicitly")
            norm_cols = model_cols  # "follow the normalization settings in the previously saved model"
        else:
            if model_normalized:
                warnings.warn("some features have been normalized in previously saved model, but those in data will not")
            norm_cols = None
    else:
        norm_cols = _normalize_columns(normalize, p)
        if model_normalized and not np.array_equal(model_cols, norm_cols):
            raise ValueError("the selected features to normalize are different from those in previously saved model")
    controls = {"model": mdl["model.control"], "solver": dict(mdl["solver.control"]), "track": mdl["track.control"]}
    controls["solver"]["max_iter"] = max(10000, 2 * data.dim[0])  # R/fm_update.R:90
    if max_iter is not None:
        controls["solver"]["max_iter"] = int(max_iter)
    eng = object.get("engine", {})
    if rng is not None:
        hp = controls["model"]["hyper.params"]
        rng.normal(hp["v.init_mean"], hp["v.init_stdev"], (int(hp["factor.number"]), p))   # Model::init's draws, discarded (src/FM.cpp:64)
    fit = _train(data, controls, mdl["w0"], mdl["w"], mdl["v"], object["Scales"]["target.range"],
                 mode or eng.get("mode", "sequential"), batch_rows or eng.get("batch_rows", 65536),
                 eng.get("device", 0) if device is None else device, norm_cols, **({"rng": rng} if rng is not None else {}))
    if object.get("Trace") is not None and fit.get("Trace") is not None:  # R/fm_update.R:125-133: traces are concatenated
        old, new = object["Trace"], fit["Trace"]
        idx = np.concatenate([np.asarray(old["trace"][0]), np.asarray(new["trace"][0]) + np.asarray(old["trace"][0])[-1]])
        fit["Trace"] = {"trace": [idx] + list(old["trace"][1:]) + list(new["trace"][1:]),
                        "evaluation.train": np.concatenate([old["evaluation.train"], new["evaluation.train"]])}
    return fit


def predict(object, newdata=None, normalize=True):
    """predict.FM() -- R/fm_predict.R:12-34 -> FMPredict (src/FM.cpp:177-214): probabilities for CLASSIFICATION
    (logistic link for SGD/FTRL/TDAP models, the probit table for ALS models), predictions clamped to the training target range for REGRESSION."""
    if newdata is None:
        raise ValueError("newdata is null")
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata must be a fm.matrix object")
    if np.any(np.isnan(newdata.features["value"])):
        raise ValueError("there are NAs in newdata")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    mdl = object["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, newdata.dim[1], object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    m = _device_matrix(newdata, None, device)
    if normalize:  # src/FM.cpp:183-186: m.normalize(scales)
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    if controls["model"]["task"] == "RANK":
        link = L.LINK_NONE  # a ranking model's scores order items; they are not probabilities
    elif controls["model"]["task"] != "CLASSIFICATION":
        link = L.LINK_CLAMP
    else:  # Model::predict_prob, core/Model.h:163-180: probit table for MCMC / ALS models, logistic otherwise
        link = L.LINK_PROBIT if controls["solver"]["solver"]["solver"] in ("MCMC", "ALS") else L.LINK_LOGISTIC
    return eng.predict(m, link)


def _exclude_csr(exclude, n_ctx, n_items, name="exclude"):
    """fm_recommend's `exclude` (or another id list, called `name` in the messages) as CSR arrays (row_ptr, col): a scipy sparse matrix
    n_ctx x n_items (stored entries = excluded items) or a list of n_ctx arrays of 0-based item indices."""
    import scipy.sparse as sp
    if sp.issparse(exclude):
        X = exclude.tocsr()
        if X.shape != (n_ctx, n_items):
            raise ValueError(f"{name} must be {n_ctx} x {n_items} (got {X.shape[0]} x {X.shape[1]})")
        return X.indptr.astype(np.int64), X.indices.astype(np.int64)
    rows = list(exclude)
    if len(rows) != n_ctx:
        raise ValueError(f"{name} must hold one index array per row of newdata ({n_ctx}), got {len(rows)}")
    rows = [np.asarray(r, np.int64).ravel() for r in rows]
    col = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if col.size and (col.min() < 0 or col.max() >= n_items):
        raise ValueError(f"{name} holds item indices outside 0..{n_items - 1}")
    return np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), col


def fm_recommend(object, newdata, items, top_k=10, exclude=None, normalize=True):
    """The top_k rows of `items` for every row of `newdata` under the model's score of the concatenated row (context entries followed by
    item entries), on predict()'s scale: probabilities for CLASSIFICATION (logistic, or the probit table of ALS / MCMC models), the training
    target range's clamp for REGRESSION.  The ranking is on the raw score (higher first, ties by the lower item index); exclude: a scipy
    sparse matrix (rows of newdata x rows of items) or a list of index arrays naming items a context must not receive.
    Returns {"index": int64[n, top_k] (0-based, -1 where a context has fewer eligible items), "score": float64[n, top_k] (NaN there)}."""
    for name, d in (("newdata", newdata), ("items", items)):
        if not isinstance(d, FmMatrix):
            raise TypeError(f"{name} must be a fm.matrix object")
        if np.any(np.isnan(d.features["value"])):
            raise ValueError(f"there are NAs in {name}")
    if isinstance(top_k, (bool, np.bool_)) or int(top_k) != top_k:
        raise ValueError("top_k must be an integer")
    top_k = int(top_k)
    if not 1 <= top_k <= 1024:
        raise ValueError(f"top_k must be in 1..1024 (got {top_k})")
    mdl = object["Model"]
    p = len(mdl["w"])
    if newdata.dim[1] != p or items.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}, items {items.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    n_ctx, n_items = newdata.dim[0], items.dim[0]
    excl = None if exclude is None else _exclude_csr(exclude, n_ctx, n_items)
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    mc, mi = _device_matrix(newdata, None, device), _device_matrix(items, None, device)
    if normalize:
        mc.normalize(object["Scales"]["mean"], object["Scales"]["std"])
        mi.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    mx = None
    if excl is not None:
        rp, col = excl
        mx = Matrix.from_csr(rp, col.astype(np.uint32), np.ones(len(col), np.float32), n_items, device=device)
    if controls["model"]["task"] == "RANK":
        link = L.LINK_NONE
    elif controls["model"]["task"] != "CLASSIFICATION":
        link = L.LINK_CLAMP
    else:
        link = L.LINK_PROBIT if controls["solver"]["solver"]["solver"] in ("MCMC", "ALS") else L.LINK_LOGISTIC
    index, score = eng.topk(mc, mi, top_k, exclude=mx, link=link)
    return {"index": index, "score": score}


def fm_recommend_metrics(object, newdata, items, heldout, k=10, exclude=None, normalize=True, per_context=False, ranks=False):
    """Full-ranking quality of the model's recommendations on held-out items (include/fmx.h: fmx_heldout_metrics).

    For every row c of `newdata`, every row of `items` not named in exclude's row c is ranked by the model's raw score of the concatenated
    row, as fm_recommend ranks it (higher first, ties by the lower item index, NaN last); rank(c, h) is the 0-based position of held-out
    item h among them, so h is in fm_recommend(top_k = K, exclude = exclude)'s list iff rank < K.  heldout and exclude: scipy sparse matrices
    (rows of newdata x rows of items; stored entries name items) or lists of index arrays, one per row of newdata; duplicates count once, and
    an item both held out and excluded for one context is an error.  k: an int or a sequence of ints >= 1 (up to 32).

    Returns {"precision@K", "recall@K", "ndcg@K", "hit@K" for every K, "mrr", "auc", "n_contexts", "n_auc_contexts"}: means over the contexts
    with at least one held-out item (auc over those with at least one eligible item that is not held out).  auc is the share of
    (held-out, other eligible) pairs ordered correctly, ties split by item index.  per_context=True adds "per_context": {name: float64[n]}
    (NaN for a context without held-out items); ranks=True adds "rank": a scipy.sparse.csr_matrix with heldout's pattern holding each entry's rank."""
    import scipy.sparse as sp
    for name, d in (("newdata", newdata), ("items", items)):
        if not isinstance(d, FmMatrix):
            raise TypeError(f"{name} must be a fm.matrix object")
        if np.any(np.isnan(d.features["value"])):
            raise ValueError(f"there are NAs in {name}")
    ks = [k] if np.isscalar(k) else list(k)
    if not ks or len(ks) > 32:
        raise ValueError(f"k must hold 1..32 cut-offs (got {len(ks)})")
    for K in ks:
        if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or int(K) < 1 or int(K) >= 2**31:
            raise ValueError(f"every k must be an integer >= 1 (got {K!r})")
    ks = [int(K) for K in ks]
    mdl = object["Model"]
    p = len(mdl["w"])
    if newdata.dim[1] != p or items.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}, items {items.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    n_ctx, n_items = newdata.dim[0], items.dim[0]
    if heldout is None:
        raise TypeError("heldout must be a scipy sparse matrix or a list of index arrays")
    try:
        hrp, hcol = _exclude_csr(heldout, n_ctx, n_items)
    except ValueError as err:
        raise ValueError(str(err).replace("exclude", "heldout")) from None
    if hcol.size and (hcol.min() < 0 or hcol.max() >= n_items):
        raise ValueError(f"heldout holds item indices outside 0..{n_items - 1}")
    if hcol.size == 0:
        raise ValueError("heldout holds no item: there is nothing to rank")
    excl = None if exclude is None else _exclude_csr(exclude, n_ctx, n_items)
    if excl is not None and excl[1].size:
        hrow = np.repeat(np.arange(n_ctx, dtype=np.int64), np.diff(hrp))
        xrow = np.repeat(np.arange(n_ctx, dtype=np.int64), np.diff(excl[0]))
        both = np.intersect1d(hrow * n_items + hcol, xrow * n_items + excl[1])
        if both.size:
            raise ValueError(f"context {int(both[0] // n_items)} holds item {int(both[0] % n_items)} both in heldout and in exclude")
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    mc, mi = _device_matrix(newdata, None, device), _device_matrix(items, None, device)
    if normalize:
        mc.normalize(object["Scales"]["mean"], object["Scales"]["std"])
        mi.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    mh = Matrix.from_csr(hrp, hcol.astype(np.uint32), np.ones(len(hcol), np.float32), n_items, device=device)
    mx = None
    if excl is not None:
        mx = Matrix.from_csr(excl[0], excl[1].astype(np.uint32), np.ones(len(excl[1]), np.float32), n_items, device=device)
    res = eng.heldout_metrics(mc, mi, mh, ks, exclude=mx, per_context=per_context)
    names = [f"{m}@{K}" for K in ks for m in ("precision", "recall", "ndcg", "hit")] + ["mrr", "auc"]
    out = {name: float(v) for name, v in zip(names, res["mean"])}
    out["n_contexts"], out["n_auc_contexts"] = res["counted"]
    if per_context:
        out["per_context"] = {name: res["per_context"][:, q].copy() for q, name in enumerate(names)}
    if ranks:
        rank, _ = eng.heldout_rank(mc, mi, mh, exclude=mx)
        out["rank"] = sp.csr_matrix((rank, hcol, hrp), shape=(n_ctx, n_items))
    return out


def _recommend_inputs(object, newdata, items, normalize):
    """the host-side checks fm_recommend runs on its model and matrices; returns the model's feature count"""
    for name, d in (("newdata", newdata), ("items", items)):
        if d is None:
            continue
        if not isinstance(d, FmMatrix):
            raise TypeError(f"{name} must be a fm.matrix object")
        if np.any(np.isnan(d.features["value"])):
            raise ValueError(f"there are NAs in {name}")
    p = len(object["Model"]["w"])
    if newdata.dim[1] != p or (items is not None and items.dim[1] != p):
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}" +
                         ("" if items is None else f", items {items.dim[1]}"))
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    return p


def _recommend_engine(object, p, normalize, *data):
    """the engine holding the model, and the device matrices of `data` (normalised as the model was)"""
    mdl = object["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    mats = [_device_matrix(d, None, device) for d in data]
    if normalize:
        for m in mats:
            m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    if controls["model"]["task"] == "RANK":
        link = L.LINK_NONE
    elif controls["model"]["task"] != "CLASSIFICATION":
        link = L.LINK_CLAMP
    else:
        link = L.LINK_PROBIT if controls["solver"]["solver"]["solver"] in ("MCMC", "ALS") else L.LINK_LOGISTIC
    return eng, mats, link, device


def fm_rerank(object, newdata, items, candidates, top_k=None, normalize=True):
    """Scores and orders, for every row of `newdata`, the candidate rows of `items` that `candidates` names for it -- the ranking stage behind a
    retrieval step, or sampled evaluation -- with work proportional to the lists, not to the item count (include/fmx.h: fmx_rank_lists,
    DESIGN.md section 17).  candidates: a scipy sparse matrix (rows of newdata x rows of items; stored entries name items) or a list of index
    arrays, one per row of newdata; any order, duplicates allowed, empty lists allowed.  Scores are on predict()'s scale, as fm_recommend's;
    the order is fm_recommend's (the raw score, higher first, ties by the lower item index, NaN last).

    top_k=None returns {"score": csr_matrix, "position": csr_matrix} with candidates' pattern, entry for entry (duplicates and explicit zeros
    kept): the score of the pair and the 0-based position of the item among the list's distinct candidates.  top_k=K (1..1024) returns
    fm_recommend's {"index": int64[n, K] (-1 beyond a list's distinct candidates), "score": float64[n, K] (NaN there)}."""
    import scipy.sparse as sp
    p = _recommend_inputs(object, newdata, items, normalize)
    if top_k is not None:
        if isinstance(top_k, (bool, np.bool_)) or int(top_k) != top_k:
            raise ValueError("top_k must be an integer")
        top_k = int(top_k)
        if not 1 <= top_k <= 1024:
            raise ValueError(f"top_k must be in 1..1024 (got {top_k})")
    n_ctx, n_items = newdata.dim[0], items.dim[0]
    if candidates is None:
        raise TypeError("candidates must be a scipy sparse matrix or a list of index arrays")
    rp, col = _exclude_csr(candidates, n_ctx, n_items, name="candidates")
    eng, (mc, mi), link, device = _recommend_engine(object, p, normalize, newdata, items)
    ml = Matrix.from_csr(rp, col.astype(np.uint32), np.ones(len(col), np.float32), n_items, device=device)
    if top_k is not None:
        index, score = eng.topk_lists(mc, mi, ml, top_k, link=link)
        return {"index": index, "score": score}
    score, pos = eng.rank_lists(mc, mi, ml, link=link)
    return {"score": sp.csr_matrix((score, col, rp), shape=(n_ctx, n_items)), "position": sp.csr_matrix((pos, col, rp), shape=(n_ctx, n_items))}


def fm_diversify(object, newdata, items, top_k=10, trade_off=0.7, pool=None, candidates=None, exclude=None, relevance="minmax", normalize=True):
    """Diversified recommendations: for every row of `newdata`, top_k of its `pool` best-scored rows of `items`, picked one at a time by greedy
    maximal marginal relevance (include/fmx.h: fmx_diversify).  Each step takes the candidate with the largest
    trade_off * relevance - (1 - trade_off) * (its largest cosine similarity to an item picked before), the similarity being the cosine of the
    items' factor sums (fm_embed's "s").  trade_off = 1 is the ranking by score alone, 0 the most spread-out picks.

    The pool: with `candidates` (as fm_rerank's) the pool best of every row's list; otherwise the pool best of all items, `exclude` (as
    fm_recommend's) left out.  pool=None means min(1024, number of items, max(100, 10 * top_k)).  Scores are on predict()'s scale, as
    fm_recommend's.  relevance: "minmax" rescales a row's pool scores to [0, 1] so that trade_off means the same for every model; "score" takes
    the score as it is (a link that saturates can tie scores the raw ranking tells apart: such ties go to the lower item index).

    Returns {"index": int64[n, top_k] in the order picked (-1 beyond a pool's candidates), "score": float64[n, top_k] (the items' scores, NaN
    there), "margin": float64[n, top_k] (what each pick scored at its step)}."""
    p = _recommend_inputs(object, newdata, items, normalize)
    if isinstance(top_k, (bool, np.bool_)) or int(top_k) != top_k:
        raise ValueError("top_k must be an integer")
    top_k = int(top_k)
    if not 1 <= top_k <= 1024:
        raise ValueError(f"top_k must be in 1..1024 (got {top_k})")
    if candidates is not None and exclude is not None:
        raise ValueError("candidates and exclude can not be given together: leave the excluded items out of the candidates")
    if relevance not in ("minmax", "score"):
        raise ValueError(f"relevance must be 'minmax' or 'score' (got {relevance!r})")
    trade_off = float(trade_off)
    if not 0.0 <= trade_off <= 1.0:
        raise ValueError(f"trade_off must be in [0, 1] (got {trade_off})")
    n_ctx, n_items = newdata.dim[0], items.dim[0]
    if pool is None:
        pool = min(1024, n_items, max(100, 10 * top_k))
    if isinstance(pool, (bool, np.bool_)) or int(pool) != pool:
        raise ValueError("pool must be an integer")
    pool = int(pool)
    if not top_k <= pool <= 1024:
        raise ValueError(f"pool must be in top_k..1024 (got pool {pool}, top_k {top_k})")
    lists = None if candidates is None else _exclude_csr(candidates, n_ctx, n_items, name="candidates")
    excl = None if exclude is None else _exclude_csr(exclude, n_ctx, n_items)
    eng, (mc, mi), link, device = _recommend_engine(object, p, normalize, newdata, items)
    if lists is not None:
        ml = Matrix.from_csr(lists[0], lists[1].astype(np.uint32), np.ones(len(lists[1]), np.float32), n_items, device=device)
        index, score = eng.topk_lists(mc, mi, ml, pool, link=link)
    else:
        mx = None
        if excl is not None:
            mx = Matrix.from_csr(excl[0], excl[1].astype(np.uint32), np.ones(len(excl[1]), np.float32), n_items, device=device)
        index, score = eng.topk(mc, mi, pool, exclude=mx, link=link)
    rel = L.DIV_REL_MINMAX if relevance == "minmax" else L.DIV_REL_SCORE
    index, score, margin = eng.diversify(mi, index, score, top_k, trade_off, rel)
    return {"index": index, "score": score, "margin": margin}


def fm_similar(object, items, queries=None, top_k=10, metric="cosine", normalize=True):
    """"More like this": for every row of `queries`, the top_k rows of `items` whose factor sums (fm_embed's "s") point the same way (include/fmx.h:
    fmx_neighbors).  metric "cosine" is the cosine of the two factor sums -- fm_diversify's similarity, bit for bit -- and
    "dot" their dot product; biases and linear weights play no part.  queries=None means the items against themselves, a row never being its own
    neighbour.  The order is fm_recommend's (a higher score first, ties by the lower item index, NaN last).

    Returns {"index": int64[n, top_k] (-1 where there are fewer items), "score": float64[n, top_k] (NaN there)}."""
    if metric not in ("cosine", "dot"):
        raise ValueError(f"metric must be 'cosine' or 'dot' (got {metric!r})")
    if isinstance(top_k, (bool, np.bool_)) or int(top_k) != top_k:
        raise ValueError("top_k must be an integer")
    top_k = int(top_k)
    if not 1 <= top_k <= 1024:
        raise ValueError(f"top_k must be in 1..1024 (got {top_k})")
    sim = L.SIM_COSINE if metric == "cosine" else L.SIM_DOT
    if queries is None:
        p = _recommend_inputs(object, items, None, normalize)
        eng, (mi,), _, _ = _recommend_engine(object, p, normalize, items)
        index, score = eng.neighbors(mi, mi, top_k, metric=sim, skip_self=True)
    else:
        p = _recommend_inputs(object, queries, items, normalize)
        eng, (mq, mi), _, _ = _recommend_engine(object, p, normalize, queries, items)
        index, score = eng.neighbors(mq, mi, top_k, metric=sim)
    return {"index": index, "score": score}


INDEX_MAX_LISTS, INDEX_MAX_ITER = 65536, 100   # include/fmx.h: FMX_INDEX_MAX_LISTS, FMX_INDEX_MAX_ITER


def _index_int(name, value, lo, hi):
    if isinstance(value, (bool, np.bool_)) or int(value) != value:
        raise ValueError(f"{name} must be an integer")
    value = int(value)
    if not lo <= value <= hi:
        raise ValueError(f"{name} must be in {lo}..{hi} (got {value})")
    return value


def fm_index(object, items, n_lists=None, n_iter=10, seed=0, normalize=True):
    """A clustered index over the rows of `items` for fm_recommend_indexed (include/fmx.h: fmx_index_build): a deterministic
    k-means -- n_iter rounds, seeds drawn by `seed` -- over the items' sides of the model's pair score (fm_embed's "s" and "base").  n_lists=None
    takes round(sqrt(rows of items)), clipped to 1..65536.  The index holds no parameters: after the model changes it still serves, at a lower
    recall.  Returns an engine.ItemIndex (.centroids, .assign, .list_ptr, .list_item, .n_lists, .non_empty)."""
    p = _recommend_inputs(object, items, None, normalize)
    n_items = items.dim[0]
    if n_items < 1:
        raise ValueError("items holds no rows")
    if n_lists is None:
        n_lists = min(max(int(round(np.sqrt(n_items))), 1), INDEX_MAX_LISTS, n_items)
    n_lists = _index_int("n_lists", n_lists, 1, min(INDEX_MAX_LISTS, n_items))
    n_iter = _index_int("n_iter", n_iter, 0, INDEX_MAX_ITER)
    seed = _index_int("seed", seed, 0, 2 ** 64 - 1)
    eng, (mi,), _, _ = _recommend_engine(object, p, normalize, items)
    return eng.index_build(mi, n_lists, n_iter=n_iter, seed=seed)


def _indexed_args(index, items, top_k, n_probes):
    from .engine import ItemIndex
    if not isinstance(index, ItemIndex):
        raise TypeError("index must be the object fm_index returned")
    top_k = _index_int("top_k", top_k, 1, 1024)
    if isinstance(items, FmMatrix) and items.dim[0] != index.n_items:
        raise ValueError(f"the index holds {index.n_items} items, items has {items.dim[0]} rows")
    return top_k, [_index_int("n_probe", q, 1, index.n_lists) for q in n_probes]


def fm_recommend_indexed(object, index, newdata, items, top_k=10, n_probe=8, exclude=None, normalize=True):
    """fm_recommend over the items of the n_probe lists of `index` (fm_index's result) closest to each row of `newdata` instead of over every row
    of `items` (include/fmx.h: fmx_topk_index).  A returned item's score is fm_recommend's, bit for bit, and so is the order; what may differ
    is which items are looked at -- fm_index_recall measures it.  n_probe >= index.non_empty is fm_recommend itself.
    Returns fm_recommend's {"index", "score"} and "scanned": int64[n], the number of items in each row's probed lists."""
    top_k, (n_probe,) = _indexed_args(index, items, top_k, [n_probe])
    p = _recommend_inputs(object, newdata, items, normalize)
    n_ctx, n_items = newdata.dim[0], items.dim[0]
    excl = None if exclude is None else _exclude_csr(exclude, n_ctx, n_items)
    eng, (mc, mi), link, device = _recommend_engine(object, p, normalize, newdata, items)
    mx = None
    if excl is not None:
        rp, col = excl
        mx = Matrix.from_csr(rp, col.astype(np.uint32), np.ones(len(col), np.float32), n_items, device=device)
    idx, score, scanned = eng.topk_index(index, mc, mi, top_k, n_probe, exclude=mx, link=link)
    return {"index": idx, "score": score, "scanned": scanned}


def fm_index_recall(object, index, newdata, items, top_k, n_probes, normalize=True):
    """The tool for choosing n_probe: for every value of `n_probes`, the mean share of fm_recommend's top_k (the exact, exhaustive ranking) that
    fm_recommend_indexed returns, and the mean number of scanned items.  Returns {"n_probe": int64[m], "recall": float64[m], "scanned":
    float64[m]}; a row without eligible items counts as fully recalled."""
    n_probes = list(np.atleast_1d(n_probes))
    top_k, n_probes = _indexed_args(index, items, top_k, n_probes)
    p = _recommend_inputs(object, newdata, items, normalize)
    eng, (mc, mi), link, _ = _recommend_engine(object, p, normalize, newdata, items)
    full, _ = eng.topk(mc, mi, top_k, link=link)
    recall, scanned = np.zeros(len(n_probes)), np.zeros(len(n_probes))
    for t, q in enumerate(n_probes):
        got, _, sc = eng.topk_index(index, mc, mi, top_k, q, link=link)
        share = [1.0 if not (f >= 0).any() else np.isin(f[f >= 0], g[g >= 0]).mean() for f, g in zip(full, got)]
        recall[t] = float(np.mean(share)) if len(share) else 1.0
        scanned[t] = float(np.mean(sc)) if len(sc) else 0.0
    return {"n_probe": np.asarray(n_probes, np.int64), "recall": recall, "scanned": scanned}


def fm_embed(object, data, normalize=True, with_w0=False):
    """The two sides of the model's pair score for every row of `data` (include/fmx.h: fmx_project): {"base": float64[n] -- the row's own raw
    prediction, the global bias added only with with_w0 -- and "s": float64[n, k] -- its factor sums}.  For a context row c (with_w0=True) and an
    item row i (with_w0=False) the raw score fm_recommend ranks by is base_c + base_i + <s_c, s_i> (bit for bit with the dot product taken as
    one fma chain in the model's state type), so "s" is what a nearest-neighbour index or an item-item similarity needs."""
    p = _recommend_inputs(object, data, None, normalize)
    eng, (m,), _, _ = _recommend_engine(object, p, normalize, data)
    base, s = eng.project(m, with_w0=bool(with_w0))
    return {"base": base, "s": s}


def _positives_csr(positives, n_ctx, n_items):
    """fm_train_rank's `positives` (a scipy sparse matrix or a list of index arrays, as fm_recommend's exclude) as CSR arrays, checked on the host:
    every context must leave at least one item that is not a positive (duplicates count once)."""
    rp, col = _exclude_csr(positives, n_ctx, n_items)
    if col.size and (col.min() < 0 or col.max() >= n_items):
        raise ValueError(f"positives holds item indices outside 0..{n_items - 1}")
    if col.size:
        row = np.repeat(np.arange(n_ctx, dtype=np.int64), np.diff(rp))
        distinct = np.unique(row * n_items + col) // n_items
        full = np.nonzero(np.bincount(distinct, minlength=n_ctx) >= n_items)[0]
        if full.size:
            raise ValueError(f"context {int(full[0])} has every item as a positive: there is no negative to draw")
    return rp, col


def _rank_inputs(context, items, p=None):
    for name, d in (("context", context), ("items", items)):
        if not isinstance(d, FmMatrix):
            raise TypeError(f"{name} must be a fm.matrix object")
        if np.any(np.isnan(d.features["value"])):
            raise ValueError(f"there are NAs in {name}")
    if context.dim[1] != items.dim[1] or (p is not None and context.dim[1] != p):
        raise ValueError(f"number of input's features is not correct: context {context.dim[1]}, items {items.dim[1]}" + ("" if p is None else f", the model {p}"))


def _rank_pairs(context, items, positives, device):
    """device matrices of context, items and positives (fmx_matrix_pairs' inputs)"""
    rp, col = positives
    mc, mi = _device_matrix(context, None, device), _device_matrix(items, None, device)
    mx = Matrix.from_csr(rp, col.astype(np.uint32), np.ones(len(col), np.float32), items.dim[0], device=device)
    return mc, mi, mx


def fm_train_rank(context, items, positives, control=None, n_neg=1, epochs=10, seed=None, batch_rows=65536, mode="minibatch", device=0,
                  n_candidates=1):
    """Train an FM on implicit feedback with the pairwise BPR loss (task RANK).

    The score of (context c, item i) is the model's raw score of the concatenated row c (+) i -- context entries, then item entries, as
    fm_recommend scores it.  Every epoch samples fresh negatives ON THE DEVICE (fmx_matrix_pairs, epoch = the epoch index): for every distinct
    positive i of every context c, n_neg items j drawn uniformly from the items that are not positives of c, and trains one pass of mini-batch
    SGD or FTRL over the pairs, minimising log(1 + exp(-(y(c (+) i) - y(c (+) j)))).  w0 cancels in every pair and stays 0.
    positives: a scipy sparse matrix (context rows x item rows; stored entries = positives) or a list of index arrays, one per context row.
    control: model.control(task = "RANK", ...) and an SGD or FTRL solver (default SGD.solver()); mode "minibatch" (fp32 state) or
    "minibatch_fp64".  V0 ~ N(v.init_mean, v.init_stdev) is drawn as fm_train draws it; `seed` makes V0 and the samples repeatable.
    n_candidates: 1 (the default) draws every negative uniformly as above.  2..64: dynamic negative sampling -- each
    negative is the best-scored of n_candidates uniform draws under the model as it stands at the start of the epoch (fmx_matrix_pairs_hard;
    the rows, positives and order are the uniform sampler's, candidate 0 is its negative).
    Returns an FM object like fm_train's; its Scales carry no means, so predict / fm_recommend / fm_explain take normalize=False."""
    if isinstance(n_candidates, (bool, np.bool_)) or not isinstance(n_candidates, (int, np.integer)) or not 1 <= int(n_candidates) <= 64:
        raise ValueError(f"n_candidates must be an integer in 1..64 (got {n_candidates!r})")
    n_candidates = int(n_candidates)
    _rank_inputs(context, items)
    n_ctx, n_items, p = context.dim[0], items.dim[0], context.dim[1]
    for name, val, lo in (("n_neg", n_neg, 1), ("epochs", epochs, 0), ("batch_rows", batch_rows, 2)):
        if isinstance(val, (bool, np.bool_)) or int(val) != val or int(val) < lo:
            raise ValueError(f"{name} must be an integer >= {lo} (got {val!r})")
    n_neg, epochs, batch_rows = int(n_neg), int(epochs), int(batch_rows)
    if batch_rows % 2:
        raise ValueError(f"batch_rows must be even: a step may not split a pair (got {batch_rows})")
    if mode not in ("minibatch", "minibatch_fp64"):
        raise ValueError(f"task RANK trains in mode 'minibatch' or 'minibatch_fp64' (got {mode!r})")
    given = {}
    for c in (control or []):
        cls = c.get("class", "") if isinstance(c, dict) else ""
        if not cls.endswith(".control"):
            raise ValueError("control list is wrong")
        given[cls.split(".")[0]] = c
    model = given.get("model", model_control(task="RANK"))
    if model["task"] != "RANK":
        raise ValueError(f"fm_train_rank trains task RANK: the control names task {model['task']}")
    solver = given.get("solver", solver_control(solver=SGD_solver()))
    if solver["solver"]["solver"] not in ("SGD", "FTRL"):
        raise ValueError(f"task RANK trains with the SGD or FTRL solver (got {solver['solver']['solver']})")
    track = given.get("track", track_control())
    if track["step_size"] > 0:
        raise ValueError("the tracker (track.control(step_size > 0)) does not follow RANK training: evaluate with fm_rank_evaluate")
    pos = _positives_csr(positives, n_ctx, n_items)
    controls = {"model": model, "solver": solver, "track": track}
    hp = model["hyper.params"]
    k = int(hp["factor.number"])
    rng = np.random.default_rng(seed)
    v0 = rng.normal(hp["v.init_mean"], hp["v.init_stdev"], (k, p)) if k > 0 else np.zeros((0, p))
    sample_seed = int(rng.integers(0, 2**63))
    eng = _engine_for(controls, p, (-1.0, 1.0), mode, batch_rows, device)
    eng.set_params(0.0, np.zeros(p), v0)
    mc, mi, mx = _rank_pairs(context, items, pos, device)
    for epoch in range(epochs):
        if n_candidates == 1:
            pm = Matrix.pairs(mc, mi, mx, n_neg, sample_seed, epoch)
        else:
            pm = Matrix.pairs_hard(eng, mc, mi, mx, n_neg, n_candidates, sample_seed, epoch)
        if pm.n:
            eng.train(pm, pm.n)
        pm.close()
    w0, w, v = eng.get_params()
    fit_model = {"w0": w0, "w": w, "v": v, "model.control": model, "solver.control": solver, "track.control": track, "convergence": False}
    scales = {"mean": None, "std": None, "model.vars": list(context.feature_names), "target.range": (-1.0, 1.0)}
    return {"class": "FM", "Model": fit_model, "Scales": scales, "engine": {"mode": mode, "batch_rows": batch_rows, "device": device},
            "rank": {"n_neg": n_neg, "epochs": epochs, "sample_seed": sample_seed, "n_candidates": n_candidates}}


def fm_rank_evaluate(object, context, items, positives, n_neg=1, seed=0):
    """Pairwise quality of a model on device-sampled pairs (fmx_matrix_pairs with `seed`, epoch 0): {"pair_acc": the share of pairs whose positive
    scores above the negative (ties count 1/2), "bpr": the mean BPR loss log(1 + exp(-d))}, from the raw scores of the concatenated rows."""
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    mdl = object["Model"]
    p = len(mdl["w"])
    _rank_inputs(context, items, p)
    if isinstance(n_neg, (bool, np.bool_)) or int(n_neg) != n_neg or int(n_neg) < 1:
        raise ValueError(f"n_neg must be an integer >= 1 (got {n_neg!r})")
    pos = _positives_csr(positives, context.dim[0], items.dim[0])
    hp = mdl["model.control"]["hyper.params"]
    device = object.get("engine", {}).get("device", 0)
    eng = Engine(p, task=L.TASK_RANKING, solver=L.SOLVER_SGD, num_factor=int(hp["factor.number"]), keep_w0=int(hp["keep.w0"]), keep_w1=int(hp["keep.w1"]),
                 mode=L.MODE_MINIBATCH, state_fp64=1, batch_rows=2, device=device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    mc, mi, mx = _rank_pairs(context, items, pos, device)
    pm = Matrix.pairs(mc, mi, mx, int(n_neg), int(seed), 0)
    if pm.n == 0:
        raise ValueError("positives holds no positive: there is no pair to evaluate")
    return {"pair_acc": eng.evaluate(pm, L.EVAL_PAIR_ACC), "bpr": eng.evaluate(pm, L.EVAL_BPR)}


def fm_explain(object, newdata, normalize=True, summary=False):
    """The exact contribution of every stored entry of `newdata` to its row's prediction -- predict(type = "terms") for a degree-2 FM.

    Contributions are on the RAW-SCORE scale, before the logistic, probit or clamp link that predict() applies, and their baseline is the
    EMPTY row (every feature absent), not an average over data: for every row, intercept + the row's contributions = its raw score.  The
    contribution of entry e is its Shapley value, phi_e = keep_w1 x_e w_j + 1/2 x_e sum_f v_jf (s_f - x_e v_jf) with s = sum over the row's
    entries of x v (include/fmx.h: fmx_contrib); a feature stored twice in a row is two entries.  With normalize (as in predict()) the values
    are first scaled by the model's Scales, and contributions refer to the values the model sees.

    Returns {"intercept": keep_w0 * w0, "contrib": scipy.sparse.csr_matrix (n x p)} whose stored pattern is newdata's (duplicates and explicit
    zeros kept, not summed); with summary=True also "summary": {"sum", "abs_sum", "count", "importance"} per feature over all rows, where
    importance = abs_sum / max(count, 1) is the mean |contribution| of the feature's entries."""
    import scipy.sparse as sp
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata must be a fm.matrix object")
    if np.any(np.isnan(newdata.features["value"])):
        raise ValueError("there are NAs in newdata")
    mdl = object["Model"]
    p = len(mdl["w"])
    if newdata.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    m = _device_matrix(newdata, None, device)
    if normalize:
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    phi = eng.contrib(m)
    rp, col, _, _ = m.export()
    out = {"intercept": float(mdl["w0"]) if controls["model"]["hyper.params"]["keep.w0"] else 0.0,
           "contrib": sp.csr_matrix((phi, col.astype(np.int64), rp), shape=(m.n, p))}
    if summary:
        sm = eng.contrib_summary(m)
        sm["importance"] = sm["abs_sum"] / np.maximum(sm["count"], 1)
        out["summary"] = sm
    return out


def fm_interactions(object, newdata, top=5, groups=None, normalize=True):
    """Which features interact in the rows of `newdata`, and how strongly: per row the `top` strongest pair terms of the degree-2 FM,
    I(a, b) = x_a x_b <v_a, v_b> -- the halves fm_explain hands to the two entries, and exactly their Shapley interaction index for the raw
    score with the empty row as baseline (include/fmx.h: fmx_interactions).  Strongest = the largest |I|; ties go to the earlier entries.
    Values are on the RAW-SCORE scale, and with normalize (as in predict()) they refer to the values the model sees.

    Returns {"row", "feature_a", "feature_b" (int64), "value" (float64)}: one element per reported pair, rows ascending, strongest first
    inside a row (rows with fewer than `top` pairs report what they have); feature_a / feature_b are the column ids of the two entries.
    With groups (one group id per feature, at most 64 groups -- the fields of one-hot data) also "summary": {"sum", "abs_sum", "count",
    "importance"} as G x G symmetric tables over every pair of every row, importance = abs_sum / max(count, 1), the mean |I| of a pair of
    the two groups."""
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata must be a fm.matrix object")
    if np.any(np.isnan(newdata.features["value"])):
        raise ValueError("there are NAs in newdata")
    mdl = object["Model"]
    p = len(mdl["w"])
    if newdata.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    top = int(top)
    if not 1 <= top <= 64:
        raise ValueError(f"top must be in 1..64 (got {top})")
    n_groups = 0
    if groups is not None:
        groups = np.asarray(groups)
        if groups.ndim != 1 or len(groups) != p or not np.issubdtype(groups.dtype, np.integer):
            raise ValueError(f"groups must hold one integer group id per feature ({p})")
        if p and groups.min() < 0:
            raise ValueError("group ids must be >= 0")
        n_groups = int(groups.max()) + 1 if p else 1
        if n_groups > 64:
            raise ValueError(f"at most 64 groups (got ids up to {n_groups - 1})")
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    m = _device_matrix(newdata, None, device)
    if normalize:
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    a, b, value = eng.interactions(m, top)
    rp, col, _, _ = m.export()
    row, slot = np.nonzero(a >= 0)
    col = col.astype(np.int64)
    out = {"row": row.astype(np.int64), "feature_a": col[rp[row] + a[row, slot]], "feature_b": col[rp[row] + b[row, slot]],
           "value": value[row, slot]}
    if groups is not None:
        sm = eng.interactions_summary(m, groups.astype(np.uint32), n_groups)
        sm["importance"] = sm["abs_sum"] / np.maximum(sm["count"], 1)
        out["summary"] = sm
    return out


_MET_NAMES = {"CLASSIFICATION": ("auc", "logloss", "accuracy", "brier", "mean_pred", "mean_label"),
              "REGRESSION": ("mse", "rmse", "mae", "mean_err", "mean_pred", "mean_label")}
_MET_COUNTS = ("rows", "positives", "pairs2", "correct")


def fm_metrics(object, newdata, groups=None, normalize=True):
    """Standard quality figures of a CLASSIFICATION or REGRESSION model on labelled data, pooled and per segment (include/fmx.h: fmx_metrics).

    CLASSIFICATION: "auc" (the exact Mann-Whitney AUC, ties as 1/2; NaN without both classes), "logloss" (mean negative log-likelihood),
    "accuracy" (cutoff 0.5), "brier", "mean_pred", "mean_label"; labels c(0, 1) or c(-1, 1).  REGRESSION: "mse", "rmse", "mae", "mean_err"
    (prediction - label), "mean_pred", "mean_label".  Predictions are predict()'s: the same link (logistic or probit, the clamp to the
    training range), the same normalization.  Unlike fm_track, which reproduces the reference's metric definitions, these are the usual ones.

    groups: one integer id per row (a user, a day, a campaign; any values).  Returns {"pooled": {name: value}, "groups": the distinct ids
    ascending (None without groups), "per_group": {name: float64[G]}, "counts": {"rows", "positives", "pairs2", "correct": int64[G]}} and for
    CLASSIFICATION "gauc", the per-group AUC weighted by the group's rows over the groups where it is defined (both classes present), and
    "macro_auc", their plain mean; NaN when no group has both classes.  Without groups the one group is the whole of newdata."""
    import math
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata must be a fm.matrix object")
    mdl = object["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    task = controls["model"]["task"]
    if task not in _MET_NAMES:
        raise ValueError("fm_metrics measures CLASSIFICATION and REGRESSION models (a RANK model has fm_rank_evaluate and fm_recommend_metrics)")
    if newdata.labels is None:
        raise ValueError("there are no labels in newdata")
    if np.any(np.isnan(newdata.features["value"])):
        raise ValueError("there are NAs in newdata")
    p = len(mdl["w"])
    if newdata.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, newdata {newdata.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize newdata because all the variables have not been normalized in FM model")
    n = newdata.dim[0]
    ids = dense = None
    if groups is not None:
        groups = np.asarray(groups)
        if groups.ndim != 1 or len(groups) != n or not np.issubdtype(groups.dtype, np.integer):
            raise ValueError(f"groups must hold one integer group id per row ({n})")
        ids, dense = np.unique(groups, return_inverse=True)
    y = _check_track_labels(newdata, task, "newdata")
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in newdata will not")
    m = _device_matrix(newdata, y, device)
    if normalize:
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    if task != "CLASSIFICATION":
        link = L.LINK_CLAMP
    else:  # predict()'s rule
        link = L.LINK_PROBIT if controls["solver"]["solver"]["solver"] in ("MCMC", "ALS") else L.LINK_LOGISTIC
    names = _MET_NAMES[task]
    pv, pc = eng.metrics(m, None, 1, link)
    out = {"pooled": {nm: float(pv[0, j]) for j, nm in enumerate(names)}, "groups": ids}
    if dense is None:
        gv, gc = pv, pc
    else:
        gv, gc = eng.metrics(m, dense.astype(np.uint32), max(len(ids), 1), link)
    out["per_group"] = {nm: gv[:, j].copy() for j, nm in enumerate(names)}
    out["counts"] = {nm: gc[:, j].copy() for j, nm in enumerate(_MET_COUNTS)}
    if task == "CLASSIFICATION":
        auc, rows = gv[:, L.MET_AUC], gc[:, L.MET_ROWS]
        ok = ~np.isnan(auc)
        if ok.any():
            out["gauc"] = math.fsum(float(a) * int(r) for a, r in zip(auc[ok], rows[ok])) / int(rows[ok].sum())
            out["macro_auc"] = math.fsum(float(a) for a in auc[ok]) / int(ok.sum())
        else:
            out["gauc"] = out["macro_auc"] = float("nan")
    return out


def _calibration_check(calibration):
    """a calibration object (fm_calibrate, fm_prior_correction) or None; every refusal before any device is touched"""
    if calibration is None:
        return
    if not isinstance(calibration, dict) or calibration.get("class") != "FMcalibration":
        raise TypeError("calibration must be a calibration object (fm_calibrate, fm_prior_correction) or None")


def _calibration_setup(object, data, groups, normalize, who, calibration=None, need_labels=True):
    """what fm_reliability, fm_calibrate and fm_predict_calibrated share: the checks of fm_metrics (labels, groups, feature count), the model's
    engine and the device matrix -- (engine, matrix, dense group ids or None, the distinct ids or None, the model's link)"""
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    if not isinstance(data, FmMatrix):
        raise TypeError(f"{who}: the data must be a fm.matrix object")
    _calibration_check(calibration)
    mdl = object["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    task = controls["model"]["task"]
    if task != "CLASSIFICATION":
        raise ValueError(f"{who} calibrates CLASSIFICATION models only")
    if data.labels is None and need_labels:
        raise ValueError("there are no labels in the data")
    if np.any(np.isnan(data.features["value"])):
        raise ValueError("there are NAs in the data")
    p = len(mdl["w"])
    if data.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, the data {data.dim[1]}")
    if normalize and object["Scales"]["mean"] is None:
        raise ValueError("can not normalize the data because all the variables have not been normalized in FM model")
    n = data.dim[0]
    ids = dense = None
    if groups is not None:
        groups = np.asarray(groups)
        if groups.ndim != 1 or len(groups) != n or not np.issubdtype(groups.dtype, np.integer):
            raise ValueError(f"groups must hold one integer group id per row ({n})")
        ids, dense = np.unique(groups, return_inverse=True)
        if calibration is not None and calibration["groups"] is not None:
            where = np.searchsorted(calibration["groups"], ids)
            where[where == len(calibration["groups"])] = 0
            if len(calibration["groups"]) == 0 or np.any(calibration["groups"][where] != ids):
                raise ValueError("groups holds ids that the calibration was not fitted on")
            ids, dense = calibration["groups"], where[dense]
    elif calibration is not None and calibration["groups"] is not None:
        raise ValueError("the calibration was fitted per group: groups is needed")
    # (the calls take a labelled matrix; where nobody reads the labels, any will do)
    y = np.ones(n) if not need_labels else _check_track_labels(data, task, "data")
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    if not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in the data will not")
    m = _device_matrix(data, y, device)
    if normalize:
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    link = L.LINK_PROBIT if controls["solver"]["solver"]["solver"] in ("MCMC", "ALS") else L.LINK_LOGISTIC   # predict()'s rule
    return eng, m, (None if dense is None else dense.astype(np.uint32)), ids, link


_CAL_VALUES = ("ece", "mce", "brier", "logloss")


def fm_reliability(object, newdata, groups=None, bins=10, binning="width", calibration=None, normalize=True):
    """The reliability table of a CLASSIFICATION model on labelled data, pooled or per segment (include/fmx.h: fmx_reliability): how far the
    predicted probabilities are from the observed rates.

    binning "width": bins equal-width bins of the probability; "mass": bins equal-mass bins of the raw score (equal scores stay together).
    calibration: a calibration object (fm_calibrate, fm_prior_correction) to measure the calibrated probabilities, or None for predict()'s own.
    groups: one integer id per row.  Returns {"groups": the distinct ids ascending (None without groups), "rows", "positives" int64[G, bins],
    "mean_pred", "rate" float64[G, bins] (NaN for an empty bin), "lo_score", "hi_score" float64[G, bins], "nan_rows" int64[G], "ece", "mce",
    "brier", "logloss" float64[G]}: "ece" is the expected calibration error, the bins' |mean_pred - rate| weighted by their rows."""
    if binning not in ("width", "mass"):
        raise ValueError('binning must be "width" or "mass"')
    if int(bins) != bins or not 1 <= int(bins) <= 1024:
        raise ValueError("bins must be an integer in 1..1024")
    eng, m, dense, ids, link = _calibration_setup(object, newdata, groups, normalize, "fm_reliability", calibration)
    G = 1 if dense is None else max(len(ids), 1)
    t = eng.reliability(m, dense, G, int(bins), L.BINS_WIDTH if binning == "width" else L.BINS_MASS, None if calibration is None else calibration["map"], link)
    rows, pos = t["count"][:, :, 0], t["count"][:, :, 1]
    with np.errstate(all="ignore"):
        out = {"groups": ids, "rows": rows, "positives": pos, "mean_pred": np.where(rows > 0, t["sum_p"] / rows, np.nan), "rate": np.where(rows > 0, pos / rows, np.nan),
               "lo_score": t["lo_z"], "hi_score": t["hi_z"], "nan_rows": t["nan_rows"]}
    for j, nm in enumerate(_CAL_VALUES):
        out[nm] = t["value"][:, j].copy()
    return out


def fm_calibrate(object, data, method="platt", groups=None, bins=256, l2=0.1, newton_steps=8, normalize=True):
    """Fit a calibration map for a CLASSIFICATION model on labelled data (a calibration fold: fm_split, fm_folds), one map or one per segment.

    method "platt": p = logistic(a z + b) on the raw score z, by newton_steps Newton steps from the identity under the ridge l2 / 2 ((a - 1)^2 +
    b^2) (include/fmx.h: fmx_calibrate_platt).  "isotonic": the monotone step map over `bins` equal-mass bins of the score
    (fmx_calibrate_isotonic).  Returns a calibration object for fm_predict_calibrated and fm_reliability: {"class": "FMcalibration", "method",
    "groups": the distinct ids ascending or None, "map": the fitted arrays, and for "platt" "rows" and "status" (1: the group was not solved and
    predicts NaN; a warning is issued)}."""
    if method not in ("platt", "isotonic"):
        raise ValueError('method must be "platt" or "isotonic"')
    if method == "isotonic" and (int(bins) != bins or not 1 <= int(bins) <= 1024):
        raise ValueError("bins must be an integer in 1..1024")
    if method == "platt" and (not l2 >= 0 or int(newton_steps) != newton_steps or newton_steps < 1):
        raise ValueError("l2 must be a number >= 0 and newton_steps an integer >= 1")
    eng, m, dense, ids, _ = _calibration_setup(object, data, groups, normalize, "fm_calibrate")
    G = 1 if dense is None else max(len(ids), 1)
    out = {"class": "FMcalibration", "method": method, "groups": ids}
    if method == "platt":
        fit = eng.calibrate_platt(m, dense, G, l2, int(newton_steps))
        out["rows"], out["status"] = fit.pop("rows"), fit.pop("status")
        if out["status"].any():
            warnings.warn(f"{int(out['status'].sum())} group(s) could not be solved and predict NaN")
    else:
        fit = eng.calibrate_isotonic(m, dense, G, int(bins))
    out["map"] = fit
    return out


def fm_prior_correction(negative_rate):
    """The closed-form correction for a model trained on data whose negatives were kept with probability negative_rate (0 < negative_rate <= 1):
    the Platt map (a, b) = (1, log(negative_rate)), which shifts the log-odds back to the full population's.  Host arithmetic only."""
    import math
    r = float(negative_rate)
    if not 0.0 < r <= 1.0:
        raise ValueError("negative_rate must be in (0, 1]")
    return {"class": "FMcalibration", "method": "platt", "groups": None, "map": {"kind": "platt", "ab": np.array([[1.0, math.log(r)]])},
            "rows": np.zeros(1, np.int64), "status": np.zeros(1, np.int32)}


def fm_predict_calibrated(object, newdata, calibration, groups=None, normalize=True):
    """predict() followed by a calibration map, on the device (include/fmx.h: fmx_predict_calibrated): float64[n] probabilities.  A calibration
    fitted per group needs groups, one integer id per row, each one of the ids it was fitted on."""
    if calibration is None:
        raise TypeError("calibration must be a calibration object (fm_calibrate, fm_prior_correction)")
    _calibration_check(calibration)
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata must be a fm.matrix object")
    eng, m, dense, ids, link = _calibration_setup(object, newdata, groups, normalize, "fm_predict_calibrated", calibration, need_labels=False)
    G = 1 if dense is None else max(len(ids), 1)
    return eng.predict_calibrated(m, calibration["map"], dense, G, link)


def fm_fold_in(object, data, features, l2_w=0.1, l2_v=0.1, newton_steps=8, normalize=True):
    """Fold new features into a fitted model: everything learned stays fixed, and only the rows (w_u, v_u) of the listed features are solved
    from the rows of `data` that store them (include/fmx.h: fmx_fold_in) -- the closed-form ridge solution under the squared loss for a
    REGRESSION model, newton_steps Newton steps of the logistic loss for a CLASSIFICATION model.  l2_w / l2_v are the ridge weights on w_u
    and v_u.  A row of `data` may store at most one of the listed features; rows that store none are ignored.

    data: a fm.matrix with labels (checked and mapped as fm_train does; with normalize its values are scaled by the model's Scales if the
    model has any).  features: column indices (0-based) or feature names.  Returns a new FM object -- `object` is left untouched -- in which
    the solved features' w and v are replaced, with "fold.in": {"features", "rows", "status"} (rows: how many rows held the feature;
    status 1: the normal equations were not positive definite -- such a feature keeps its old row, and a warning is issued).

    RANK models and CLASSIFICATION models trained by MCMC or ALS are refused: the latter predict through the probit link, which a logistic
    fit would not match."""
    import copy
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    if not isinstance(data, FmMatrix):
        raise TypeError("data must be a fm.matrix object")
    mdl = object["Model"]
    task = mdl["model.control"]["task"]
    if task == "RANK":
        raise ValueError("fm_fold_in does not fold into a RANK model (a pairwise fold-in is not built)")
    if task == "CLASSIFICATION" and mdl["solver.control"]["solver"]["solver"] in ("MCMC", "ALS"):
        raise ValueError("fm_fold_in fits the logistic loss: a CLASSIFICATION model trained by MCMC or ALS predicts through the probit link")
    p = len(mdl["w"])
    if data.dim[1] != p:
        raise ValueError(f"number of input's features is not correct: the model has {p}, data {data.dim[1]}")
    if np.any(np.isnan(data.features["value"])):
        raise ValueError("there are NAs in data")
    names = list(object["Scales"]["model.vars"])
    if list(data.feature_names) != names:   # as fm_update: another column order would fold the wrong column
        raise ValueError("the features in data are not the same as those in FM model")
    ids = []
    for f in features:
        if isinstance(f, str):
            if f not in names:
                raise ValueError(f"feature {f!r} is not in the model")
            ids.append(names.index(f))
        else:
            if int(f) != f or not 0 <= int(f) < p:
                raise ValueError(f"feature index {f!r} out of range")
            ids.append(int(f))
    if len(set(ids)) != len(ids):
        raise ValueError("a feature is listed twice")
    y = _check_labels(data, task)
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, p, object["Scales"]["target.range"], "sequential_bitwise", 1, device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    m = _device_matrix(data, y, device)
    if normalize and object["Scales"]["mean"] is not None:
        m.normalize(object["Scales"]["mean"], object["Scales"]["std"])
    elif not normalize and object["Scales"]["mean"] is not None:
        warnings.warn("some variables in FM model are normalized, but those in data will not")
    w, v, rows, status = eng.fold_in(m, ids, l2_w, l2_v, newton_steps=newton_steps, apply=False)
    out = copy.deepcopy(object)
    ok = status == 0
    idx = np.asarray(ids, np.int64)
    out["Model"]["w"] = np.array(mdl["w"], np.float64)
    out["Model"]["v"] = np.array(mdl["v"], np.float64)
    out["Model"]["w"][idx[ok]] = w[ok]
    if out["Model"]["v"].shape[0] > 0:
        out["Model"]["v"][:, idx[ok]] = v[:, ok]
    if not np.all(ok):
        warnings.warn(f"{int(np.sum(~ok))} feature(s) could not be solved (status 1) and keep their rows: " + ", ".join(names[j] for j in idx[~ok][:10]))
    out["fold.in"] = {"features": [names[j] for j in ids], "rows": rows.copy(), "status": status.copy()}
    return out


def fm_fold_in_rank(object, context, items, positives, features, n_neg=4, l2_w=0.1, l2_v=0.1, newton_steps=8, seed=0):
    """Fold new users or new items into a fitted RANK model: everything learned stays fixed, and only the rows (w_u, v_u) of the listed
    features are solved, by newton_steps Newton steps of the pairwise logistic (BPR) loss on device-sampled pairs (include/fmx.h:
    fmx_fold_in_pairs).  context, items, positives are as for fm_train_rank; pass the contexts that matter -- the new
    users' rows, or the contexts whose positives include the new items.  The pairs are fmx_matrix_pairs' with n_neg negatives per positive,
    `seed` and epoch 0, as fm_rank_evaluate draws them; a pair takes part if one of its rows stores a listed feature.

    features: column indices (0-based) or feature names.  l2_w / l2_v: the ridge weights on w_u and v_u.  A pair carries no information on the
    w of a feature that sits in both of its rows (a new user): with l2_w > 0 such a w comes out exactly 0, with l2_w = 0 the feature is not
    solved (status 1) unless the model has keep.w1 = False.  A row may store at most one listed feature: a new user and a new item that meet
    in one row are folded in separate calls.

    Returns a new FM object -- `object` is left untouched -- in which the solved features' w and v are replaced, with "fold.in":
    {"features", "pairs", "status"} (pairs: how many pairs held the feature; status 1: the Newton system was not positive definite -- such
    a feature keeps its old row, and a warning is issued).  Models of other tasks are refused: fm_fold_in folds into those."""
    import copy
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    mdl = object["Model"]
    if mdl["model.control"]["task"] != "RANK":
        raise ValueError(f"fm_fold_in_rank folds into a RANK model (this one's task is {mdl['model.control']['task']}: use fm_fold_in)")
    p = len(mdl["w"])
    _rank_inputs(context, items, p)
    if isinstance(n_neg, (bool, np.bool_)) or int(n_neg) != n_neg or int(n_neg) < 1:
        raise ValueError(f"n_neg must be an integer >= 1 (got {n_neg!r})")
    names = list(object["Scales"]["model.vars"])
    for name, d in (("context", context), ("items", items)):
        if list(d.feature_names) != names:   # as fm_fold_in: another column order would fold the wrong column
            raise ValueError(f"the features in {name} are not the same as those in FM model")
    ids = []
    for f in features:
        if isinstance(f, str):
            if f not in names:
                raise ValueError(f"feature {f!r} is not in the model")
            ids.append(names.index(f))
        else:
            if int(f) != f or not 0 <= int(f) < p:
                raise ValueError(f"feature index {f!r} out of range")
            ids.append(int(f))
    if len(set(ids)) != len(ids):
        raise ValueError("a feature is listed twice")
    pos = _positives_csr(positives, context.dim[0], items.dim[0])
    hp = mdl["model.control"]["hyper.params"]
    device = object.get("engine", {}).get("device", 0)
    eng = Engine(p, task=L.TASK_RANKING, solver=L.SOLVER_SGD, num_factor=int(hp["factor.number"]), keep_w0=int(hp["keep.w0"]), keep_w1=int(hp["keep.w1"]),
                 mode=L.MODE_MINIBATCH, state_fp64=1, batch_rows=2, device=device)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    mc, mi, mx = _rank_pairs(context, items, pos, device)
    pm = Matrix.pairs(mc, mi, mx, int(n_neg), int(seed), 0)
    try:
        w, v, pairs, status = eng.fold_in_pairs(pm, ids, l2_w, l2_v, newton_steps=newton_steps, apply=False)
    except L.FmxError as err:
        if "more than one entry of the fold features" in str(err):
            raise ValueError("a row of the pairs stores two of the listed features (a new user and a new item that meet in one row?): "
                             "fold users and items in separate calls") from err
        raise
    out = copy.deepcopy(object)
    ok = status == 0
    idx = np.asarray(ids, np.int64)
    out["Model"]["w"] = np.array(mdl["w"], np.float64)
    out["Model"]["v"] = np.array(mdl["v"], np.float64)
    out["Model"]["w"][idx[ok]] = w[ok]
    if out["Model"]["v"].shape[0] > 0:
        out["Model"]["v"][:, idx[ok]] = v[:, ok]
    if not np.all(ok):
        warnings.warn(f"{int(np.sum(~ok))} feature(s) could not be solved (status 1) and keep their rows: " + ", ".join(names[j] for j in idx[~ok][:10]))
    out["fold.in"] = {"features": [names[j] for j in ids], "pairs": pairs.copy(), "status": status.copy()}
    return out


def _check_track_labels(data, task, what):
    y = np.asarray(data.labels, np.float64)
    if task == "CLASSIFICATION":  # R/fm_track.R:44-53
        u = np.unique(y)
        if len(u) != 2:
            raise ValueError(f"{what}'s target should have two levels")
        if np.array_equal(u, [0.0, 1.0]):
            y = np.where(y < 1, -1.0, 1.0)
        elif not np.array_equal(u, [-1.0, 1.0]):
            raise ValueError(f"{what}'s target should be c(0, 1) or c(-1, 1)")
    return y


def _fm_track_eval(object, data, metric):
    """FMTrack (src/FM.cpp:218-258): the metric of every recorded snapshot on `data` (Tracker::report, core/Tracker.h:70-94)."""
    mdl = object["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    task = controls["model"]["task"]
    device = object.get("engine", {}).get("device", 0)
    eng = _engine_for(controls, data.dim[1], object["Scales"]["target.range"], "sequential", 1, device)
    m = _device_matrix(data, _check_track_labels(data, task, "data"), device)
    out = []
    for snap in object["Trace"]["trace"][1:]:
        eng.set_params(snap["w0"], snap["w"], snap["v"])
        out.append(eng.evaluate(m, getattr(L, "EVAL_" + metric)))
    return np.array(out)


def fm_track(object, data=None, newdata=None, evaluate_metric="LL"):
    """fm.track() -- R/fm_track.R:28-86: the training-trace metric and the same metric on new data per snapshot."""
    if object.get("Trace") is None:
        raise ValueError("no Trace in fm object")
    task = object["Model"]["model.control"]["task"]
    if evaluate_metric not in ("LL", "AUC", "ACC", "RMSE", "MAE"):
        raise ValueError("'arg' should be one of 'LL', 'AUC', 'ACC', 'RMSE', 'MAE'")
    if (task == "CLASSIFICATION" and evaluate_metric in ("RMSE", "MAE")) or (task == "REGRESSION" and evaluate_metric in ("LL", "AUC", "ACC")):
        raise ValueError("evaluate.metric is error")
    if object["Model"]["track.control"]["evaluate.metric"] != evaluate_metric:
        if data is None:
            raise ValueError("data is missing")
        if not isinstance(data, FmMatrix):
            raise TypeError("data is not a fm.matrix object")
        val1 = _fm_track_eval(object, data, evaluate_metric)
    else:
        val1 = np.asarray(object["Trace"]["evaluation.train"])
    if newdata is None:
        raise ValueError("newdata is missing")
    if not isinstance(newdata, FmMatrix):
        raise TypeError("newdata is not a fm.matrix object")
    val2 = _fm_track_eval(object, newdata, evaluate_metric)
    return {"class": "FMTrace", "iter": np.asarray(object["Trace"]["trace"][0]), "trace.train": val1, "trace.test": val2,
            "evaluate.metric": evaluate_metric}


def fm_select(object, trace=None, best_iter=None, drop_trace=False):
    """fm.select() -- R/fm_select.R:22-66: put the best snapshot (by the test trace) into the model."""
    if trace is None:
        raise ValueError("trace is missing")
    if not isinstance(trace, dict) or trace.get("class") != "FMTrace":
        raise TypeError("trace is not a FMTrace object")
    if object.get("Trace") is None or len(object["Trace"]) <= 1:
        raise ValueError("the Trace part in object have been dropped")
    bigger_is_better = object["Model"]["track.control"]["evaluate.metric"] in ("LL", "ACC", "AUC")  # cmp(), R/fm_select.R:69-77
    better = (lambda a, b: a > b) if bigger_is_better else (lambda a, b: a < b)
    pick = np.max if bigger_is_better else np.min
    iterations = np.asarray(object["Trace"]["trace"][0])
    test, train = np.asarray(trace["trace.test"]), np.asarray(trace["trace.train"])
    if best_iter is not None:
        if best_iter < iterations[0] or best_iter > iterations[-1]:
            raise ValueError("best.iter is out of range")
        if best_iter in iterations:
            idx = int(np.where(iterations == best_iter)[0][0])
        else:  # the recorded neighbour with the better test metric (R/fm_select.R:43-48, 1-based there)
            i1 = int(np.argmin(best_iter >= iterations)) - 1
            idx = i1 if (i1 + 1 >= len(iterations) or better(test[i1], test[i1 + 1])) else i1 + 1
    else:
        cand = np.where(test == pick(test))[0]
        idx = int(cand[0]) if len(cand) == 1 else int(np.where(train == pick(train[cand]))[0][0])
    snap = object["Trace"]["trace"][idx + 1]
    out = dict(object)
    out["Model"] = dict(object["Model"], w0=snap["w0"], w=snap["w"], v=snap["v"])
    if drop_trace:
        out.pop("Trace", None)
    return out


_SPLIT_HOW = {"rows": L.SPLIT_ROWS, "within": L.SPLIT_WITHIN_GROUPS, "groups": L.SPLIT_GROUPS}
_SPLIT_ORDER = {"random": L.SPLIT_ORDER_HASH, "last": L.SPLIT_ORDER_TAIL}


def _split_int(name, value, lo):
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < lo:
        raise ValueError(f"{name} must be an integer >= {lo} (got {value!r})")
    return int(value)


def _split_groups(data, by, how):
    """the checks fm_split and fm_folds share, on the host: (scope, dense group ids or None, their number)"""
    if not isinstance(data, FmMatrix):
        raise TypeError("data must be a fm.matrix object")
    if how not in _SPLIT_HOW:
        raise ValueError(f'how must be "rows", "within" or "groups" (got {how!r})')
    n = data.dim[0]
    if by is None:
        if how != "rows":
            raise ValueError(f'how = "{how}" needs `by`: one integer group id per row')
        return _SPLIT_HOW[how], None, 1
    by = np.asarray(by)
    if by.ndim != 1 or len(by) != n or not np.issubdtype(by.dtype, np.integer):
        raise ValueError(f"by must hold one integer group id per row ({n})")
    ids, dense = np.unique(by, return_inverse=True)
    return _SPLIT_HOW[how], dense.astype(np.uint32), max(len(ids), 1)


def _host_matrix(m, labels, feature_names):
    """a device Matrix back as a fm.matrix (values as the device holds them: fp32)"""
    rp, col, val, _ = m.export()
    features = {"value": val.astype(np.float64), "col_idx": col.astype(np.int32), "row_size": np.diff(rp).astype(np.int32), "dim": (m.n, m.p),
                "size": int(len(col))}
    return FmMatrix(features, labels, list(feature_names))


def fm_split(data, test_fraction=0.2, test_count=None, by=None, how="rows", order="random", min_keep=0, seed=0, device=0):
    """Cut a fm.matrix into a train and a test part on the device (include/fmx.h: fmx_split_assign, fmx_matrix_select).

    how = "rows": test_count rows (or floor(test_fraction * rows)) of the whole matrix go to test.  how = "within": that many of every group
    of `by` (a stratified split; by = the label stratifies by label, by = the user leaves test_count rows of every user out), never more than
    leave min_keep rows of the group in train.  how = "groups": that many whole groups go to test, so no group has rows on both sides (the
    split GAUC figures need).  order = "random" picks by a hash of (seed, row index) -- the same call gives the same split, and a smaller
    test_count's test set is part of a larger one's --, order = "last" takes the last rows (of the matrix, of every group) or the last group
    ids: a temporal hold-out on data in time order.  by: one integer id per row, any values.
    Returns (train, test, test_mask): fm.matrix objects with the rows in their original order, labels and feature names carried over, ready for
    fm_train, fm_metrics and fm_track, and the boolean mask of the rows that went to test.  Stored values come back as the device holds them
    (single precision, which is what training reads)."""
    scope, groups, n_groups = _split_groups(data, by, how)
    if order not in _SPLIT_ORDER:
        raise ValueError(f'order must be "random" or "last" (got {order!r})')
    count = 0 if test_count is None else _split_int("test_count", test_count, 1)
    frac = float(test_fraction)
    if test_count is None and not 0.0 <= frac <= 1.0:   # (false for NaN)
        raise ValueError(f"test_fraction must be in [0, 1] (got {test_fraction!r})")
    min_keep = _split_int("min_keep", min_keep, 0)
    seed = _split_int("seed", seed, 0)
    n = data.dim[0]
    part = split_assign(n, groups, n_groups, scope=scope, order=_SPLIT_ORDER[order], hold_count=count, hold_fraction=0.0 if count else frac,
                        min_keep=min_keep, seed=seed, device=device)
    m = _device_matrix(data, None, device)
    out = []
    mask = np.zeros(n, bool)
    for which in (0, 1):
        sub, rows = m.select(part, which, return_rows=True)
        labels = None if data.labels is None else np.asarray(data.labels)[rows]
        out.append(_host_matrix(sub, labels, data.feature_names))
        sub.close()
        if which == 1:
            mask[rows] = True
    m.close()
    return out[0], out[1], mask


def fm_folds(data, k, by=None, how="rows", seed=0, device=0):
    """The fold 0 .. k-1 of every row of `data` for k-fold cross-validation (include/fmx.h: fmx_split_assign): int64[rows].  how = "rows":
    folds of the whole matrix; "within": every group of `by` is spread over the folds (sizes inside a group differ by at most one);
    "groups": whole groups go to a fold.  Fold f's test rows are folds == f, its train rows the rest."""
    scope, groups, n_groups = _split_groups(data, by, how)
    k = _split_int("k", k, 2)
    if k > 65536:
        raise ValueError(f"k must be at most 65536 (got {k})")
    seed = _split_int("seed", seed, 0)
    return split_assign(data.dim[0], groups, n_groups, scope=scope, n_folds=k, seed=seed, device=device).astype(np.int64)


def fm_holdout(positives, hold=1, fraction=None, order="random", min_keep=1, seed=0, device=0):
    """Split the positives of fm_train_rank into a train part and a held-out part per context (include/fmx.h: fmx_matrix_split_entries).

    positives: what fm_train_rank takes -- a scipy sparse matrix (context rows x item rows; stored entries = positives) or a list of index
    arrays, one per context.  Of every context, `hold` positives (or floor(fraction * its positives)) are held out, never more than leave
    min_keep behind: hold = 1, min_keep = 1 is leave-one-out that keeps every context trainable.  order = "random": chosen by a hash of
    (seed, context, item); "last": the last stored ones (leave-last-out on lists in time order).
    Returns (train_positives, heldout) in the form positives came in: fm_train_rank(positives = train_positives), then
    fm_recommend_metrics(heldout = heldout, exclude = train_positives)."""
    import scipy.sparse as sp
    if order not in _SPLIT_ORDER:
        raise ValueError(f'order must be "random" or "last" (got {order!r})')
    if fraction is None:
        hold, frac = _split_int("hold", hold, 1), None
    else:
        frac = float(fraction)
        if not 0.0 <= frac <= 1.0:
            raise ValueError(f"fraction must be in [0, 1] (got {fraction!r})")
    min_keep = _split_int("min_keep", min_keep, 0)
    seed = _split_int("seed", seed, 0)
    sparse = sp.issparse(positives)
    if sparse:
        n_ctx, n_items = positives.shape
    else:
        positives = [np.asarray(r, np.int64).ravel() for r in positives]
        n_ctx = len(positives)
        n_items = max([int(r.max()) + 1 for r in positives if r.size] + [1])
    rp, col = _exclude_csr(positives, n_ctx, n_items, name="positives")
    if col.size and (col.min() < 0 or col.max() >= n_items):
        raise ValueError(f"positives holds item indices outside 0..{n_items - 1}")
    m = Matrix.from_csr(rp, col.astype(np.uint32), np.ones(len(col), np.float32), n_items, device=device)
    kept, held = m.split_entries(hold=hold, fraction=frac, order=_SPLIT_ORDER[order], min_keep=min_keep, seed=seed)
    out = []
    for part in (kept, held):
        prp, pcol, _, _ = part.export()
        part.close()
        if sparse:
            out.append(sp.csr_matrix((np.ones(len(pcol)), pcol.astype(np.int64), prp), shape=(n_ctx, n_items)))
        else:
            out.append([pcol[prp[c]:prp[c + 1]].astype(np.int64) for c in range(n_ctx)])
    m.close()
    return out[0], out[1]


_RARE = {"drop": L.RARE_DROP, "bucket": L.RARE_BUCKET}
_COMBINE = {"keep": L.COMBINE_KEEP, "sum": L.COMBINE_SUM, "first": L.COMBINE_FIRST}


class ColumnMap:
    """What fm_prune_features and fm_hash_features decided, to be applied again (fm_apply_columns: validation and serving data; fm_remap_model).
    map: uint32[old features], the new id of every old one (0xFFFFFFFF: dropped); new_p; combine: how entries that meet in one new id are
    merged; carried: bool[old features], the features whose model rows move with them (fm_remap_model); segment_base: the segments' new ranges."""

    def __init__(self, cmap, new_p, combine, carried, feature_names, new_feature_names, segment_base=None, kind="prune"):
        self.map, self.new_p, self.combine, self.carried = cmap, int(new_p), combine, carried
        self.feature_names, self.new_feature_names, self.segment_base, self.kind = list(feature_names), list(new_feature_names), segment_base, kind


def _columns_data(data, who):
    if not isinstance(data, FmMatrix):
        raise TypeError("data must be a fm.matrix object")
    if data.features["size"] > 2**31 - 1 or data.dim[0] > 2**31 - 1:
        raise ValueError(f"{who} takes at most 2^31 - 1 rows and stored entries")
    return data.dim[1]


def _columns_int(name, value, lo, hi=None, none=None):
    if value is None and none is not None:
        return none
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError(f"{name} must be an integer in {lo}..{'' if hi is None else hi} (got {value!r})")
    return int(value)


def _columns_combine(combine):
    if combine not in _COMBINE:
        raise ValueError(f'combine must be "keep", "sum" or "first" (got {combine!r})')
    return combine


def _remapped(m, data, cmap, new_p, combine, names):
    out = m.remap_columns(cmap, new_p, _COMBINE[combine])
    host = _host_matrix(out, data.labels, names)
    out.close()
    return host


def fm_feature_stats(data, device=0):
    """How often every feature occurs, counted on the device (include/fmx.h: fmx_matrix_column_stats).  Returns a dict of
    arrays over the features: "entries" (stored entries), "rows" (rows that store the feature at least once), "positive_rows" (those with a
    label > 0; zeros without labels), "sum" and "sum_sq" (of the stored values, read in single precision as training reads them, added in the
    fixed order the header states), and "feature_names"."""
    _columns_data(data, "fm_feature_stats")
    m = _device_matrix(data, data.labels, device)
    count, value = m.column_stats()
    m.close()
    return {"entries": count[:, 0].copy(), "rows": count[:, 1].copy(), "positive_rows": count[:, 2].copy(), "sum": value[:, 0].copy(),
            "sum_sq": value[:, 1].copy(), "feature_names": list(data.feature_names)}


def fm_prune_features(data, min_rows=1, max_rows=None, max_features=None, keep_prefix=0, rare="drop", fields=None, combine=None, device=0):
    """Drop or bucket the features that occur too rarely or too often, on the device (include/fmx.h: fmx_matrix_column_stats,
    fmx_column_map_select, fmx_matrix_remap_columns).

    A feature from keep_prefix on survives if it occurs in at least min_rows and (max_rows given) at most max_rows rows; with max_features only
    that many survive, the most frequent ones, ties to the lower id.  The first keep_prefix features (dense columns) always survive.  rare =
    "drop" removes the other features' entries; rare = "bucket" sends them to one out-of-vocabulary feature per field -- fields: the ascending
    feature offsets of the fields from 0 to the feature count (None: one field), as a one-hot encoded data frame has them -- which exists
    whether or not anything maps to it, so the layout does not depend on the data.  combine ("keep", "sum", "first") says what happens to
    entries of one row that meet in a bucket: None takes "keep" under "drop" (nothing meets) and "sum" under "bucket"; "first" keeps one-hot
    data one-hot.  Returns (the new fm.matrix, a ColumnMap for fm_apply_columns and fm_remap_model)."""
    p = _columns_data(data, "fm_prune_features")
    if rare not in _RARE:
        raise ValueError(f'rare must be "drop" or "bucket" (got {rare!r})')
    min_rows = _columns_int("min_rows", min_rows, 0)
    max_rows = _columns_int("max_rows", max_rows, 1, none=0)
    max_features = _columns_int("max_features", max_features, 1, none=0)
    keep_prefix = _columns_int("keep_prefix", keep_prefix, 0, p)
    combine = _columns_combine(("keep" if rare == "drop" else "sum") if combine is None else combine)
    base = None
    if fields is not None:
        base = np.asarray(fields)
        if base.ndim != 1 or len(base) < 2 or not np.issubdtype(base.dtype, np.integer) or base[0] != 0 or base[-1] != p or np.any(np.diff(base) < 0):
            raise ValueError(f"fields must ascend from 0 to the feature count ({p})")
        base = base.astype(np.uint32)
    m = _device_matrix(data, None, device)
    count, _ = m.column_stats(values=False)
    cmap, new_p, nsb = column_map_select(p, count, device=device, by=L.COLUMNS_BY_ROWS, min_count=min_rows, max_count=max_rows,
                                         max_features=max_features, keep_prefix=keep_prefix, rare=_RARE[rare], segment_base=base)
    kept = np.zeros(p, bool)
    names = [None] * new_p
    if rare == "bucket":
        for s in range(len(nsb) - 1):
            names[int(nsb[s + 1]) - 1] = f"rare{s + 1}"
        buckets = nsb[1:].astype(np.int64) - 1
        kept = ~np.isin(cmap.astype(np.int64), buckets)
    else:
        kept = cmap != L.COLUMN_DROP
    for j in np.flatnonzero(kept):
        names[int(cmap[j])] = data.feature_names[j]
    out = _remapped(m, data, cmap, new_p, combine, names)
    m.close()
    return out, ColumnMap(cmap, new_p, combine, kept, data.feature_names, names, nsb, "prune")


def fm_hash_features(data, n_buckets, seed=0, keep_prefix=0, combine="sum", device=0):
    """The hashing trick on the device (include/fmx.h: fmx_column_map_hash, fmx_matrix_remap_columns): the first keep_prefix features stay,
    every other feature goes to one of n_buckets features behind them by a hash of (seed, feature id); entries of a row that meet are merged
    by `combine`.  Unsigned: there is no sign hash.  Returns (the new fm.matrix, a ColumnMap)."""
    p = _columns_data(data, "fm_hash_features")
    keep_prefix = _columns_int("keep_prefix", keep_prefix, 0, p)
    n_buckets = _columns_int("n_buckets", n_buckets, 1, 2**32 - 2 - keep_prefix)
    seed = _columns_int("seed", seed, 0, 2**64 - 1)
    combine = _columns_combine(combine)
    m = _device_matrix(data, None, device)
    count, _ = m.column_stats(values=False)
    cmap, new_p = column_map_hash(p, n_buckets, seed=seed, keep_prefix=keep_prefix, device=device)
    names = list(data.feature_names[:keep_prefix]) + [f"h{b + 1}" for b in range(n_buckets)]
    carried = count[:, 0] > 0
    carried[:keep_prefix] = True
    out = _remapped(m, data, cmap, new_p, combine, names)
    m.close()
    return out, ColumnMap(cmap, new_p, combine, carried, data.feature_names, names, None, "hash")


def fm_apply_columns(data, cmap, device=0):
    """The column map of fm_prune_features / fm_hash_features on other data with the same features (validation, test and serving data): the
    same ids, buckets and merge.  Returns the new fm.matrix."""
    p = _columns_data(data, "fm_apply_columns")
    if not isinstance(cmap, ColumnMap):
        raise TypeError("cmap must be the column map fm_prune_features or fm_hash_features returned")
    if p != len(cmap.map) or list(data.feature_names) != cmap.feature_names:
        raise ValueError("the features in data are not the same as those the column map was made for")
    m = _device_matrix(data, None, device)
    out = _remapped(m, data, cmap.map, cmap.new_p, cmap.combine, cmap.new_feature_names)
    m.close()
    return out


def fm_remap_model(object, cmap):
    """A fitted FM moved into a column map's feature space (on the host, in numpy): a carried feature -- a survivor of fm_prune_features, a
    feature that occurred in the data fm_hash_features saw -- takes its w and its V column (and its normalisation) along; buckets, and ids that
    only unseen features map to, start at zero.  Refused for a map that sends two carried features to one id (two occurring features that share
    a hash bucket: their rows cannot both live there).  Optimizer state is not carried, as in fm_update."""
    if not isinstance(object, dict) or object.get("class") != "FM":
        raise TypeError("object must be a FM object")
    if not isinstance(cmap, ColumnMap):
        raise TypeError("cmap must be the column map fm_prune_features or fm_hash_features returned")
    if list(object["Scales"]["model.vars"]) != cmap.feature_names:
        raise ValueError("the features of the model are not the same as those the column map was made for")
    src = np.flatnonzero(cmap.carried & (cmap.map != L.COLUMN_DROP))
    dst = cmap.map[src].astype(np.int64)
    if len(np.unique(dst)) != len(dst):
        raise ValueError("the column map sends two occurring features to one id: their model rows cannot be merged")
    mdl = object["Model"]
    w = np.zeros(cmap.new_p)
    v = np.zeros((np.asarray(mdl["v"]).shape[0], cmap.new_p))
    w[dst] = np.asarray(mdl["w"])[src]
    v[:, dst] = np.asarray(mdl["v"])[:, src]
    sc = dict(object["Scales"])
    if sc["mean"] is not None:
        mean, std = np.zeros(cmap.new_p), np.ones(cmap.new_p)
        mean[dst] = np.asarray(sc["mean"])[src]; std[dst] = np.asarray(sc["std"])[src]
        sc["mean"], sc["std"] = mean, std
    sc["model.vars"] = list(cmap.new_feature_names)
    out = dict(object)
    out["Model"] = dict(mdl, w=w, v=v)
    out["Scales"] = sc
    out.pop("Trace", None)   # its snapshots live in the old feature space
    return out


# ---- value binning (include/fmx.h: fmx_matrix_column_quantiles, fmx_matrix_bin_columns) -----------------------------------
class Binning:
    """What fm_bin_features decided, to be applied again (fm_apply_bins: validation and serving data).  columns: the binned columns' old ids,
    ascending; edges: one float32 array per binned column; new_base: uint32[old features + 1], the first new id of every old column; new_p;
    feature_names / new_feature_names: the names before and after ("age[<18.5]", "age[18.5,31)", "age[>=31]", "age[nan]"); unbinned: the new ids
    of the columns left as values, which is what fm_train's normalize= takes."""

    def __init__(self, columns, edges, new_base, feature_names, new_feature_names):
        self.columns, self.edges, self.new_base = columns, edges, new_base
        self.new_p = int(new_base[-1])
        self.feature_names, self.new_feature_names = list(feature_names), list(new_feature_names)
        binned = np.zeros(len(new_base) - 1, bool)
        binned[columns] = True
        self.unbinned = new_base[:-1][~binned].astype(np.int64)


def _bin_names(names, cols, edges):
    """the new feature names: an unbinned column keeps its name, a binned one gets one name per bucket and one for NaN"""
    out, at = [], dict((int(c), e) for c, e in zip(cols, edges))
    for j, name in enumerate(names):
        if j not in at:
            out.append(name)
            continue
        e = [f"{float(x):.6g}" for x in at[j]]
        if not e:
            out.append(f"{name}[all]")
        else:
            out.append(f"{name}[<{e[0]}]")
            out.extend(f"{name}[{a},{b})" for a, b in zip(e[:-1], e[1:]))
            out.append(f"{name}[>={e[-1]}]")
        out.append(f"{name}[nan]")
    return out


def _bin_columns_arg(columns, p):
    cols = np.asarray(columns)
    if cols.ndim != 1 or (cols.size and cols.dtype.kind not in "iu"):
        raise ValueError("columns must be a one-dimensional integer array")
    if cols.size and (int(cols.min()) < 0 or int(cols.max()) >= p):
        raise ValueError(f"columns must lie in 0..{p - 1}")
    cols = np.sort(cols.astype(np.int64))
    if np.any(np.diff(cols) == 0):
        raise ValueError("columns names a column twice")
    return cols


def _bin_edges_arg(edges, col):
    e = np.asarray(edges, np.float64).ravel().astype(np.float32)
    if len(e) > L.BINS_MAX_EDGES or np.any(np.isnan(e)) or np.any(e[1:] <= e[:-1]):
        raise ValueError(f"the edges of column {col} must ascend strictly (in single precision), hold no NaN and at most {L.BINS_MAX_EDGES} values")
    return e


def _binned(m, data, cols, edges, names):
    out, base = m.bin_columns(cols, edges)
    host = _host_matrix(out, data.labels, names)
    out.close()
    return host, base


def fm_bin_features(data, columns, bins=32, method="quantile", edges=None, device=0):
    """Discretise numeric columns into one-hot buckets on the device (include/fmx.h: fmx_matrix_column_quantiles, fmx_matrix_bin_columns;
    DESIGN.md section 28).  An FM sees a numeric feature x only as w x and x <v, .>; binned, every bucket has its own w and v, so a non-monotone
    effect of x can be learned.

    columns: the ids of the columns to bin.  method = "quantile": at most bins - 1 edges per column that cut its stored, non-NaN values into
    bins of equal mass (ties share a bin; no transform of the values is needed first: the bins are the same under any increasing map).  method =
    "width": the edges float32(lo + (hi - lo) b / bins), b = 1 .. bins-1, between the lowest and the highest stored value, repeats dropped.
    edges = {column: array}: the caller's own edges for those columns (ascending strictly, no NaN), the method for the others.  A value x goes
    to bucket #{edges <= x}; NaN goes to a bucket of its own, which exists whether or not the data holds one.  Absent entries stay absent.
    Returns (the new fm.matrix, a Binning for fm_apply_bins)."""
    p = _columns_data(data, "fm_bin_features")
    cols = _bin_columns_arg(columns, p)
    bins = _columns_int("bins", bins, 1, L.BINS_MAX_BINS)
    if method not in ("quantile", "width"):
        raise ValueError(f'method must be "quantile" or "width" (got {method!r})')
    given = {}
    if edges is not None:
        if not isinstance(edges, dict):
            raise TypeError("edges must be a dict of column to array")
        for c, e in edges.items():
            if isinstance(c, (bool, np.bool_)) or not isinstance(c, (int, np.integer)) or int(c) not in cols:
                raise ValueError(f"edges names column {c!r}, which is not one of columns")
            given[int(c)] = _bin_edges_arg(e, int(c))
    m = _device_matrix(data, None, device)
    fit = [int(c) for c in cols if int(c) not in given]
    if fit:
        q_edges, _, rng = m.column_quantiles(fit, bins)
        for s, c in enumerate(fit):
            if method == "quantile":
                given[c] = q_edges[s]
            else:
                lo, hi = np.float64(rng[s, 0]), np.float64(rng[s, 1])
                e = (lo + (hi - lo) * np.arange(1, bins, dtype=np.float64) / bins).astype(np.float32)
                given[c] = np.unique(e[np.isfinite(e)])
    all_edges = [given[int(c)] for c in cols]
    names = _bin_names(data.feature_names, cols, all_edges)
    out, base = _binned(m, data, cols, all_edges, names)
    m.close()
    return out, Binning(cols, all_edges, base, data.feature_names, names)


def fm_apply_bins(data, binning, device=0):
    """The buckets of fm_bin_features on other data with the same features (validation, test and serving data): the same edges and ids.
    Returns the new fm.matrix."""
    p = _columns_data(data, "fm_apply_bins")
    if not isinstance(binning, Binning):
        raise TypeError("binning must be the Binning fm_bin_features returned")
    if p != len(binning.new_base) - 1 or list(data.feature_names) != binning.feature_names:
        raise ValueError("the features in data are not the same as those the binning was made for")
    m = _device_matrix(data, None, device)
    out, _ = _binned(m, data, binning.columns, binning.edges, binning.new_feature_names)
    m.close()
    return out


# ---- feature crosses (include/fmx.h: fmx_matrix_cross) ----------------------------------------------------------------------
class Crossing:
    """What fm_cross_features decided, to be applied again (fm_apply_crosses: validation and serving data).  segment_base: the fields' offsets,
    uint32 from 0 to the old feature count; terms: [(a, b, n_buckets)], n_buckets 0 for exact ids; seed, salt, keep; cross_base: uint32[terms + 1],
    the first new id of every term, cross_base[-1] = new_p; new_segment_base: the segments of the output (with keep: the fields, then one segment
    per term), which is what a second fm_cross_features and fm_prune_features(fields=) take; feature_names / new_feature_names."""

    def __init__(self, segment_base, terms, seed, salt, keep, cross_base, feature_names, new_feature_names):
        self.segment_base, self.terms, self.seed, self.salt, self.keep = segment_base, list(terms), int(seed), int(salt), bool(keep)
        self.cross_base = cross_base
        self.new_p = int(cross_base[-1])
        lead = np.asarray(segment_base, np.int64) if keep else np.zeros(1, np.int64)
        self.new_segment_base = np.concatenate([lead, np.asarray(cross_base[1:], np.int64)]).astype(np.uint32)
        self.feature_names, self.new_feature_names = list(feature_names), list(new_feature_names)


def _cross_names(names, base, terms, keep):
    """the new feature names: the source's (keep), then per exact term "<name_u>:<name_v>" in id order, per hashed term "<a>x<b>#<bucket>" """
    out = list(names) if keep else []
    for a, b, nb in terms:
        if nb:
            out.extend(f"{a}x{b}#{k}" for k in range(nb))
        else:
            right = names[int(base[b]):int(base[b + 1])]
            for u in names[int(base[a]):int(base[a + 1])]:
                out.extend(f"{u}:{v}" for v in right)
    return out


def _crossed(m, data, crossing, names):
    out, cross_base = m.cross(crossing["base"], crossing["terms"], seed=crossing["seed"], salt=crossing["salt"], keep_source=crossing["keep"])
    host = _host_matrix(out, data.labels, names)
    out.close()
    return host, cross_base


def fm_cross_features(data, pairs, fields, buckets=None, seed=0, keep=True, device=0):
    """Cross fields on the device (include/fmx.h: fmx_matrix_cross).  A degree-2 FM gives a pair of features only the
    rank-k term <v_a, v_b>; crossed, the pair is a feature of its own, with its own w and v: a full-rank correction for the field pairs that
    need one (fm_cross_candidates names them), and third-order effects through <v_ab, v_c>.

    fields: the ascending feature offsets of the fields from 0 to the feature count, as fm_prune_features takes them (a dense column is a field
    of width 1).  pairs: a list of (a, b) or (a, b, n_buckets) over field indices, a <= b; a == b crosses a field with itself (a bag of ids:
    every pair of its entries in a row).  A pair without n_buckets takes `buckets`; None or 0 gives exact ids u * width(b) + v, a positive
    count hashes the pair into that many ids.  The value of a crossed entry is the product of the two values.  keep: the source's entries stay in
    front of the crosses.  Returns (the new fm.matrix, a Crossing for fm_apply_crosses)."""
    p = _columns_data(data, "fm_cross_features")
    default = _columns_int("buckets", buckets, 0, 0xFFFFFFFF, none=0)
    if not isinstance(keep, (bool, np.bool_)):
        raise ValueError(f"keep must be True or False (got {keep!r})")
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"seed must be an integer (got {seed!r})")
    try:
        terms = [tuple(t) + ((default,) if len(tuple(t)) == 2 else ()) for t in pairs]
    except TypeError:
        raise ValueError("pairs must be a list of (a, b) or (a, b, n_buckets)") from None
    base, terms, total = Matrix._cross_args(p, fields, terms)
    new_p = total + (p if keep else 0)
    if new_p > 2**31 - 1:
        raise ValueError(f"the crossed matrix would have {new_p} features: a fm.matrix holds at most 2^31 - 1 (hash the widest pairs: buckets=)")
    names = _cross_names(data.feature_names, base, terms, keep)
    m = _device_matrix(data, None, device)
    out, cross_base = _crossed(m, data, dict(base=base, terms=terms, seed=seed, salt=0, keep=bool(keep)), names)
    m.close()
    return out, Crossing(base, terms, seed, 0, keep, cross_base, data.feature_names, names)


def fm_apply_crosses(data, crossing, device=0):
    """The crosses of fm_cross_features on other data with the same features (validation, test and serving data): the same ids.  Returns the
    new fm.matrix."""
    p = _columns_data(data, "fm_apply_crosses")
    if not isinstance(crossing, Crossing):
        raise TypeError("crossing must be the Crossing fm_cross_features returned")
    if p != int(crossing.segment_base[-1]) or list(data.feature_names) != crossing.feature_names:
        raise ValueError("the features in data are not the same as those the crossing was made for")
    m = _device_matrix(data, None, device)
    out, _ = _crossed(m, data, dict(base=crossing.segment_base, terms=crossing.terms, seed=crossing.seed, salt=crossing.salt, keep=crossing.keep),
                      crossing.new_feature_names)
    m.close()
    return out


def fm_cross_candidates(object, newdata, fields, top=8, normalize=True):
    """Which field pairs to cross: the pairs (a, b), a < b, of the fields `fields` (offsets, as in fm_cross_features) ordered by the total
    |interaction| the fitted model gives them on `newdata` -- the abs_sum cell of fm_interactions(..., groups=fields)'s summary --, strongest
    first, at most `top` of them.  Returns a list of (a, b, abs_sum)."""
    top = _columns_int("top", top, 1)
    p = len(object["Model"]["w"])
    base = np.asarray(fields)
    if base.ndim != 1 or len(base) < 2 or base.dtype.kind not in "iu" or base[0] != 0 or base[-1] != p or np.any(np.diff(base.astype(np.int64)) < 0):
        raise ValueError(f"fields must ascend from 0 to the feature count ({p})")
    width = np.diff(base.astype(np.int64))
    groups = np.repeat(np.arange(len(width), dtype=np.int64), width)
    table = fm_interactions(object, newdata, top=1, groups=groups, normalize=normalize)["summary"]["abs_sum"]
    G = len(width)
    cells = [(a, b, float(table[a, b])) for a in range(G) for b in range(a + 1, G)]
    cells.sort(key=lambda c: (-c[2], c[0], c[1]))
    return cells[:top]


# ---- target and count encoding (include/fmx.h: fmx_target_stats, fmx_matrix_encode_targets) -------------------------------------
_ENCODE_KINDS = {"mean": L.ENCODE_MEAN, "count": L.ENCODE_COUNT}
_TARGETS = {"positive": L.TARGET_POSITIVE, "label": L.TARGET_LABEL}


class TargetEncoding:
    """What fm_encode_targets fitted, to be applied again (fm_apply_targets: validation and serving data).  Host arrays only, so it pickles.
    segment_base: the fields' offsets, uint32 from 0 to the old feature count; term_segment: the encoded fields; n_parts, target ("positive" or
    "label"); count int64[W][n_parts][2] and sum float64[W][n_parts] (None under "positive"): the exported table; kinds uint32[terms] (bit 0 mean,
    bit 1 count), prior, strength, keep; enc_base uint32[terms + 1]: the first new id of every term, enc_base[-1] = new_p; new_segment_base: the
    segments of the output (with keep: the fields, then one per encoded field), which fm_bin_features' columns and fm_cross_features take."""

    def __init__(self, segment_base, term_segment, n_parts, target, count, sum, kinds, prior, strength, keep, enc_base, feature_names, new_feature_names):
        self.segment_base, self.term_segment = np.asarray(segment_base, np.uint32), np.asarray(term_segment, np.uint32)
        self.n_parts, self.target, self.count, self.sum = int(n_parts), target, count, sum
        self.kinds, self.prior, self.strength, self.keep = np.asarray(kinds, np.uint32), float(prior), float(strength), bool(keep)
        self.enc_base = np.asarray(enc_base, np.uint32)
        self.new_p = int(self.enc_base[-1])
        lead = self.segment_base.astype(np.int64) if self.keep else np.zeros(1, np.int64)
        self.new_segment_base = np.concatenate([lead, self.enc_base[1:].astype(np.int64)]).astype(np.uint32)
        self.feature_names, self.new_feature_names = list(feature_names), list(new_feature_names)


def _target_names(names, base, encode, kinds, keep):
    """the new feature names: the source's (keep), then per encoded field "te(<field>)" and / or "cnt(<field>)"; <field> is the name of a field of
    one column, the index of a wider one"""
    out = list(names) if keep else []
    for s, k in zip(encode, kinds):
        field = names[int(base[s])] if int(base[s + 1]) - int(base[s]) == 1 else str(int(s))
        if k & L.ENCODE_MEAN:
            out.append(f"te({field})")
        if k & L.ENCODE_COUNT:
            out.append(f"cnt({field})")
    return out


def _target_layout(p, fields, encode):
    base = np.asarray(fields)
    if base.ndim != 1 or not 2 <= len(base) <= L.CROSS_MAX_SEGMENTS + 1 or base.dtype.kind not in "iu" or base[0] != 0 or base[-1] != p \
            or np.any(np.diff(base.astype(np.int64)) < 0):
        raise ValueError(f"fields must ascend from 0 to the feature count ({p}), 2..{L.CROSS_MAX_SEGMENTS + 1} offsets")
    seg = np.asarray(encode)
    if seg.ndim != 1 or not 1 <= len(seg) <= L.TARGET_MAX_TERMS or seg.dtype.kind not in "iu" or int(seg.min()) < 0 or int(seg.max()) >= len(base) - 1 \
            or np.any(np.diff(seg.astype(np.int64)) <= 0):
        raise ValueError(f"encode must hold 1..{L.TARGET_MAX_TERMS} strictly ascending field indices inside 0..{len(base) - 2}")
    return base.astype(np.uint32), seg.astype(np.uint32)


def fm_encode_targets(data, fields, encode, folds=5, by=None, how="rows", kinds=("mean",), strength=20.0, prior=None, target=None, keep=True, seed=0,
                      device=0):
    """Target (mean) and count encoding of high-cardinality fields on the device, out of fold (include/fmx.h: fmx_target_stats,
    fmx_matrix_encode_targets).  Per row and encoded field the matrix gains "mean" -- (a + prior * strength) / (n + strength),
    n and a the rows and the target sum of the id the row carries -- and / or "count" -- n.  Fitted on the rows it is applied to, the mean leaks the
    label; so the rows get folds (fmx_split_assign under by / how, as fm_folds) and a row's n and a leave its own fold out.

    fields: the ascending feature offsets of the fields from 0 to the feature count, as fm_cross_features takes them; encode: the indices of the
    fields to encode, strictly ascending.  kinds: "mean", "count" or both, for every encoded field.  prior None: the mean of [label > 0], or of
    the labels under target "label"; target None: "positive" when every label is -1, 0 or 1, "label" otherwise.  keep: the source's entries stay
    in front of the new columns.  Returns (the new fm.matrix, a TargetEncoding for fm_apply_targets)."""
    p = _columns_data(data, "fm_encode_targets")
    base, seg = _target_layout(p, fields, encode)
    folds = _columns_int("folds", folds, 2, L.TARGET_MAX_PARTS)
    scope, groups, n_groups = _split_groups(data, by, how)
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    if not kinds or len(set(kinds)) != len(kinds) or any(k not in _ENCODE_KINDS for k in kinds):
        raise ValueError(f'kinds must be "mean", "count" or both (got {kinds!r})')
    bits = np.full(len(seg), sum(_ENCODE_KINDS[k] for k in kinds), np.uint32)
    if not isinstance(keep, (bool, np.bool_)):
        raise ValueError(f"keep must be True or False (got {keep!r})")
    seed = _split_int("seed", seed, 0)
    strength = float(strength)
    if not np.isfinite(strength) or strength < 0:
        raise ValueError(f"strength must be finite and not negative (got {strength!r})")
    if data.labels is None:
        raise ValueError("fm_encode_targets needs labels: the data has none")
    y = np.asarray(data.labels, np.float64)
    if target is None:
        target = "positive" if np.all(np.isin(y, (-1.0, 0.0, 1.0))) else "label"
    if target not in _TARGETS:
        raise ValueError(f'target must be "positive", "label" or None (got {target!r})')
    if prior is None:
        prior = np.float64(np.mean(y > 0)) if target == "positive" else np.float64(np.mean(y))
    prior = float(prior)
    if not np.isfinite(prior):
        raise ValueError(f"prior must be finite (got {prior!r})")
    names = _target_names(data.feature_names, base, seg, bits, keep)
    part = split_assign(data.dim[0], groups, n_groups, scope=scope, n_folds=folds, seed=seed, device=device)
    held = []   # the device handles, released on every way out: the table is gigabytes on wide fields
    try:
        m = _device_matrix(data, y, device)
        held.append(m)
        table = m.target_stats(part, base, seg, n_parts=folds, target=_TARGETS[target])
        held.append(table)
        out, enc_base = m.encode_targets(table, part, kinds=bits, prior=prior, strength=strength, keep_source=bool(keep))
        held.append(out)
        count, total = table.export()
        host = _host_matrix(out, data.labels, names)
    finally:
        for h in reversed(held):
            h.close()
    return host, TargetEncoding(base, seg, folds, target, count, total, bits, prior, strength, keep, enc_base, data.feature_names, names)


def fm_apply_targets(data, encoding, device=0):
    """The encoding of fm_encode_targets on other data with the same features (validation, test and serving data): every row is encoded with the
    totals over the folds.  The data needs no labels.  Returns the new fm.matrix."""
    p = _columns_data(data, "fm_apply_targets")
    if not isinstance(encoding, TargetEncoding):
        raise TypeError("encoding must be the TargetEncoding fm_encode_targets returned")
    if p != int(encoding.segment_base[-1]) or list(data.feature_names) != encoding.feature_names:
        raise ValueError("the features in data are not the same as those the encoding was made for")
    from .engine import TargetTable
    held = []
    try:
        table = TargetTable.from_arrays(encoding.segment_base, encoding.term_segment, encoding.count, encoding.sum, target=_TARGETS[encoding.target], device=device)
        held.append(table)
        m = _device_matrix(data, None, device)
        held.append(m)
        out, _ = m.encode_targets(table, None, kinds=encoding.kinds, prior=encoding.prior, strength=encoding.strength, keep_source=encoding.keep)
        held.append(out)
        host = _host_matrix(out, data.labels, encoding.new_feature_names)
    finally:
        for h in reversed(held):
            h.close()
    return host


# ---- matrix composition (include/fmx.h: fmx_matrix_join, fmx_matrix_stack)----------------------------------------------
def _design_ids(name, ids, n, count):
    """an id column of fm_design on the host: int64[n] in 0 .. count-1 (count None: 1 + the largest id); returns (ids, count)"""
    ids = np.asarray(ids)
    if ids.ndim != 1 or (ids.size and not np.issubdtype(ids.dtype, np.integer)):
        raise ValueError(f"{name} must be a one-dimensional integer array")
    if n is not None and len(ids) != n:
        raise ValueError(f"{name} holds {len(ids)} ids, user holds {n}: one interaction per position")
    ids = ids.astype(np.int64)
    if ids.size and int(ids.min()) < 0:
        raise ValueError(f"{name} holds a negative id")
    if count is None:
        count = int(ids.max()) + 1 if ids.size else 0
    elif ids.size and int(ids.max()) >= count:
        raise ValueError(f"{name} holds the id {int(ids.max())}, outside 0..{count - 1}")
    return ids, count


def _design_side(name, features, count, count_name):
    """a side table of fm_design: None or a fm.matrix; returns the row count it fixes"""
    if features is None:
        return count
    if not isinstance(features, FmMatrix):
        raise TypeError(f"{name} must be a fm.matrix object")
    if np.any(np.isnan(features.features["value"])):
        raise ValueError(f"there are NAs in {name}")
    if count is not None and features.dim[0] != count:
        raise ValueError(f"{name} holds {features.dim[0]} rows, {count_name} is {count}: one row per id")
    return features.dim[0]


def fm_design(user, item, labels=None, user_features=None, item_features=None, n_users=None, n_items=None, ids=True, device=0):
    """The FM design of an interaction table with side information, assembled on the device (fmx_matrix_join): interaction t = (user[t],
    item[t], labels[t]) becomes the row [onehot(user) | onehot(item) | U[user] | I[item]], the four blocks in disjoint column ranges.
    user_features / item_features: fm.matrix objects with one row per user / per item (None: no such block); n_users / n_items: the
    vocabularies (None: the side table's rows, else 1 + the largest id); ids=False leaves the two one-hot id blocks out (their ranges are empty).
    Returns {"data": the interactions' rows with `labels`, "context": one row per user [onehot(u) | 0 | U[u] | 0], "items": one row per item
    [0 | onehot(i) | 0 | I[i]], "bases": int64[4], the first column of the four blocks} -- all in one column space, so a model trained on
    `data` is what fm_recommend(fit, context, items), fm_rerank, fm_similar and fm_train_rank(context, items, ...) score and train.  Stored
    values come back as the device holds them (single precision)."""
    user, _ = _design_ids("user", user, None, None)
    n = len(user)
    item, _ = _design_ids("item", item, n, None)
    if labels is not None:
        labels = np.asarray(labels, np.float64)
        if labels.ndim != 1 or len(labels) != n:
            raise ValueError(f"labels must hold one value per interaction ({n})")
        if np.any(np.isnan(labels)):
            raise ValueError("there are NAs in labels")
    for name, v in (("n_users", n_users), ("n_items", n_items)):
        if v is not None:
            _split_int(name, v, 0)
    n_users = _design_side("user_features", user_features, n_users, "n_users")
    n_items = _design_side("item_features", item_features, n_items, "n_items")
    user, n_users = _design_ids("user", user, None, n_users)
    item, n_items = _design_ids("item", item, n, n_items)
    if not ids and user_features is None and item_features is None:
        raise ValueError("nothing to join: ids=False needs user_features or item_features")
    pu = 0 if user_features is None else user_features.dim[1]
    pi = 0 if item_features is None else item_features.dim[1]
    bases = np.concatenate([[0], np.cumsum([n_users if ids else 0, n_items if ids else 0, pu, pi])]).astype(np.int64)
    p = int(bases[4])
    if p > np.iinfo(np.int32).max:
        raise ValueError("fm.matrix keeps col_idx as 32-bit integers: more columns than 2^31 - 1")
    names = ([f"user{u + 1}" for u in range(n_users)] + [f"item{i + 1}" for i in range(n_items)] if ids else []) + \
        ([] if user_features is None else [f"user.{c}" for c in user_features.feature_names]) + \
        ([] if item_features is None else [f"item.{c}" for c in item_features.feature_names])
    mu = None if user_features is None else _device_matrix(user_features, None, device)
    mi = None if item_features is None else _device_matrix(item_features, None, device)
    all_users, all_items = np.arange(n_users, dtype=np.int64), np.arange(n_items, dtype=np.int64)

    def joined(u_rows, i_rows, count):
        blocks = []
        if ids and u_rows is not None:
            blocks.append((n_users, u_rows, int(bases[0])))
        if ids and i_rows is not None:
            blocks.append((n_items, i_rows, int(bases[1])))
        if mu is not None and u_rows is not None:
            blocks.append((mu, u_rows, int(bases[2])))
        if mi is not None and i_rows is not None:
            blocks.append((mi, i_rows, int(bases[3])))
        if not blocks:   # (ids=False and this side has no table: rows without entries)
            return Matrix.from_csr(np.zeros(count + 1, np.int64), np.zeros(0, np.uint32), np.zeros(0, np.float32), p, device=device)
        return Matrix.join(blocks, n=count, p=p, device=device)

    out = {"bases": bases[:4].copy()}
    for key, (u_rows, i_rows, count, y) in (("data", (user, item, n, labels)), ("context", (all_users, None, n_users, None)),
                                            ("items", (None, all_items, n_items, None))):
        m = joined(u_rows, i_rows, count)
        out[key] = _host_matrix(m, y, names)
        m.close()
    for m in (mu, mi):
        if m is not None:
            m.close()
    return out


def fm_stack(parts, device=0):
    """The rows of parts[0], then parts[1], and so on as one fm.matrix, put together on the device (fmx_matrix_stack): what puts the folds of
    fm_folds or the two sides of fm_split back together.  All parts share the feature names; labels iff every part has them."""
    parts = list(parts)
    if not 1 <= len(parts) <= L.STACK_MAX_PARTS:
        raise ValueError(f"fm_stack takes 1 to {L.STACK_MAX_PARTS} parts (got {len(parts)})")
    for k, d in enumerate(parts):
        if not isinstance(d, FmMatrix):
            raise TypeError(f"part {k} must be a fm.matrix object")
        if d.dim[1] != parts[0].dim[1] or list(d.feature_names) != list(parts[0].feature_names):
            raise ValueError(f"part {k}'s features are not the same as part 0's")
    labelled = sum(d.labels is not None for d in parts)
    if labelled not in (0, len(parts)):
        raise ValueError(f"{labelled} of the {len(parts)} parts have labels: all of them or none")
    mats = [_device_matrix(d, None, device) for d in parts]
    m = Matrix.stack(mats)
    labels = np.concatenate([np.asarray(d.labels, np.float64) for d in parts]) if labelled else None
    out = _host_matrix(m, labels, parts[0].feature_names)
    for x in mats + [m]:
        x.close()
    return out
