"""numpy restatement of fold-in (include/fmx.h: fmx_fold_in) and the inputs its tests share.

For a fold feature u and a row r that stores u exactly once, with value x,
    y(r) = b_r + <z_r, theta_u>,   theta_u = (w_u, v_u),   z_r = x (keep_w1, t_r),   t_r = sum_{j != u} x_j v_j,
b_r the forward of the row without that entry.  Squared loss: (Z'Z + Lambda) theta = Z'(y - b).  Logistic loss (labels +-1): n_newton full
Newton steps from theta = 0,  sigma = 1 / (1 + exp(-y y^)),  g = sum -y (1 - sigma) z + Lambda theta,  H = sum sigma (1 - sigma) z z' + Lambda,
theta -= H^-1 g.  With keep_w1 = 0, w_u is not a variable and stays 0.

Everything takes the dtype as a parameter, so the same code runs in float64 and in np.longdouble (numpy's linalg does not: the Cholesky
solve below is written out)."""
import functools

import numpy as np

SQUARED, LOGISTIC = "squared", "logistic"

ROW_CHUNK = 256   # FI_CHUNK of fmwr_amd/csrc/fm_foldin.hip: rows per (group, chunk) workgroup; ROW_CHUNK +- 1 are in the list already
GROUP_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2 * ROW_CHUNK - 1, 2 * ROW_CHUNK, 2 * ROW_CHUNK + 1, 1000, 5000]
KS = [0, 1, 2, 15, 16, 17, 32, 33, 64]
N_ITEMS, N_SIDE = 200, 50


def chol_solve(H, rhs):
    """x with H x = rhs through H = L L' in H's dtype; None when a pivot is not positive or not finite."""
    D = len(rhs)
    A = H.copy()
    diag = np.zeros(D, H.dtype)
    for j in range(D):
        piv = A[j, j]
        if not (piv > 0 and np.isfinite(piv)):
            return None
        l = np.sqrt(piv)
        diag[j] = l
        A[j + 1:, j] = A[j + 1:, j] / l
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    x = rhs.copy()
    for j in range(D):
        x[j] = x[j] / diag[j]
        x[j + 1:] -= A[j + 1:, j] * x[j]
    for j in range(D - 1, -1, -1):
        x[j] = x[j] / diag[j]
        x[:j] -= A[j, :j] * x[j]
    return x


def rows_of(rp, col, val, ids, w0, w, v, k0, k1, dtype):
    """(rows, group, b, z): the participating rows ascending, each one's index into ids, b_r and z_r [1 + k] in `dtype`.  Raises ValueError
    when a row stores two entries of the fold features."""
    n, p, k = len(rp) - 1, len(w), v.shape[0]
    slot = np.full(p, -1, np.int64)
    slot[np.asarray(ids, np.int64)] = np.arange(len(ids))
    row = np.repeat(np.arange(n), np.diff(rp))
    fold = slot[col] >= 0
    cnt = np.bincount(row[fold], minlength=n)
    if np.any(cnt > 1):
        raise ValueError("a row stores more than one entry of the fold features")
    x = val.astype(dtype)
    keep = ~fold
    T = v.T.astype(dtype)[col[keep]] * x[keep][:, None]          # [entries][k], walked in entry order
    S = np.zeros((n, k), dtype); Q = np.zeros((n, k), dtype); lin = np.zeros(n, dtype)
    np.add.at(S, row[keep], T)
    np.add.at(Q, row[keep], T * T)
    np.add.at(lin, row[keep], w.astype(dtype)[col[keep]] * x[keep])
    b = (dtype(w0) if k0 else dtype(0)) + (lin if k1 else 0) + dtype(0.5) * (S * S - Q).sum(1)
    rows = row[fold]                                              # ascending: one fold entry per participating row
    xu = x[fold]
    z = xu[:, None] * np.concatenate([np.full((len(rows), 1), 1 if k1 else 0, dtype), S[rows]], axis=1)
    return rows, slot[col[fold]], b[rows], z


def solve_group(z, b, y, lw, lv, k1, loss, n_newton, dtype, first_steps=None):
    """theta [1 + k] of one group from its rows (in the order given), or None on a failed pivot; first_steps: a list that receives theta
    after every Newton step."""
    D = z.shape[1]
    lam = np.full(D, lv, dtype); lam[0] = lw
    theta = np.zeros(D, dtype)
    y = y.astype(dtype)
    for _ in range(n_newton if loss == LOGISTIC else 1):
        yh = b + z @ theta
        if loss == LOGISTIC:
            sg = 1 / (1 + np.exp(-y * yh))
            c, d = sg * (1 - sg), y * (1 - sg)
        else:
            c, d = np.ones(len(y), dtype), y - yh
        zc = z * c[:, None]
        H = np.zeros((D, D), dtype)
        for i0 in range(0, D, 8):   # the upper triangle in strips of 8 rows (longdouble products are slow), mirrored
            H[i0:i0 + 8, i0:] = zc[:, i0:i0 + 8].T @ z[:, i0:]
        H = np.triu(H) + np.triu(H, 1).T + np.diag(lam)
        rhs = z.T @ d - lam * theta
        if not k1:
            H[0, :] = 0; H[:, 0] = 0; H[0, 0] = 1; rhs[0] = 0
        step = chol_solve(H, rhs)
        if step is None:
            return None
        theta = theta + step
        if first_steps is not None:
            first_steps.append(theta.copy())
    return theta


def fold_in(rp, col, val, y, ids, w0, w, v, lw, lv, k0=1, k1=1, loss=SQUARED, n_newton=8, dtype=np.float64, perm_seed=None):
    """(theta [n_ids][1 + k] with NaN rows where the solve failed, rows int64[n_ids], status int32[n_ids]); perm_seed: each group's rows in a
    random order instead of ascending (the spread of the model itself)."""
    rows, grp, b, z = rows_of(rp, col, val, ids, w0, w, v, k0, k1, dtype)
    D = 1 + v.shape[0]
    theta = np.zeros((len(ids), D), dtype); cnt = np.zeros(len(ids), np.int64); status = np.zeros(len(ids), np.int32)
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None
    for g in range(len(ids)):
        R = np.flatnonzero(grp == g)
        cnt[g] = len(R)
        if rng is not None:
            R = rng.permutation(R)
        t = solve_group(z[R], b[R], np.asarray(y)[rows[R]], dtype(lw), dtype(lv), k1, loss, n_newton, dtype)
        if t is None:
            theta[g] = np.nan; status[g] = 1
        else:
            theta[g] = t
    return theta, cnt, status


def gradient(rp, col, val, y, ids, theta, yhat, w0, w, v, lw, lv, k0=1, k1=1, loss=SQUARED):
    """max |d objective / d theta_u| over the fold features, the objective halved for the squared loss (sum (y - y^)^2 / 2 + theta' Lambda
    theta / 2), from predictions `yhat` of the full model WITH theta written back: d y^ / d theta_u = z_r exactly."""
    rows, grp, _, z = rows_of(rp, col, val, ids, w0, w, v, k0, k1, np.float64)
    D = z.shape[1]
    lam = np.full(D, lv); lam[0] = lw
    yy, yh = np.asarray(y, np.float64)[rows], yhat[rows]
    mult = -(yy - yh) if loss == SQUARED else -yy * (1 - 1 / (1 + np.exp(-yy * yh)))
    worst = 0.0
    for g in range(len(ids)):
        R = grp == g
        gvec = z[R].T @ mult[R] + lam * theta[g]
        if not k1:
            gvec[0] = 0
        worst = max(worst, float(np.max(np.abs(gvec))))
    return worst


def rel_err(got, ref):
    """largest |got - ref| over a feature's theta relative to that feature's max |theta| (1 where theta is all zero)"""
    ref = np.asarray(ref, np.longdouble)
    scale = np.max(np.abs(ref), axis=1)
    scale = np.where(scale > 0, scale, 1)
    return float(np.max(np.max(np.abs(np.asarray(got, np.longdouble) - ref), axis=1) / scale))


# ------------------------------------------------------------------------------------------------------------ shared inputs

@functools.lru_cache(maxsize=None)
def inputs(valued, sizes=tuple(GROUP_SIZES), seed=0):
    """The GPU test's rows: N_ITEMS item columns, N_SIDE side columns, one fold column per group.  Each row holds one item (value 1), two side
    features with values in [0.5, 1.5] and one fold entry (one-hot, or valued in [0.5, 1.5]); the groups' rows are interleaved, and a
    hundred rows without a fold feature are mixed in.  Returns a dict: rp, col, val, p, ids, sizes."""
    rng = np.random.default_rng(1000 + seed + int(valued))
    G = len(sizes)
    p = N_ITEMS + N_SIDE + G
    grp = np.concatenate([np.repeat(np.arange(G), sizes), np.full(100, -1)])
    grp = grp[rng.permutation(len(grp))]
    n = len(grp)
    col, val, lens = [], [], []
    for r in range(n):
        side = np.sort(rng.choice(N_SIDE, 2, replace=False)) + N_ITEMS
        c = [rng.integers(0, N_ITEMS), side[0], side[1]]
        x = [1.0, rng.uniform(0.5, 1.5), rng.uniform(0.5, 1.5)]
        if grp[r] >= 0:
            c.append(N_ITEMS + N_SIDE + grp[r])
            x.append(rng.uniform(0.5, 1.5) if valued else 1.0)
        col += c; val += x; lens.append(len(c))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return {"rp": rp, "col": np.asarray(col, np.uint32), "val": np.asarray(val, np.float32), "p": p, "n": n,
            "ids": np.arange(N_ITEMS + N_SIDE, p, dtype=np.uint32), "sizes": np.asarray(sizes, np.int64)}


@functools.lru_cache(maxsize=None)
def model_params(p, k, seed=0):
    """(w0, w[p], v[k][p]): V ~ N(0, 0.3), w ~ N(0, 0.1), every value exactly representable in float32 (both table types hold it exactly)"""
    rng = np.random.default_rng(77 + 31 * k + seed)
    w0 = float(np.float32(rng.normal(0, 0.1)))
    w = rng.normal(0, 0.1, p).astype(np.float32).astype(np.float64)
    v = rng.normal(0, 0.3, (k, p)).astype(np.float32).astype(np.float64)
    return w0, w, v


@functools.lru_cache(maxsize=None)
def targets(valued, k, loss, seed=0):
    """float32 labels of inputs(valued): planted -- the model's own prediction with a planted theta for every fold feature, plus noise
    (squared) or thresholded with label noise (logistic).  The logistic label noise is small (scale 0.3) on purpose: the specified iteration
    is the UNDAMPED Newton step from theta = 0, and on groups of about 1 + k rows (nearly separable whatever the labels) noisier labels
    make it need more than eight steps, or overshoot and diverge (scale 1 and 3 were tried with three seeds each: gradients of 1e-10 up to
    4e+1 after eight steps); with these labels it converges on every group, gradient <= 3e-13 after eight steps."""
    inp = inputs(valued)
    w0, w, v = model_params(inp["p"], k)
    rng = np.random.default_rng(501 + k + seed)
    rows, grp, b, z = rows_of(inp["rp"], inp["col"], inp["val"], inp["ids"], w0, w, v, 1, 1, np.float64)
    planted = np.concatenate([rng.normal(0, 0.1, (len(inp["ids"]), 1)), rng.normal(0, 0.3, (len(inp["ids"]), k))], axis=1)
    score = np.zeros(inp["n"])
    score[rows] = b + np.einsum("ij,ij->i", z, planted[grp])
    if loss == SQUARED:
        return (score + rng.normal(0, 0.2, inp["n"])).astype(np.float32)
    y = np.where(score + rng.logistic(0, 0.3, inp["n"]) > 0, 1.0, -1.0)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(valued, k, loss, lw=0.1, lv=0.1, k0=1, k1=1, n_newton=8):
    """the np.longdouble model on inputs(valued) / model_params / targets: (theta, rows, status), computed once per process"""
    inp = inputs(valued)
    w0, w, v = model_params(inp["p"], k)
    y = targets(valued, k, loss)
    return fold_in(inp["rp"], inp["col"], inp["val"], y, inp["ids"], w0, w, v, lw, lv, k0, k1, loss, n_newton, np.longdouble)


@functools.lru_cache(maxsize=None)
def spread(valued, k, loss, n_newton=8):
    """the model's own fp64 spread on these inputs: the float64 model with every group's rows permuted against the longdouble model"""
    inp = inputs(valued)
    w0, w, v = model_params(inp["p"], k)
    y = targets(valued, k, loss)
    t64, _, st = fold_in(inp["rp"], inp["col"], inp["val"], y, inp["ids"], w0, w, v, 0.1, 0.1, 1, 1, loss, n_newton, np.float64, perm_seed=k + 1)
    ref, _, rst = reference(valued, k, loss, n_newton=n_newton)
    assert not st.any() and not rst.any()
    return rel_err(t64, ref)
