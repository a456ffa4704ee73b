"""numpy restatement of the pairwise fold-in (include/fmx.h: fmx_fold_in_pairs) and the inputs its tests share.

m is a pair matrix: rows 2t and 2t + 1 are pair t, row 2t the preferred one.  Per row, b_r (WITHOUT w0: it cancels) and z_r are those of
tests/foldin_model.py; a row without a fold entry has b_r = its whole forward and z_r = 0 (set, not multiplied).  A pair takes part if one of
its rows stores a fold feature u, its group (two different ones: ValueError), with B_t = b_2t - b_2t+1, Z_t = z_2t - z_2t+1, and theta_u
comes from foldin_model.solve_group's logistic loop with every label +1.  Everything takes the dtype as a parameter."""
import functools

import numpy as np

from tests import foldin_model as M

KS = M.KS
GROUP_SIZES = M.GROUP_SIZES   # in PAIRS: the Gram chunk's boundaries
N_ITEMS, N_SIDE = M.N_ITEMS, M.N_SIDE


def row_terms(rp, col, val, ids, w, v, k1, dtype):
    """(grp int64[n]: the row's index into ids or -1, b [n], z [n][1 + k]) of EVERY row, in `dtype`; w0 takes no part"""
    n, p, k = len(rp) - 1, len(w), v.shape[0]
    slot = np.full(p, -1, np.int64)
    slot[np.asarray(ids, np.int64)] = np.arange(len(ids))
    row = np.repeat(np.arange(n), np.diff(rp))
    fold = slot[col] >= 0
    if np.any(np.bincount(row[fold], minlength=n) > 1):
        raise ValueError("a row stores more than one entry of the fold features")
    x = val.astype(dtype)
    keep = ~fold
    T = v.T.astype(dtype)[col[keep]] * x[keep][:, None]
    S = np.zeros((n, k), dtype); Q = np.zeros((n, k), dtype); lin = np.zeros(n, dtype)
    np.add.at(S, row[keep], T)
    np.add.at(Q, row[keep], T * T)
    np.add.at(lin, row[keep], w.astype(dtype)[col[keep]] * x[keep])
    b = (lin if k1 else 0) + dtype(0.5) * (S * S - Q).sum(1)
    grp = np.full(n, -1, np.int64)
    rows = row[fold]
    grp[rows] = slot[col[fold]]
    z = np.zeros((n, 1 + k), dtype)                                  # rows without a fold entry: zero by construction
    z[rows, 0] = x[fold] if k1 else 0
    z[rows, 1:] = x[fold][:, None] * S[rows]
    return grp, b, z


def pairs_of(rp, col, val, ids, w, v, k1, dtype):
    """(pairs ascending, group, B, Z [.][1 + k]) of the participating pairs"""
    grp, b, z = row_terms(rp, col, val, ids, w, v, k1, dtype)
    ga, gb = grp[0::2], grp[1::2]
    if np.any((ga >= 0) & (gb >= 0) & (ga != gb)):
        raise ValueError("the two rows of a pair store different fold features")
    pg = np.where(ga >= 0, ga, gb)
    T = np.flatnonzero(pg >= 0)
    return T, pg[T], (b[0::2] - b[1::2])[T], (z[0::2] - z[1::2])[T]


def fold_in_pairs(rp, col, val, ids, w, v, lw, lv, k1=1, n_newton=8, dtype=np.float64, perm_seed=None):
    """(theta [n_ids][1 + k] with NaN rows where the solve failed, pairs int64[n_ids], status int32[n_ids]); perm_seed: each group's pairs in a
    random order instead of ascending (the spread of the model itself)."""
    if (len(rp) - 1) % 2:
        raise ValueError("a pair matrix has an even row count")
    T, grp, B, Z = pairs_of(rp, col, val, ids, w, v, k1, dtype)
    D = 1 + v.shape[0]
    theta = np.zeros((len(ids), D), dtype); cnt = np.zeros(len(ids), np.int64); status = np.zeros(len(ids), np.int32)
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None
    for g in range(len(ids)):
        R = np.flatnonzero(grp == g)
        cnt[g] = len(R)
        if rng is not None:
            R = rng.permutation(R)
        t = M.solve_group(Z[R], B[R], np.ones(len(R)), dtype(lw), dtype(lv), k1, M.LOGISTIC, n_newton, dtype)
        if t is None:
            theta[g] = np.nan; status[g] = 1
        else:
            theta[g] = t
    return theta, cnt, status


def gradient(rp, col, val, ids, theta, yhat, w, v, lw, lv, k1=1):
    """max |d objective / d theta_u| over the fold features, objective = sum log(1 + exp(-d_t)) + theta' Lambda theta / 2, from the forward
    `yhat` of the pair rows under the full model WITH theta written back: d_t = yhat[2t] - yhat[2t + 1], d d_t / d theta_u = Z_t exactly."""
    T, grp, _, Z = pairs_of(rp, col, val, ids, w, v, k1, np.float64)
    D = Z.shape[1]
    lam = np.full(D, lv); lam[0] = lw
    d = yhat[2 * T] - yhat[2 * T + 1]
    mult = -1 / (1 + np.exp(d))
    worst = 0.0
    for g in range(len(ids)):
        R = grp == g
        gvec = Z[R].T @ mult[R] + lam * theta[g]
        if not k1:
            gvec[0] = 0
        worst = max(worst, float(np.max(np.abs(gvec))))
    return worst


# ------------------------------------------------------------------------------------------------------------ shared inputs

FORMS = ("U", "V", "P", "N")


def user_like(g):
    """groups alternate: even ones hold a new user's pairs (the fold entry in both rows), odd ones a new item's (in one row)"""
    return g % 2 == 0


# The ridge weight of every (k, valued) case: 0.1 unless the model itself says otherwise.  The specified iteration is eight UNDAMPED Newton
# steps from theta = 0, and on user-like groups of about 1 + k pairs with 64 factors they have not settled at lambda = 0.1 (the float64
# model on these inputs: gradient 3e-10 for the valued matrix, 1e-12 for the one-hot one, against <= 3e-14 at every other k; the fp64 spread
# stays <= 4e-15 throughout).  k = 64 therefore runs at lambda = 1, where eight steps converge (gradient 2e-14).
# tests/test_foldin_pairs_cpu.py asserts the gradient and the spread of every case under this rule.
def case_lambda(k, valued):
    return 1.0 if k == 64 else 0.1


@functools.lru_cache(maxsize=None)
def _base(valued, sizes, seed):
    """the pairs before their orientation is planted: per pair the two rows' (columns, values) and the form"""
    rng = np.random.default_rng(2000 + seed + int(valued))
    G = len(sizes)
    grp = np.concatenate([np.repeat(np.arange(G), sizes), np.full(100, -1)])
    grp = grp[rng.permutation(len(grp))]
    rows = []

    def plain():
        side = np.sort(rng.choice(N_SIDE, 2, replace=False)) + N_ITEMS
        return [int(rng.integers(0, N_ITEMS)), int(side[0]), int(side[1])], [1.0, float(rng.uniform(0.5, 1.5)), float(rng.uniform(0.5, 1.5))]

    def with_fold(cx, g, x):
        at = int(rng.integers(0, 4))                                 # the fold entry sits anywhere in the row
        c, vals = list(cx[0]), list(cx[1])
        c.insert(at, N_ITEMS + N_SIDE + g); vals.insert(at, x)
        return c, vals

    for g in grp:
        a, b = plain(), plain()
        if g >= 0 and user_like(g):
            xa = float(rng.uniform(0.5, 1.5)) if valued else 1.0
            xb = float(rng.uniform(0.5, 1.5)) if valued else xa      # V: different values; U: equal ones
            a, b = with_fold(a, g, xa), with_fold(b, g, xb)
        elif g >= 0:
            a = with_fold(a, g, float(rng.uniform(0.5, 1.5)) if valued else 1.0)   # P as built; N once the planted order swaps the rows
        rows.append((a, b))
    return grp, rows


@functools.lru_cache(maxsize=None)
def inputs(valued, k, sizes=tuple(GROUP_SIZES), seed=0):
    """The GPU test's pair matrix: N_ITEMS item columns, N_SIDE side columns, one fold column per group.  Every row holds one item (value 1)
    and two side features with values in [0.5, 1.5]; the groups' pairs are interleaved, with a hundred pairs without any fold feature mixed
    in.  Which row of a pair is preferred is planted: the sign of d_t under a planted theta (model_params(p, k)'s model) plus logistic noise
    of scale 0.3 -- so the matrix depends on k.  Returns a dict: rp, col, val, p, n, ids, sizes, forms (per pair: U, V, P, N or '-')."""
    grp, rows = _base(valued, sizes, seed)
    G = len(sizes)
    p = N_ITEMS + N_SIDE + G
    ids = np.arange(N_ITEMS + N_SIDE, p, dtype=np.uint32)
    w0, w, v = M.model_params(p, k)

    def assemble(order):
        col, val, lens = [], [], []
        for (a, b), swap in zip(rows, order):
            for c, x in ((b, a) if swap else (a, b)):
                col += c; val += x; lens.append(len(c))
        return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.asarray(col, np.uint32), np.asarray(val, np.float32)

    rp, col, val = assemble(np.zeros(len(rows), bool))
    rng = np.random.default_rng(601 + k + seed)
    planted = np.concatenate([rng.normal(0, 0.1, (G, 1)), rng.normal(0, 0.3, (G, k))], axis=1)
    T, pg, B, Z = pairs_of(rp, col, val, ids, w, v, 1, np.float64)
    swap = np.zeros(len(rows), bool)
    swap[T] = B + np.einsum("ij,ij->i", Z, planted[pg]) + rng.logistic(0, 0.3, len(T)) < 0
    rp, col, val = assemble(swap)
    forms = []
    for g, s in zip(grp, swap):
        forms.append("-" if g < 0 else ("V" if valued else "U") if user_like(g) else ("N" if s else "P"))
    return {"rp": rp, "col": col, "val": val, "p": p, "n": 2 * len(rows), "ids": ids, "sizes": np.asarray(sizes, np.int64), "forms": np.asarray(forms),
            "pair_group": grp}


@functools.lru_cache(maxsize=None)
def reference(valued, k, lw=None, lv=None, k1=1, n_newton=8):
    """the np.longdouble model on inputs(valued, k) / model_params: (theta, pairs, status), computed once per process"""
    inp = inputs(valued, k)
    _, w, v = M.model_params(inp["p"], k)
    lam = case_lambda(k, valued)
    return fold_in_pairs(inp["rp"], inp["col"], inp["val"], inp["ids"], w, v, lam if lw is None else lw, lam if lv is None else lv, k1, n_newton,
                         np.longdouble)


@functools.lru_cache(maxsize=None)
def spread(valued, k, n_newton=8):
    """the model's own fp64 spread on these inputs: the float64 model with every group's pairs permuted against the longdouble model"""
    inp = inputs(valued, k)
    _, w, v = M.model_params(inp["p"], k)
    lam = case_lambda(k, valued)
    t64, _, st = fold_in_pairs(inp["rp"], inp["col"], inp["val"], inp["ids"], w, v, lam, lam, 1, n_newton, np.float64, perm_seed=k + 1)
    ref, _, rst = reference(valued, k, n_newton=n_newton)
    assert not st.any() and not rst.any()
    return M.rel_err(t64, ref)


# ------------------------------------------------------------------------------------------------------------ the cold-start problem

CS_ITEMS, CS_USERS, CS_K, CS_TRAIN, CS_HELD, CS_NEG = 300, 40, 8, 12, 4, 4


@functools.lru_cache(maxsize=None)
def cold_start(seed=0):
    """A planted recommender: CS_ITEMS one-hot items with rows V ~ N(0, 0.3), w ~ N(0, 0.1) (float32-exact), CS_USERS new one-hot users
    (columns CS_ITEMS ..) with planted theta ~ N(0, 0.6) whose rows in the model are ZERO; each user's 16 best items under the planted score
    + Gumbel(0.3) noise: 12 training positives and 4 held out.  Returns a dict: p, w, v (k x p), train / held (users x items index arrays)."""
    rng = np.random.default_rng(9000 + seed)
    p = CS_ITEMS + CS_USERS
    w = np.zeros(p); v = np.zeros((CS_K, p))
    w[:CS_ITEMS] = rng.normal(0, 0.1, CS_ITEMS).astype(np.float32)
    v[:, :CS_ITEMS] = rng.normal(0, 0.3, (CS_K, CS_ITEMS)).astype(np.float32)
    theta = rng.normal(0, 0.6, (CS_USERS, CS_K))
    score = w[:CS_ITEMS][None, :] + theta @ v[:, :CS_ITEMS] + rng.gumbel(0, 0.3, (CS_USERS, CS_ITEMS))
    best = np.argsort(-score, axis=1)[:, :CS_TRAIN + CS_HELD]
    best = np.stack([rng.permutation(r) for r in best])
    return {"p": p, "w": w, "v": v, "train": np.sort(best[:, :CS_TRAIN], axis=1), "held": np.sort(best[:, CS_TRAIN:], axis=1)}


def cold_start_pairs(cs, seed=0):
    """numpy-sampled pairs of the cold-start problem, as fmx_matrix_pairs forms them: for every (user, training positive), CS_NEG negatives
    drawn uniformly from the user's non-positives; rows 2t = user + positive, 2t + 1 = user + negative (one-hot, user entry first)"""
    rng = np.random.default_rng(77 + seed)
    col = []
    for u in range(CS_USERS):
        others = np.setdiff1d(np.arange(CS_ITEMS), cs["train"][u])
        for i in cs["train"][u]:
            for j in rng.choice(others, CS_NEG, replace=False):
                col += [CS_ITEMS + u, i, CS_ITEMS + u, j]
    col = np.asarray(col, np.uint32)
    return np.arange(0, len(col) + 1, 2, dtype=np.int64), col, np.ones(len(col), np.float32)


def cold_start_auc(cs, w, v):
    """held-out AUC with the training positives excluded: over users and their held-out items, the share of the user's other eligible items
    (neither training positives nor held out) that score below the held-out item (ties count 1/2)"""
    users = CS_ITEMS + np.arange(CS_USERS)
    score = w[:CS_ITEMS][None, :] + v[:, users].T @ v[:, :CS_ITEMS]
    total = []
    for u in range(CS_USERS):
        rest = np.setdiff1d(np.arange(CS_ITEMS), np.concatenate([cs["train"][u], cs["held"][u]]))
        for h in cs["held"][u]:
            total.append(np.mean(score[u, rest] < score[u, h]) + 0.5 * np.mean(score[u, rest] == score[u, h]))
    return float(np.mean(total))
