"""fmx_matrix_pairs_hard / Matrix.pairs_hard / fm_train_rank(n_candidates=...) (hard negatives): n_cand = 1 is the
uniform sampler bit for bit; the chosen negatives equal a numpy restatement of the draws, the shuffle and fmx_topk's order on fmx_topk's own
scores; ties go to the lower index and NaN below every number; the invariants; the refusals; and training with hard negatives reaching a
higher held-out recall than the uniform sampler on the planted problem of test_gpu_rank.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

KINDS = ["mb64", "mb32", "mb32_wir"]


def _L():
    from fmwr_amd import _lib as L
    return L


def _engine(kind, p, k, monkeypatch, seed=7, nan_feature=None, copies=()):
    """a ranking engine with random nonzero w0, w and V; copies: (feature, source feature) pairs whose w and V column are set equal"""
    from fmwr_amd import engine
    L = _L()
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    e = engine.Engine(p, task=L.TASK_RANKING, solver=L.SOLVER_SGD, num_factor=k, mode=L.MODE_MINIBATCH, state_fp64=int(kind == "mb64"),
                      batch_rows=64)
    rng = np.random.default_rng(seed)
    w, v = rng.normal(0, 0.5, p), rng.normal(0, 0.4, (k, p))
    for f, src in copies:
        w[f] = w[src]; v[:, f] = v[:, src]
    if nan_feature is not None:
        w[nan_feature] = np.nan
    e.set_params(0.7, w, v)
    return e


def _csr(rows, vals):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    col = np.concatenate([np.asarray(r, np.int64) for r in rows]).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    val = np.concatenate([np.asarray(x, np.float32) for x in vals]).astype(np.float32) if rp[-1] else np.zeros(0, np.float32)
    return rp, col, val


def _problem(n_ctx, n_items, rng, extra=6, ties=None, nan_items=()):
    """context c holds feature c (value 1) and some of `extra` shared features; item i holds its own feature n_ctx + extra + i (value 1) and
    some of 3 shared item features -- so every exported row names its context and item.  ties: {copy: source}: the copy holds the source's
    shared entries (the engine gives its own feature the source's parameters: the same scores, bit for bit).  nan_items: hold feature p - 1
    (the engine's NaN w) after their own."""
    p = n_ctx + extra + n_items + 3 + 1
    crows, cvals, irows, ivals = [], [], [], []
    for c in range(n_ctx):
        sh = sorted(rng.choice(extra, rng.integers(0, extra + 1), replace=False) + n_ctx)
        crows.append([c] + sh); cvals.append([1.0] + list(rng.normal(0, 1, len(sh))))
    for i in range(n_items):
        sh = sorted(rng.choice(3, rng.integers(0, 3), replace=False) + n_ctx + extra + n_items)
        irows.append([n_ctx + extra + i] + sh); ivals.append([1.0] + list(rng.normal(0, 1, len(sh))))
    for i, src in (ties or {}).items():
        irows[i] = [n_ctx + extra + i] + irows[src][1:]; ivals[i] = list(ivals[src])
    for i in nan_items:
        irows[i] = [n_ctx + extra + i, p - 1]; ivals[i] = [1.0, 1.0]
    return p, _csr(crows, cvals), _csr(irows, ivals)


def _dev(m, p):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _pos(lists, n_items):
    from fmwr_amd import engine
    rp, col, _ = _csr(lists, [np.ones(len(x)) for x in lists])
    return engine.Matrix.from_csr(rp, col, np.ones(len(col), np.float32), n_items)


def _parse(pm, n_ctx, extra, C_, I_):
    """the (context, item) of every exported row, each row checked against the context's and the item's entries"""
    rp, col, val, y = pm.export()
    out = []
    for r in range(pm.n):
        cc, vv = col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]
        c = int(cc[0])
        lc = int(C_[0][c + 1] - C_[0][c])
        assert np.array_equal(cc[:lc], C_[1][C_[0][c]:C_[0][c + 1]]) and np.array_equal(vv[:lc], C_[2][C_[0][c]:C_[0][c + 1]])
        it = int(cc[lc]) - n_ctx - extra
        assert np.array_equal(cc[lc:], I_[1][I_[0][it]:I_[0][it + 1]]) and np.array_equal(vv[lc:], I_[2][I_[0][it]:I_[0][it + 1]])
        out.append((c, it))
    assert np.all(y == 1.0)
    return out


def _triples(pm, n_ctx, extra, C_, I_):
    rows = _parse(pm, n_ctx, extra, C_, I_)
    assert all(rows[2 * s][0] == rows[2 * s + 1][0] for s in range(pm.n // 2))
    return [(rows[2 * s][0], rows[2 * s][1], rows[2 * s + 1][1]) for s in range(pm.n // 2)]


# ------------------------------------------------------------------------------------------------ numpy restatement of the sampler
def _mix64(x):
    x = x ^ (x >> np.uint64(30)); x = x * np.uint64(0xBF58476D1CE4E5B9)
    x = x ^ (x >> np.uint64(27)); x = x * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _pair_hash(seed, epoch, t, stream):
    """fm_pairs.hip's pair_hash over the uint64 array t"""
    with np.errstate(over="ignore"):
        h = _mix64(np.array([seed], np.uint64) + np.uint64(0x9E3779B97F4A7C15))
        h = _mix64(h ^ (np.array([epoch], np.uint64) * np.uint64(0xD6E8FEB86659FD93) + np.uint64(stream)))
        return _mix64(h ^ (t + np.uint64(0x632BE59BD9B4E019)))


def _mulhi(a, b):
    """the high 64 bits of the 128-bit products a * b (uint64 arrays)"""
    m32 = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    al, ah, bl, bh = a & m32, a >> s32, b & m32, b >> s32
    with np.errstate(over="ignore"):
        p0, p1, p2, p3 = al * bl, al * bh, ah * bl, ah * bh
        mid = (p0 >> s32) + (p1 & m32) + (p2 & m32)
        return p3 + (p1 >> s32) + (p2 >> s32) + (mid >> s32)


def _before(sa, ja, sb, jb):
    """fmx_topk's order: (sa, ja) before (sb, jb)?"""
    an, bn = np.isnan(sa), np.isnan(sb)
    if an != bn:
        return bool(bn)
    if not an and sa != sb:
        return bool(sa > sb)
    return ja < jb


def _expected(lists, n_items, n_neg, n_cand, seed, epoch, S):
    """the (c, i, j) sequence of fmx_matrix_pairs_hard from its definition, scores S[c, j]; also the uniform negatives, in output order"""
    keys = sorted({(c, int(i)) for c, l in enumerate(lists) for i in l})
    P = [np.array(sorted({int(i) for i in l}), np.int64) for l in lists]
    T = len(keys) * n_neg
    t = np.arange(T, dtype=np.uint64)
    pc = np.array([keys[x // n_neg][0] for x in range(T)], np.int64)
    pi = np.array([keys[x // n_neg][1] for x in range(T)], np.int64)
    avail = np.array([n_items - len(P[c]) for c in pc], np.uint64)
    cand = np.empty((T, n_cand), np.int64)
    for q in range(n_cand):
        r = _mulhi(_pair_hash(seed, epoch, t, 0 if q == 0 else q + 1), avail)
        for x in range(T):
            Pc = P[pc[x]]
            rr = int(r[x])
            cand[x, q] = rr + int(np.searchsorted(Pc - np.arange(len(Pc)), rr, side="right"))  # the r-th non-positive
    best = cand[:, 0].copy()
    for x in range(T):
        for q in range(1, n_cand):
            j = cand[x, q]
            if _before(S[pc[x], j], j, S[pc[x], best[x]], best[x]):
                best[x] = j
    order = np.argsort(_pair_hash(seed, epoch, t, 1), kind="stable")
    return [(int(pc[o]), int(pi[o]), int(best[o])) for o in order], [int(cand[o, 0]) for o in order], cand[order]


def _scores(e, cm, im, n_ctx, n_items):
    """S[c, j]: fmx_topk's raw scores of every pair (K = n_items)"""
    idx, sc = e.topk(cm, im, n_items)
    S = np.full((n_ctx, n_items), np.nan)
    for c in range(n_ctx):
        assert np.all(idx[c] >= 0)
        S[c, idx[c]] = sc[c]
    return S


def _lists(n_ctx, n_items, rng, most=12):
    lists = [list(rng.integers(0, n_items, rng.integers(1, most))) for _ in range(n_ctx)]
    lists[1] = []                                                      # no positive: no pair
    lists[2] = [5, 5, 9, 5, 9]                                         # duplicates count once
    lists[3] = [i for i in range(n_items) if i != 17]                  # all items but one: every negative is item 17
    return lists


def _export_equal(a, b):
    return a.n == b.n and a.nnz == b.nnz and all(np.array_equal(x, y) for x, y in zip(a.export(), b.export()))


# ------------------------------------------------------------------------------------------------ 1. n_cand = 1 is the uniform sampler
@pytest.mark.parametrize("kind", KINDS)
def test_one_candidate_gives_the_uniform_bits(kind, monkeypatch):
    from fmwr_amd import engine
    rng = np.random.default_rng(1)
    n_ctx, n_items = 30, 120
    p, C_, I_ = _problem(n_ctx, n_items, rng)
    e = _engine(kind, p, 12, monkeypatch)
    cm, im, xm = _dev(C_, p), _dev(I_, p), _pos(_lists(n_ctx, n_items, rng), n_items)
    for seed in (0, 5, 2**63 + 11):
        for epoch in (0, 3):
            for n_neg in (1, 3):
                u = engine.Matrix.pairs(cm, im, xm, n_neg, seed, epoch)
                h = engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, 1, seed, epoch)
                assert u.n > 0 and _export_equal(u, h), (seed, epoch, n_neg)


# ------------------------------------------------------------------------------------------------ 2. the exact choice
@pytest.mark.parametrize("kind", KINDS)
def test_exact_choice_matches_numpy(kind, monkeypatch):
    from fmwr_amd import engine
    rng = np.random.default_rng(2)
    n_ctx, n_items, extra, n_neg, seed, epoch = 40, 300, 6, 2, 123456789, 4
    p, C_, I_ = _problem(n_ctx, n_items, rng, extra)
    e = _engine(kind, p, 12, monkeypatch)
    lists = _lists(n_ctx, n_items, rng)
    cm, im, xm = _dev(C_, p), _dev(I_, p), _pos(lists, n_items)
    S = _scores(e, cm, im, n_ctx, n_items)
    for n_cand in (2, 7, 64):
        pm = engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, n_cand, seed, epoch)
        got = _triples(pm, n_ctx, extra, C_, I_)
        want, uniform, _ = _expected(lists, n_items, n_neg, n_cand, seed, epoch, S)
        assert got == want, n_cand
        free = [(j, u) for (c, _, j), u in zip(got, uniform) if c != 3]
        assert sum(1 for j, u in free if j != u) > len(free) // 4   # many choices are not the uniform draw
        assert all(j == 17 for c, _, j in got if c == 3)
        assert not any(c == 1 for c, _, _ in got)


# ------------------------------------------------------------------------------------------------ 3. ties and NaN
@pytest.mark.parametrize("kind", KINDS)
def test_ties_go_to_the_lower_index_and_nan_is_never_chosen_over_a_number(kind, monkeypatch):
    """Items 10..14 copy item 3's shared entries and their own feature carries item 3's parameters (the copies must stay distinguishable in
    the exported rows), so the six score alike bit for bit; items 15 and 16 hold the feature whose w is NaN."""
    from fmwr_amd import engine
    rng = np.random.default_rng(3)
    n_ctx, n_items, extra, n_neg, seed, epoch = 12, 40, 6, 3, 99, 1
    ties = {i: 3 for i in range(10, 15)}
    p, C_, I_ = _problem(n_ctx, n_items, rng, extra, ties=ties, nan_items=(15, 16))
    base = n_ctx + extra
    e = _engine(kind, p, 12, monkeypatch, nan_feature=p - 1, copies=[(base + i, base + 3) for i in ties])
    tied, nan = [3, 10, 11, 12, 13, 14], [15, 16]
    lists = [list(rng.integers(0, n_items, 6)) for _ in range(n_ctx)]
    for c in (0, 1, 2):      # non-positives: the tied items and one NaN item
        lists[c] = [i for i in range(n_items) if i not in tied + [15]]
    for c in (3, 4):         # non-positives: the NaN items alone
        lists[c] = [i for i in range(n_items) if i not in nan]
    for c in (5, 6):         # non-positives: two tied items, both NaN items
        lists[c] = [i for i in range(n_items) if i not in (11, 13, 15, 16)]
    cm, im, xm = _dev(C_, p), _dev(I_, p), _pos(lists, n_items)
    S = _scores(e, cm, im, n_ctx, n_items)
    assert np.all(np.isnan(S[:, nan])) and not np.any(np.isnan(np.delete(S, nan, axis=1)))
    assert all(S[c, i].tobytes() == S[c, 3].tobytes() for c in range(n_ctx) for i in tied)
    for n_cand in (2, 5, 16):
        pm = engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, n_cand, seed, epoch)
        got = _triples(pm, n_ctx, extra, C_, I_)
        want, _, cands = _expected(lists, n_items, n_neg, n_cand, seed, epoch, S)
        assert got == want, n_cand
        for (c, _, j), cand in zip(got, cands):
            drawn = set(int(x) for x in cand)
            numeric = [x for x in drawn if not np.isnan(S[c, x])]
            if numeric:
                assert not np.isnan(S[c, j])                               # a NaN score is never chosen over a number
            if c in (0, 1, 2, 5, 6) and numeric:
                assert j == min(numeric)                                   # tied candidates: the lowest index
            if not numeric:
                assert j == min(drawn)                                     # NaN only: the lowest index


# ------------------------------------------------------------------------------------------------ 4. invariants
@pytest.mark.parametrize("kind", KINDS)
def test_invariants(kind, monkeypatch):
    from fmwr_amd import engine
    L = _L()
    rng = np.random.default_rng(4)
    n_ctx, n_items, extra, n_neg, n_cand, seed, epoch = 40, 250, 6, 2, 8, 17, 2
    p, C_, I_ = _problem(n_ctx, n_items, rng, extra)
    e = _engine(kind, p, 12, monkeypatch)
    lists = _lists(n_ctx, n_items, rng)
    cm, im, xm = _dev(C_, p), _dev(I_, p), _pos(lists, n_items)
    before = e.get_params()
    u = engine.Matrix.pairs(cm, im, xm, n_neg, seed, epoch)
    h = engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, n_cand, seed, epoch)
    after = e.get_params()
    assert after[0] == before[0] and after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()
    S = _scores(e, cm, im, n_ctx, n_items)
    tu, th = _triples(u, n_ctx, extra, C_, I_), _triples(h, n_ctx, extra, C_, I_)
    assert len(tu) == len(th) > 0
    for (c, i, ju), (c2, i2, jh) in zip(tu, th):
        assert (c, i) == (c2, i2) and jh not in set(lists[c])
        assert jh == ju or _before(S[c, jh], jh, S[c, ju], ju)      # never after the uniform negative
    # rows 2s: the uniform sampler's bits
    ru, rh = u.export(), h.export()
    for s in range(h.n // 2):
        a0, a1, b0, b1 = ru[0][2 * s], ru[0][2 * s + 1], rh[0][2 * s], rh[0][2 * s + 1]
        assert a1 - a0 == b1 - b0 and np.array_equal(ru[1][a0:a1], rh[1][b0:b1]) and np.array_equal(ru[2][a0:a1], rh[2][b0:b1])
    # the same inputs: the same bits; chunks of 1 and 3 contexts: the same bits
    assert _export_equal(h, engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, n_cand, seed, epoch))
    for chunk in (1, 3):
        assert L.lib().fmx_debug_pairs_hard_chunk(C.c_int64(chunk)) == L.OK
        assert _export_equal(h, engine.Matrix.pairs_hard(e, cm, im, xm, n_neg, n_cand, seed, epoch)), chunk


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_leave_out_null_and_the_parameters_untouched(monkeypatch):
    from fmwr_amd import engine
    L = _L()
    lib = L.lib()
    rng = np.random.default_rng(5)
    n_ctx, n_items = 8, 30
    p, C_, I_ = _problem(n_ctx, n_items, rng)
    e = _engine("mb32", p, 8, monkeypatch)
    e_p = _engine("mb32", p + 1, 8, monkeypatch)                           # p differs from the matrices'
    lists = _lists(n_ctx, n_items, rng)
    cm, im, xm = _dev(C_, p), _dev(I_, p), _pos(lists, n_items)
    full = _pos([list(range(n_items))] + lists[1:], n_items)               # context 0 holds every item
    short = _pos(lists[:-1], n_items)
    before = [x.get_params() for x in (e, e_p)]   # (fmx_topk's factor limit lies above the engines' 128 factors)
    calls = [(None, cm, im, xm, 1, 8, 0), (e, cm, im, xm, 1, 0, 0), (e, cm, im, xm, 1, 65, 0), (e, cm, im, xm, 1, -3, 0),
             (e_p, cm, im, xm, 1, 8, 0), (e, cm, im, xm, 0, 8, 0),
             (e, cm, im, xm, 1, 8, -1), (e, cm, im, short, 1, 8, 0), (e, cm, im, full, 1, 8, 0), (e, None, im, xm, 1, 8, 0),
             (e, cm, im, None, 1, 8, 0)]
    for q, (eng, c_, i_, x_, n_neg, n_cand, epoch) in enumerate(calls):
        out = C.c_void_p(4242)
        st = lib.fmx_matrix_pairs_hard(eng.h if eng is not None else None, c_.h if c_ is not None else None, i_.h, x_.h if x_ is not None else None,
                                       n_neg, n_cand, 3, epoch, C.byref(out))
        assert st == L.ERR_INVALID, (q, lib.fmx_last_error().decode())
        assert out.value is None and lib.fmx_last_error().decode(), q
    for x, b in zip((e, e_p), before):
        a = x.get_params()
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    # the engine still samples afterwards
    assert engine.Matrix.pairs_hard(e, cm, im, xm, 1, 8, 3, 0).n > 0


# ------------------------------------------------------------------------------------------------ 6. it learns better
def _planted(n_users=2000, n_items=500, k=8, top=20, held=2, seed=11):
    """users and items with planted factors and an item bias; positives = each user's `top` best items, `held` of them held out
    (test_gpu_rank.py's problem, copied)"""
    rng = np.random.default_rng(seed)
    U = rng.normal(0, 1, (n_users, k)); W = rng.normal(0, 1, (n_items, k)); b = rng.normal(0, 1.0, n_items)
    S = U @ W.T + b[None, :]
    best = np.argsort(-S, axis=1)[:, :top]
    train, test = [], []
    for u in range(n_users):
        sel = rng.permutation(top)
        test.append(list(best[u, sel[:held]])); train.append(list(best[u, sel[held:]]))
    import fmwr_amd as fm
    p = n_users + n_items
    ctx = sp.csr_matrix((np.ones(n_users), (np.arange(n_users), np.arange(n_users))), shape=(n_users, p))
    its = sp.csr_matrix((np.ones(n_items), (np.arange(n_items), n_users + np.arange(n_items))), shape=(n_items, p))
    return fm.fm_matrix(ctx), fm.fm_matrix(its), train, test


def test_hard_negatives_learn_a_planted_order_better():
    """Held-out recall@10 (training positives excluded) after 30 epochs, uniform negatives against the best of 8 candidates, everything else
    as test_fm_train_rank_learns_a_planted_order trains.  Margins from the issue: hard >= uniform + 0.05 and hard >= 0.80."""
    import fmwr_amd as fm
    context, items, train, test = _planted()
    ctl = [fm.model_control("RANK", **{"factor.number": 16, "v.init_stdev": 0.1}), fm.solver_control(solver=fm.SGD_solver(learn_rate=0.1))]
    recall = {}
    for n_cand in (1, 8):
        fit = fm.fm_train_rank(context, items, train, control=ctl, n_neg=2, epochs=30, seed=3, batch_rows=4096, n_candidates=n_cand)
        assert fit["rank"]["n_candidates"] == n_cand
        recall[n_cand] = fm.fm_recommend_metrics(fit, context, items, test, k=10, exclude=train, normalize=False)["recall@10"]
    print("held-out recall@10: uniform", recall[1], "hard (n_cand 8)", recall[8])
    assert recall[8] >= recall[1] + 0.05
    assert recall[8] >= 0.80
