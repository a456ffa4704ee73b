"""fmx_interactions / fmx_interactions_device / fmx_interactions_summary / fm_interactions: the top_m strongest pair terms of every row, bit for bit
against the numpy model of the definition (tests/interactions_model.py) in both kernel forms and on their boundaries, the identities that tie the
pair values to fmx_contrib and to the oracle's forward, and the group summary against exactly rounded sums."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import oracle
from tests import interactions_model as im

pytestmark = pytest.mark.gpu

KINDS = ["seq64", "mb32", "mb32_wir", "mb64"]
E_W, E_T = 32, 32     # the library's default limits (fm_interactions.hip: IX_EW, IX_ET)
U = 2.0 ** -53


def _engine(kind, p, k, monkeypatch, k0=1, k1=1, seed=0, nan_col=None, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    common = dict(num_factor=k, task=L.TASK_REGRESSION, keep_w0=k0, keep_w1=k1, **kw)
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, **common)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), **common)
    rng = np.random.default_rng(seed + 7 * k + 1)
    v = rng.normal(0, 0.4, (k, p))
    if nan_col is not None:
        v[:, nan_col] = np.nan
    e.set_params(0.3, rng.normal(0, 0.5, p), v)
    return e


def _mat(m, p):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _limits(wave=0, tile=0, rows=0):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_interactions_limits(wave, tile, rows))


def _csr(rows):
    """CSR from a list of (cols, vals)"""
    rp = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    col = np.concatenate([np.asarray(c, np.uint32) for c, _ in rows]) if rp[-1] else np.zeros(0, np.uint32)
    val = np.concatenate([np.asarray(x, np.float32) for _, x in rows]) if rp[-1] else np.zeros(0, np.float32)
    return rp, col.astype(np.uint32), val.astype(np.float32)


def _random_rows(lens, p, rng):
    return [(rng.integers(0, p, n), rng.normal(0, 1, n).astype(np.float32)) for n in lens]


def _same(got, ref, what=""):
    """a, b and the value's bits"""
    assert np.array_equal(got[0], ref[0]), (what, "a")
    assert np.array_equal(got[1], ref[1]), (what, "b")
    assert np.array_equal(im.bits(got[2]), im.bits(ref[2])), (what, "value bits")


P_EDGE, NAN_COL = 50, 49


def _edge_rows(rng):
    """every row length around E_w = E_t = 8, a column stored twice, two pairs of equal magnitude and opposite sign, a NaN table row"""
    rows = _random_rows([0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 25], NAN_COL, rng)   # columns 0 .. 48: column 49's factors are NaN
    c, x = _random_rows([6], NAN_COL, rng)[0]
    c[4] = c[1]                                      # one column twice: two players
    rows.append((c, x))
    for n in (5, 12):                                # (a1, d) and (a2, d) have I of equal magnitude and opposite sign, for every d
        c, x = _random_rows([n], NAN_COL, rng)[0]
        c[3], x[3] = c[0], -x[0]
        rows.append((c, x))
    for n in (4, 11):                                # a NaN factor row: its pairs come last, in (a, b) order
        c, x = _random_rows([n], NAN_COL, rng)[0]
        c[2] = NAN_COL
        rows.append((c, x))
    return rows


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [0, 1, 3, 16, 17, 64, 100])
def test_top_m_bit_for_bit_in_both_forms(kind, k, monkeypatch):
    rng = np.random.default_rng(300 + k)
    m = _csr(_edge_rows(rng))
    e = _engine(kind, P_EDGE, k, monkeypatch, nan_col=NAN_COL)
    mat = _mat(m, P_EDGE)
    _, _, v = e.get_params()
    ref = im.top_m(v, m[0], m[1], m[2], 64)
    if k:
        assert np.isnan(ref[2][-1][45:55]).all() and not np.isnan(ref[2][-1][:45]).any()   # 11 entries: the 10 NaN pairs come after the 45 numbers
    assert np.any(ref[0][:, -1] == -1) and np.any(ref[0][:, -1] >= 0)        # rows with fewer pairs than slots, and with more
    for top in (1, 2, 63, 64):
        _limits(8, 8)          # rows of up to 8 entries: the wave form; 9 .. 25: the workgroup form in tiles of 8
        _same(e.interactions(mat, top), [r[:, :top] for r in ref], (kind, k, top))


def test_default_limits_on_their_boundaries(monkeypatch):
    rng = np.random.default_rng(17)
    p, k = 400, 16
    m = _csr(_random_rows([E_W - 1, E_W, E_W + 1, 2 * E_T + 1, 0, 30], p, rng))
    e = _engine("mb32", p, k, monkeypatch)
    _, _, v = e.get_params()
    ref = im.top_m(v, m[0], m[1], m[2], 64)
    mat = _mat(m, p)
    _same(e.interactions(mat, 64), ref)
    _same(e.interactions(mat, 5), [r[:, :5] for r in ref])


def _hip():
    import os
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library is not loadable")


def _device_slice(e, mat, r0, r1, top):
    """fmx_interactions_device for rows [r0, r1) into buffers of the HIP runtime's own, copied back"""
    hip = _hip()
    cnt = max((r1 - r0) * top, 1)
    bufs = [ctypes.c_void_p() for _ in range(3)]
    out = [np.empty((r1 - r0, top), np.int64), np.empty((r1 - r0, top), np.int64), np.empty((r1 - r0, top), np.float64)]
    for d in bufs:
        assert hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(cnt * 8)) == 0
    try:
        e.interactions_device(mat, r0, r1, top, bufs[0].value, bufs[1].value, bufs[2].value)
        e.sync()
        for d, h in zip(bufs, out):
            if h.size:
                assert hip.hipMemcpy(h.ctypes.data_as(ctypes.c_void_p), d, ctypes.c_size_t(h.size * 8), 2) == 0   # hipMemcpyDeviceToHost
    finally:
        for d in bufs:
            hip.hipFree(d)
    return out


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_forms_ranges_slices_and_prefixes_give_the_same_bits(kind, monkeypatch):
    rng = np.random.default_rng(23)
    p, k, top = 300, 20, 7
    lens = list(rng.integers(0, E_W + 1, 60)) + [E_W, 2, 0, E_W - 1]
    rows = _random_rows(lens, p, rng)
    m = _csr(rows)
    e = _engine(kind, p, k, monkeypatch)
    mat = _mat(m, p)
    wave = e.interactions(mat, top)                    # every row has at most E_w entries: the wave form
    for tile in (8, E_T):
        _limits(1, tile)                               # every row with a pair: the workgroup form
        _same(e.interactions(mat, top), wave, ("workgroup form", tile))
    n = len(lens)
    cuts = [0, 1, 2, 5, 6, 33, n - 1, n]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        _same(_device_slice(e, mat, r0, r1, top), [w[r0:r1] for w in wave], ("range", r0, r1))
    _limits(1, 8)
    _same(_device_slice(e, mat, 3, 40, top), [w[3:40] for w in wave], "range, workgroup form")
    sub = rng.permutation(n)[:25]
    _same(e.interactions(_mat(_csr([rows[r] for r in sub]), p), top), [w[sub] for w in wave], "slice")
    for small in (1, 3):
        _same(e.interactions(mat, small), [w[:, :small] for w in wave], "prefix")
    big = e.interactions(mat, 64)
    _same([b[:, :top] for b in big], wave, "prefix of 64")
    _same(_device_slice(e, mat, 0, 0, top), [w[0:0] for w in wave], "empty range")


def _oracle_raw(e, m, p):
    w0, w, v = e.get_params()
    P = oracle.params(task=oracle.REGRESSION, k=e.k, k0=bool(e.cfg.keep_w0), k1=bool(e.cfg.keep_w1))
    return oracle.predict_batch(P, oracle.Matrix(m[0], m[1], m[2], p), w0, w, v.ravel())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k0,k1", [(1, 1), (0, 1), (1, 0)])
def test_identities_with_the_contributions_and_the_forward(kind, k0, k1, monkeypatch):
    rng = np.random.default_rng(31)
    p, k = 200, 16
    lens = list(rng.integers(0, 12, 80)) + [11, 11]     # at most 11 entries: 55 pairs, top_m = 64 lists every one
    m = _csr(_random_rows(lens, p, rng))
    rp = m[0]
    e = _engine(kind, p, k, monkeypatch, k0, k1)
    mat = _mat(m, p)
    a, b, val = e.interactions(mat, 64)
    phi = e.contrib(mat)
    w0, w, _ = e.get_params()
    lin = k1 * m[2].astype(np.float64) * w[m[1]]
    yhat = _oracle_raw(e, m, p)
    for r in range(len(lens)):
        n, sl = lens[r], slice(rp[r], rp[r + 1])
        full = a[r] >= 0
        assert full.sum() == n * (n - 1) // 2 and np.all(full[:full.sum()])
        per = np.zeros(n)
        np.add.at(per, a[r][full], val[r][full])
        np.add.at(per, b[r][full], val[r][full])
        rmax = np.abs(phi[sl]).max() if n else 0.0
        err = np.abs(per - 2 * (phi[sl] - lin[sl]))
        assert np.all(err <= 2 * 1e-12 * (1 + rmax)), (r, err.max() if n else 0)
        got = k0 * w0 + lin[sl].sum() + val[r][full].sum()
        assert abs(got - yhat[r]) <= 1e-10 * (1 + abs(yhat[r])), (r, got, yhat[r])


def _check_summary(got, ref, what=""):
    """counts exact, symmetric tables, every value within N_cell * 2^-53 * abs_sum of the exactly rounded sum of the model's pair values"""
    assert np.array_equal(got["count"], ref["count"]), what
    bar = ref["count"] * U * ref["abs_sum"]
    for key in ("sum", "abs_sum"):
        assert np.array_equal(got[key], got[key].T), (what, key)
        err = np.abs(got[key] - ref[key])
        print(what, key, "max error", err.max(), "over bar", np.max(err / np.where(bar > 0, bar, 1.0)))
        assert np.all(err <= bar), (what, key, err.max())
    assert np.array_equal(got["count"], got["count"].T), what


def _summary_case(e, m, p, groups, G):
    mat = _mat(m, p)
    _, _, v = e.get_params()
    ref = im.summary(v, m[0], m[1], m[2], groups, G)
    s = e.interactions_summary(mat, groups, G)
    _check_summary(s, ref, "default cut")
    s2 = e.interactions_summary(mat, groups, G)
    for key in ("sum", "abs_sum", "count"):
        assert np.array_equal(im.bits(s[key]) if key != "count" else s[key], im.bits(s2[key]) if key != "count" else s2[key]), key
    _limits(0, 0, 7)                                  # the next summary: 7 rows per workgroup
    _check_summary(e.interactions_summary(mat, groups, G), ref, "7 rows per workgroup")
    s4 = e.interactions_summary(mat, groups, G)     # one-shot: the default cut again
    assert np.array_equal(im.bits(s4["sum"]), im.bits(s["sum"]))
    return s, ref


@pytest.mark.parametrize("kind", ["seq64", "mb32", "mb32_wir"])
def test_summary_on_one_hot_fields_finds_the_planted_pair(kind, monkeypatch):
    p, groups, v, rp, col, val = im.planted(np.random.default_rng(2))
    e = _engine(kind, p, v.shape[0], monkeypatch)
    e.set_params(0.1, np.zeros(p), v)
    s, _ = _summary_case(e, (rp, col, val), p, groups, 6)
    iu = np.triu_indices(6)
    best = np.argmax(s["abs_sum"][iu])
    assert (iu[0][best], iu[1][best]) == (1, 4)
    a, b, _ = e.interactions(_mat((rp, col, val), p), 1)
    assert np.all(a[:, 0] == 1) and np.all(b[:, 0] == 4)


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
@pytest.mark.parametrize("k", [0, 3, 16])
def test_summary_on_ragged_rows_with_repeated_groups(kind, k, monkeypatch):
    rng = np.random.default_rng(41 + k)
    p, G = 40, 5
    lens = list(rng.integers(0, 30, 40)) + [300, 1, 0, 2]   # 300 entries: two tiles of the summary, every tile pair form
    m = _csr(_random_rows(lens, p, rng))
    groups = rng.integers(0, G, p).astype(np.uint32)
    e = _engine(kind, p, k, monkeypatch)
    _summary_case(e, m, p, groups, G)
    # every feature its own group: the identity map, p <= 64
    _, _, v = e.get_params()
    short = _csr(_random_rows(list(rng.integers(0, 12, 30)), p, rng))
    _check_summary(e.interactions_summary(_mat(short, p), None, 64), im.summary(v, short[0], short[1], short[2], None, 64), "identity map")


def test_refusals_leave_the_outputs_alone(monkeypatch):
    from fmwr_amd import _lib as L
    rng = np.random.default_rng(1)
    p = 70
    m = _csr(_random_rows([3, 4, 5], p, rng))
    e = _engine("mb32", p, 4, monkeypatch)
    mat, other = _mat(m, p), _mat(_csr(_random_rows([3], p + 1, rng)), p + 1)
    idx = np.full((3, 64), 7, np.int64)
    out = np.full((64, 64), 7.0)
    pi, po = idx.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    groups = (np.arange(p) % 3).astype(np.uint32)
    pg = groups.ctypes.data_as(ctypes.c_void_p)
    lib = L.lib()
    calls = [
        lambda: lib.fmx_interactions(e.h, mat.h, 0, pi, pi, po),
        lambda: lib.fmx_interactions(e.h, mat.h, 65, pi, pi, po),
        lambda: lib.fmx_interactions(e.h, other.h, 2, pi, pi, po),
        lambda: lib.fmx_interactions(e.h, None, 2, pi, pi, po),
        lambda: lib.fmx_interactions(e.h, mat.h, 2, pi, None, po),
        lambda: lib.fmx_interactions(e.h, mat.h, 2, pi, pi, None),
        lambda: lib.fmx_interactions_device(e.h, mat.h, 0, 1, 0, pi, pi, po),
        lambda: lib.fmx_interactions_device(e.h, mat.h, 2, 1, 2, pi, pi, po),
        lambda: lib.fmx_interactions_device(e.h, mat.h, -1, 1, 2, pi, pi, po),
        lambda: lib.fmx_interactions_device(e.h, mat.h, 0, 4, 2, pi, pi, po),
        lambda: lib.fmx_interactions_device(e.h, mat.h, 0, 1, 2, None, pi, po),
        lambda: lib.fmx_interactions_summary(e.h, mat.h, pg, 0, po, po, pi),
        lambda: lib.fmx_interactions_summary(e.h, mat.h, pg, 65, po, po, pi),
        lambda: lib.fmx_interactions_summary(e.h, mat.h, pg, 2, po, po, pi),       # a group id 2 with 2 groups
        lambda: lib.fmx_interactions_summary(e.h, mat.h, None, 64, po, po, pi),    # the identity map needs p <= n_groups
        lambda: lib.fmx_interactions_summary(e.h, other.h, pg, 3, po, po, pi),
        lambda: lib.fmx_interactions_summary(e.h, mat.h, pg, 3, None, po, pi),
    ]
    for i, call in enumerate(calls):
        assert call() == L.ERR_INVALID, i
        assert lib.fmx_last_error().decode(), i
    assert np.all(idx == 7) and np.all(out == 7.0)
    # an empty matrix and an empty range are fine and write nothing; count may be NULL
    empty = _mat(_csr([]), p)
    assert lib.fmx_interactions(e.h, empty.h, 2, None, None, None) == L.OK
    assert lib.fmx_interactions_summary(e.h, empty.h, pg, 3, po, po, None) == L.OK
    assert lib.fmx_interactions_device(e.h, mat.h, 1, 1, 2, None, None, None) == L.OK
    assert np.all(out == 7.0)
    assert lib.fmx_interactions_summary(e.h, mat.h, pg, 3, po, po, None) == L.OK
    assert out.ravel()[9] == 7.0 and not np.all(out.ravel()[:9] == 7.0)


def test_parameters_are_not_modified_and_a_multi_gpu_engine_reads_its_primary_replica(monkeypatch):
    rng = np.random.default_rng(4)
    p, k = 100, 16
    m = _csr(_random_rows(list(rng.integers(0, 20, 50)), p, rng))
    e = _engine("mb32", p, k, monkeypatch, n_gpus=2, gpus_share_device=1)
    before = e.get_params()
    _same(e.interactions(_mat(m, p), 4), im.top_m(before[2], m[0], m[1], m[2], 4))
    e.interactions_summary(_mat(m, p), (np.arange(p) % 8).astype(np.uint32), 8)
    after = e.get_params()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and np.array_equal(before[2], after[2])


def test_fm_interactions_end_to_end():
    import fmwr_amd as fm
    rng = np.random.default_rng(13)
    n, p = 300, 40
    X = sp.random(n, p, density=0.2, random_state=3, format="csr")
    X.data = rng.normal(0, 1, X.nnz)
    X.sort_indices()
    y = np.where(rng.random(n) < 0.5, 0.0, 1.0)
    fit = fm.fm_train(fm.fm_matrix(X, y), normalize=False, seed=1,
                      control=[fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=2000, solver=fm.SGD_solver())])
    groups = np.arange(p) % 4
    out = fm.fm_interactions(fit, fm.fm_matrix(X), top=3, groups=groups, normalize=False)
    v = np.asarray(fit["Model"]["v"], np.float64).reshape(4, p)
    rp, col, val = X.indptr.astype(np.int64), X.indices.astype(np.uint32), X.data.astype(np.float32)
    a, b, I = im.top_m(v, rp, col, val, 3)
    row, slot = np.nonzero(a >= 0)
    assert np.array_equal(out["row"], row)
    assert np.array_equal(out["feature_a"], col[rp[row] + a[row, slot]]) and np.array_equal(out["feature_b"], col[rp[row] + b[row, slot]])
    assert np.array_equal(im.bits(out["value"]), im.bits(I[row, slot]))
    ref = im.summary(v, rp, col, val, groups, 4)
    _check_summary(out["summary"], ref, "fm_interactions")
    assert np.array_equal(out["summary"]["importance"], out["summary"]["abs_sum"] / np.maximum(out["summary"]["count"], 1))
    plain = fm.fm_interactions(fit, fm.fm_matrix(X), top=3, normalize=False)
    assert "summary" not in plain and np.array_equal(im.bits(plain["value"]), im.bits(out["value"]))
