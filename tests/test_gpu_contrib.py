"""fmx_contrib / fmx_contrib_device / fmx_contrib_summary / fm_explain: the exact Shapley value of every stored entry for the raw score, checked
against a numpy evaluation of the closed form, against the oracle's forward (efficiency), and against Shapley values enumerated from the
oracle's scores of every sub-row."""
import ctypes
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp

import oracle

pytestmark = pytest.mark.gpu

KINDS = ["seq64", "mb32", "mb32_wir", "mb64"]


def _engine(kind, p, k, monkeypatch, k0=1, k1=1, seed=0, **kw):
    from fmwr_amd import _lib as L, engine
    monkeypatch.setenv("FMX_W_IN_ROW", "1" if kind == "mb32_wir" else "0")
    common = dict(num_factor=k, task=L.TASK_REGRESSION, keep_w0=k0, keep_w1=k1, **kw)
    if kind == "seq64":
        e = engine.Engine(p, mode=L.MODE_SEQUENTIAL, **common)
    else:
        e = engine.Engine(p, mode=L.MODE_MINIBATCH, batch_rows=256, state_fp64=int(kind == "mb64"), **common)
    rng = np.random.default_rng(seed + 7 * k + 1)
    e.set_params(0.3, rng.normal(0, 0.5, p), rng.normal(0, 0.4, (k, p)))
    return e


def _rows(lens, p, rng, dup=True):
    """CSR with the given row lengths; columns drawn with replacement (dup) or distinct, normal values"""
    cols = [rng.integers(0, p, n) if dup else rng.choice(p, n, replace=False) for n in lens]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate(cols).astype(np.uint32) if rp[-1] else np.zeros(0, np.uint32)
    val = rng.normal(0, 1, len(col)).astype(np.float32)
    return rp, col, val


def _mat(m, p):
    from fmwr_amd import engine
    return engine.Matrix.from_csr(m[0], m[1], m[2], p)


def _closed_form(e, m):
    """phi of every entry in fp64 numpy from the engine's stored parameters, and each entry's row max |phi|"""
    rp, col, val = m
    _, w, v = e.get_params()
    k1 = e.cfg.keep_w1
    x = val.astype(np.float64)
    row = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    T = v.T[col] * x[:, None]                       # [nnz][k]
    S = np.zeros((len(rp) - 1, v.shape[0]))
    np.add.at(S, row, T)
    phi = (k1 * x * w[col] if k1 else np.zeros(len(x))) + 0.5 * (T * (S[row] - T)).sum(1)
    rmax = np.zeros(len(rp) - 1)
    np.maximum.at(rmax, row, np.abs(phi))
    return phi, rmax[row]


def _oracle_raw(e, m, p):
    w0, w, v = e.get_params()
    P = oracle.params(task=oracle.REGRESSION, k=e.k, k0=bool(e.cfg.keep_w0), k1=bool(e.cfg.keep_w1))
    return oracle.predict_batch(P, oracle.Matrix(m[0], m[1], m[2], p), w0, w, v.ravel())


def _row_sums(phi, rp):
    return np.add.reduceat(np.concatenate([phi, [0.0]]), rp[:-1]) * (np.diff(rp) > 0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k", [0, 1, 3, 8, 16, 64, 100])
def test_closed_form_and_efficiency(kind, k, monkeypatch):
    rng = np.random.default_rng(100 + k)
    p = 3000
    lens = [0, 1, 2, 2100, 0] + list(rng.integers(0, 40, 40)) + [1, 3000]
    m = _rows(lens, p, rng)
    for k0, k1 in ((1, 1), (0, 1), (1, 0)):
        e = _engine(kind, p, k, monkeypatch, k0, k1)
        phi = e.contrib(_mat(m, p))
        ref, rmax = _closed_form(e, m)
        assert phi.shape == ref.shape
        assert np.all(np.abs(phi - ref) <= 1e-12 * (1 + rmax)), (k0, k1, np.max(np.abs(phi - ref)))
        yhat = _oracle_raw(e, m, p)
        got = (e.get_w0() if k0 else 0.0) + _row_sums(phi, m[0])
        assert np.all(np.abs(got - yhat) <= 1e-10 * (1 + np.abs(yhat))), (k0, k1, np.max(np.abs(got - yhat)))


def _shapley(e, cols, vals, p):
    """Shapley values of a row's entries from the oracle's raw scores of all 2^n sub-rows"""
    n = len(cols)
    masks = np.arange(1 << n)
    inc = (masks[:, None] >> np.arange(n)[None, :]) & 1
    rp = np.concatenate([[0], np.cumsum(inc.sum(1))]).astype(np.int64)
    sub = (np.concatenate([cols[inc[s] == 1] for s in masks]).astype(np.uint32), np.concatenate([vals[inc[s] == 1] for s in masks]).astype(np.float32))
    y = _oracle_raw(e, (rp, sub[0], sub[1]), p)
    phi = np.zeros(n)
    for i in range(n):
        without = masks[(masks >> i) & 1 == 0]
        size = inc[without].sum(1)
        wgt = np.array([math.factorial(s) * math.factorial(n - s - 1) for s in size]) / math.factorial(n)
        phi[i] = np.sum(wgt * (y[without | (1 << i)] - y[without]))
    return phi


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_shapley_by_enumeration(kind, monkeypatch):
    rng = np.random.default_rng(5)
    p, k = 50, 8
    m = _rows([1, 2, 5, 7, 10, 10], p, rng)
    m[1][-3] = m[1][-7]          # the last row holds one column twice
    e = _engine(kind, p, k, monkeypatch)
    phi = e.contrib(_mat(m, p))
    rp = m[0]
    for r in range(len(rp) - 1):
        a, b = rp[r], rp[r + 1]
        ref = _shapley(e, m[1][a:b], m[2][a:b], p)
        assert np.all(np.abs(phi[a:b] - ref) <= 1e-10 * (1 + np.abs(ref).max())), (r, phi[a:b], ref)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k1", [1, 0])
def test_one_entry_rows_are_exactly_the_linear_term(kind, k1, monkeypatch):
    rng = np.random.default_rng(9)
    p, k = 500, 16
    m = _rows([1] * 300, p, rng)
    e = _engine(kind, p, k, monkeypatch, k1=k1)
    phi = e.contrib(_mat(m, p))
    _, w, _ = e.get_params()
    want = m[2].astype(np.float64) * w[m[1]] if k1 else np.zeros(300)
    assert np.array_equal(phi, want)


def _hip():
    for name in ("libamdhip64.so", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")):
        try:
            return ctypes.CDLL(name)
        except OSError:
            continue
    pytest.fail("the HIP runtime library is not loadable")


def _device_slice(e, mat, r0, r1, cnt):
    """fmx_contrib_device for rows [r0, r1) (cnt entries) into a buffer of the HIP runtime's own, copied back"""
    hip = _hip()
    d = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(cnt, 1) * 8)) == 0
    try:
        e.contrib_device(mat, r0, r1, d.value)
        e.sync()
        h = np.empty(cnt)
        if cnt:
            assert hip.hipMemcpy(h.ctypes.data_as(ctypes.c_void_p), d, ctypes.c_size_t(cnt * 8), 2) == 0   # hipMemcpyDeviceToHost
    finally:
        hip.hipFree(d)
    return h


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_bitwise_invariance_over_slices_and_permutations(kind, monkeypatch):
    rng = np.random.default_rng(21)
    p, k = 20_000, 16
    lens = np.concatenate([rng.integers(0, 60, 3000), [2500, 0, 1, 4000]])
    m = _rows(lens, p, rng)
    e = _engine(kind, p, k, monkeypatch)
    mat = _mat(m, p)
    phi = e.contrib(mat)
    rp = m[0]
    n = len(rp) - 1
    cuts = [0, 1, 2, 17, 600, 601, 2999, 3000, 3001, 3003, n]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        assert np.array_equal(_device_slice(e, mat, r0, r1, int(rp[r1] - rp[r0])), phi[rp[r0]:rp[r1]]), (r0, r1)
    for r in (0, 5, 3000, n - 1):
        assert np.array_equal(_device_slice(e, mat, r, r + 1, int(rp[r + 1] - rp[r])), phi[rp[r]:rp[r + 1]])
    assert np.array_equal(e.contrib(mat), phi)
    perm = rng.permutation(n)
    rows = [(m[1][rp[r]:rp[r + 1]], m[2][rp[r]:rp[r + 1]]) for r in perm]
    mp = (np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64), np.concatenate([c for c, _ in rows]),
          np.concatenate([v for _, v in rows]))
    phip = e.contrib(_mat(mp, p))
    assert np.array_equal(phip, np.concatenate([phi[rp[r]:rp[r + 1]] for r in perm]))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_one_hot_matrix_equals_explicit_ones(kind, monkeypatch):
    from fmwr_amd import engine
    monkeypatch.delenv("FMX_UNIT_VALUES", raising=False)
    p, k = 5000, 8
    e = _engine(kind, p, k, monkeypatch)
    mu = engine.Matrix.synthetic(2000, p, 12, 3)          # unit values: the kernels never read val
    rp, col, val, _ = mu.export()
    assert np.all(val == 1.0)
    phi_u = e.contrib(mu)
    phi_x = e.contrib(_mat((rp, col, val), p))
    assert np.array_equal(phi_u, phi_x)
    ref, rmax = _closed_form(e, (rp, col, val))
    assert np.all(np.abs(phi_u - ref) <= 1e-12 * (1 + rmax))


def test_multi_gpu_engine_reads_its_primary_replica(monkeypatch):
    rng = np.random.default_rng(4)
    p, k = 400, 16
    m = _rows(list(rng.integers(0, 30, 200)), p, rng)
    e = _engine("mb32", p, k, monkeypatch, n_gpus=2, gpus_share_device=1)
    ref, rmax = _closed_form(e, m)
    assert np.all(np.abs(e.contrib(_mat(m, p)) - ref) <= 1e-12 * (1 + rmax))


def _set_summary_chunk(entries):
    from fmwr_amd import _lib as L
    L.check(L.lib().fmx_debug_contrib_summary_chunk(ctypes.c_int64(entries)))


@pytest.mark.parametrize("kind", ["seq64", "mb32"])
def test_summary(kind, monkeypatch):
    rng = np.random.default_rng(8)
    p, k = 3000, 16
    lens = np.concatenate([rng.integers(0, 50, 4000), [2200]])
    m = _rows(lens, p, rng)
    e = _engine(kind, p, k, monkeypatch)
    mat = _mat(m, p)
    phi = e.contrib(mat)
    s = e.contrib_summary(mat)
    col = m[1].astype(np.int64)
    assert np.array_equal(s["count"], np.bincount(col, minlength=p))
    ws = np.bincount(col, weights=phi, minlength=p)
    wa = np.bincount(col, weights=np.abs(phi), minlength=p)
    assert np.all(np.abs(s["sum"] - ws) <= 1e-12 * (1 + wa))
    assert np.all(np.abs(s["abs_sum"] - wa) <= 1e-12 * (1 + wa))
    s2 = e.contrib_summary(mat)
    for key in ("sum", "abs_sum", "count"):
        assert np.array_equal(s[key], s2[key])
    _set_summary_chunk(777)       # the next summary: chunks of at most 777 entries (the 2200-entry row is a chunk of its own)
    s3 = e.contrib_summary(mat)
    assert np.array_equal(s3["count"], s["count"])
    assert np.all(np.abs(s3["sum"] - s["sum"]) <= 1e-12 * (1 + wa))
    assert np.all(np.abs(s3["abs_sum"] - s["abs_sum"]) <= 1e-12 * (1 + wa))
    s4 = e.contrib_summary(mat)   # one-shot: the default chunking again
    assert np.array_equal(s4["sum"], s["sum"])


def _raw_from_fit(fit, data, normalize):
    """the model's raw score of every row: the device forward (link NONE) on the matrix predict() would build"""
    from fmwr_amd import _lib as L
    from fmwr_amd import api
    mdl = fit["Model"]
    controls = {"model": mdl["model.control"], "solver": mdl["solver.control"], "track": mdl["track.control"]}
    eng = api._engine_for(controls, data.dim[1], fit["Scales"]["target.range"], "sequential", 1, 0)
    eng.set_params(mdl["w0"], mdl["w"], mdl["v"])
    m = api._device_matrix(data, None, 0)
    if normalize:
        m.normalize(fit["Scales"]["mean"], fit["Scales"]["std"])
    return eng.predict(m, L.LINK_NONE)


def _check_explain(fit, X, data, normalize):
    import fmwr_amd as fm
    out = fm.fm_explain(fit, data, normalize=normalize, summary=True)
    C = out["contrib"]
    assert isinstance(C, sp.csr_matrix) and C.shape == X.shape
    assert np.array_equal(C.indptr, X.indptr) and np.array_equal(C.indices, X.indices)
    mdl = fit["Model"]
    assert out["intercept"] == (mdl["w0"] if mdl["model.control"]["hyper.params"]["keep.w0"] else 0.0)
    raw = _raw_from_fit(fit, data, normalize)
    sums = out["intercept"] + np.asarray(C.sum(1)).ravel()
    assert np.all(np.abs(sums - raw) <= 1e-10 * (1 + np.abs(raw)))
    sm = out["summary"]
    assert np.array_equal(sm["count"], np.bincount(C.indices, minlength=C.shape[1]))
    assert np.array_equal(sm["importance"], sm["abs_sum"] / np.maximum(sm["count"], 1))
    wa = np.bincount(C.indices, weights=np.abs(C.data), minlength=C.shape[1])
    assert np.all(np.abs(sm["sum"] - np.bincount(C.indices, weights=C.data, minlength=C.shape[1])) <= 1e-12 * (1 + wa))
    return out


@pytest.mark.parametrize("normalize", [False, True])
def test_fm_explain_end_to_end(normalize):
    import fmwr_amd as fm
    rng = np.random.default_rng(13)
    n, p = 600, 40
    X = sp.random(n, p, density=0.2, random_state=3, format="csr")
    X.data = rng.normal(0, 1, X.nnz)
    y_cls = np.where(rng.random(n) < 0.5, 0.0, 1.0)
    y_reg = rng.normal(0, 1, n)
    sgd = fm.fm_train(fm.fm_matrix(X, y_cls), normalize=normalize, seed=1,
                      control=[fm.model_control("CLASSIFICATION", **{"factor.number": 4}), fm.solver_control(max_iter=2000, solver=fm.SGD_solver())])
    als = fm.fm_train(fm.fm_matrix(X, y_reg), normalize=normalize, seed=2,
                      control=[fm.model_control("REGRESSION", **{"factor.number": 4}), fm.solver_control(max_iter=5, solver=fm.ALS_solver())])
    for fit in (sgd, als):
        a = _check_explain(fit, X, fm.fm_matrix(X), normalize)
        b = _check_explain(fit, X, fm.fm_matrix(X.tocsc()), normalize)   # dgCMatrix slots: transposed on the device
        assert np.array_equal(a["contrib"].data, b["contrib"].data)


def test_configs1_shaped_rows_against_the_closed_form(monkeypatch):
    from fmwr_amd import engine
    monkeypatch.delenv("FMX_UNIT_VALUES", raising=False)
    p, k, n = 1_000_000, 16, 1_000_000
    e = _engine("mb32", p, k, monkeypatch)
    mat = engine.Matrix.synthetic(n, p, 30, 11).synthetic_values(12)
    r0, r1 = 400_000, 460_000
    rp, col, val, _ = mat.export(r0, r1)
    phi = _device_slice(e, mat, r0, r1, int(rp[-1]))
    sample = np.random.default_rng(0).choice(r1 - r0, 500, replace=False)
    rows = [(col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]]) for r in sample]
    ms = (np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64), np.concatenate([c for c, _ in rows]),
          np.concatenate([v for _, v in rows]))
    ref, rmax = _closed_form(e, ms)
    got = np.concatenate([phi[rp[r]:rp[r + 1]] for r in sample])
    assert np.all(np.abs(got - ref) <= 1e-12 * (1 + rmax))
    ys = e.predict(_mat(ms, p))
    assert np.all(np.abs(e.get_w0() + _row_sums(got, ms[0]) - ys) <= 1e-10 * (1 + np.abs(ys)))
