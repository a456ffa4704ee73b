"""A matrix changed in place after its caches are warm must behave as the same matrix changed before anything ran on it.

Five calls change an fmx_matrix in place -- fmx_matrix_synthetic_values, _scales, _normalize, _set_fields, _set_labels -- and a matrix carries caches
derived from its rows: the per-tile plans with their copies of the values, the phase-1 schedule, the whole-matrix CSC, the tiled and block forms of the
ALS sweep, the carried q table, the captured sweep graph (FMX_ALS_GRAPH=1), the shards of an n_gpus handle.  Every case builds the matrix twice:
  cold   change, then run the consumer;
  warm   run the consumer once (every cache it uses is built), change, fmx_set_params back to the same parameters, run the consumer again.
Both must agree in every bit of what the consumer returns and of fmx_get_params, and in the flags and the layout (tests/flags_model.py names them).
Cold against warm, not warm against an uploaded copy: a producer's claimed flags (a generator's max_row_len) may differ from detected ones.

PAIRS below is the table of (consumer, shape, changes) that runs; each shape is the smallest an existing test uses for that form, and the form is
asserted with that test's own info call before the change."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rows_deal_cases as rd
from tests import util
from tests.test_gpu_flags import state

pytestmark = pytest.mark.gpu

VOCAB = [50, 40, 30, 7]
Z = 30
_host = {}


# ------------------------------------------------------------------------------------------------------------------------------ matrices
START = {"a": "unit", "b": "real", "c": "real", "d": "twos", "e": "unit", "f": "real"}     # the values a change starts from


def _values(start, rng, nnz):
    return {"unit": np.ones(nnz, np.float32), "twos": np.full(nnz, 2.0, np.float32), "real": rng.normal(0, 1, nnz).astype(np.float32)}[start]


def _field_rows(rng, n, d):
    base = d + np.concatenate([[0], np.cumsum(VOCAB)])
    ids = np.stack([base[c] + rng.integers(1, VOCAB[c] - 1, n) for c in range(len(VOCAB))], axis=1)     # (the vocabularies' ends never occur: wider bases exist)
    col = np.concatenate([np.tile(np.arange(d), (n, 1)), ids], axis=1).astype(np.uint32)
    return np.arange(n + 1, dtype=np.int64) * (d + len(VOCAB)), col.ravel(), int(base[-1]), base


def host(shape, start):
    """(rp, col, val, p, y, extra) of a starting matrix, made once"""
    from fmwr_amd import _lib as L, engine
    key = (shape, start)
    if key in _host:
        return _host[key]
    rng = np.random.default_rng(len(shape) * 100 + len(start))
    extra = {}
    if shape == "head":       # tests/rows_deal_cases.py: a head tile of 32 768 rows of 30 entries, then a tail tile of 257 mixed rows
        rp, col, _, _ = rd.problem(rd.CASES[0], 257, rd.seed_of(0, 257))
        p = rd.CASES[0]["p"]
    elif shape in ("ragged", "group"):
        n, p = (3_000, 500) if shape == "ragged" else (12_000, 900)
        rp, col, _ = util.random_csr(n, p, 9, seed=3, empty_rows=shape == "ragged")
    elif shape == "fields":
        d = 2 if start == "real" else 0
        rp, col, p, base = _field_rows(rng, 3_000, d)
        extra = dict(d=d, wide=base.tolist())
    else:
        kind, n, p, z, seed = {"colwalk": ("strat", 20_000, 6_000, Z, 41), "tiled": ("strat", 16_384, 6_000, Z, 59), "block": ("strat", 20_000, 6_000, Z, 67),
                               "record": ("iid", 20_000, 6_000, Z, 47), "counter": ("iid", 20_000, 6_000, Z, 47), "graph": ("iid", 20_000, 6_000, Z, 51),
                               "coloured": ("iid", 9_000, 900, 20, 78)}[shape]
        m = engine.Matrix.synthetic(n, p, z, seed) if kind == "strat" else engine.Matrix.synthetic_iid(n, p, z, seed, law=L.COLUMNS_UNIFORM)
        rp, col, _, _ = m.export()
        m.close()
    val = _values(start, rng, len(col))
    if shape == "fields" and start == "real":
        val.reshape(-1, 2 + len(VOCAB))[:, 2:] = 1.0          # dense columns real, the fields one-hot: a layout with a dense prefix
    n = len(rp) - 1
    y = util.labels(n, 5) if shape in ("ragged", "group", "fields", "head") else util.labels(n, 5, "regression")
    _host[key] = (rp, col, val, p, y, extra)
    return _host[key]


def start_of(which, shape):
    return "unit" if (shape, which) == ("head", "f") else START[which]      # (the schedule is built for one-hot matrices only)


def upload(shape, start):
    from fmwr_amd import engine
    rp, col, val, p, y, _ = host(shape, start)
    return engine.Matrix.from_csr(rp, col, val, p, y)


# ------------------------------------------------------------------------------------------------------------------------------ changes
def change(m, which, shape):
    p = m.p
    rng = np.random.default_rng(77)
    if which == "a":
        m.synthetic_values(8)
    elif which == "b":
        m.scales(np.arange(p))
    elif which == "c":
        m.normalize(rng.normal(0, 0.3, p), np.where(rng.random(p) < 0.05, 0.0, rng.uniform(0.5, 2.0, p)))
    elif which == "d":
        m.normalize(np.zeros(p), np.full(p, 2.0))
    elif which == "e":
        ex = host(shape, START["e"])[5]
        m.set_fields(ex["d"], ex["wide"])
    elif which == "f":
        m.set_labels(-host(shape, start_of("f", shape))[4][::-1])
    else:
        raise KeyError(which)


# ------------------------------------------------------------------------------------------------------------------------------ consumers
ALS_ENV = {"colwalk": {}, "tiled": {"FMX_ALS_TILED": "1", "FMX_ALS_TILE_ROWS": "2048", "FMX_ALS_ORDER": "1"},
           "block": {"FMX_ALS_TILED": "1", "FMX_ALS_TILE_ROWS": "4096", "FMX_ALS_BLOCK_ROWS": "512", "FMX_ALS_ORDER": "2"},
           "record": {"FMX_ALS_PERSIST": "1"}, "counter": {"FMX_ALS_PERSIST": "counter"}, "coloured": {},
           "graph": {"FMX_ALS_GRAPH": "1", "FMX_ALS_PERSIST": "0", "FMX_ALS_GRAPH_VERBOSE": "1"}}   # (the persistent form would take the deep plan before the graph is asked)


def _engine(consumer, shape, p):
    from fmwr_amd import _lib as L, engine
    kind = consumer.split(":")[0]
    if kind == "step":          # step:sgd:32, step:ftrl:64
        _, solver, bits = consumer.split(":")
        return engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD if solver == "sgd" else L.SOLVER_FTRL, num_factor=8, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3,
                             l1_v=1e-4 if solver == "ftrl" else 0.0, mode=L.MODE_MINIBATCH, batch_rows=512, state_fp64=int(bits == "64"))
    if kind == "sched":         # the engine of tests/test_gpu_rows_deal.py: one step covers both tiles
        return engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=rd.K, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, mode=L.MODE_MINIBATCH,
                             batch_rows=2 * rd.HEAD, tile_rows=rd.HEAD)
    if kind == "query":
        return engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=8, mode=L.MODE_MINIBATCH, batch_rows=512)
    if kind == "seqtrain":
        return engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=8, learn_rate=0.05, l2_w1=1e-4, l2_v=1e-4, mode=L.MODE_SEQUENTIAL)
    if kind == "group":
        return engine.Engine(p, task=L.TASK_CLASSIFICATION, solver=L.SOLVER_SGD, num_factor=8, learn_rate=0.05, l2_w1=1e-3, l2_v=1e-3, mode=L.MODE_MINIBATCH, batch_rows=500,
                             n_gpus=2, gpus_share_device=1)
    if kind == "vsweep":
        e = engine.Engine(p, task=L.TASK_REGRESSION, solver=L.SOLVER_MCMC, num_factor=16, mode=L.MODE_SEQUENTIAL, **({"als_max_levels": -2} if shape == "coloured" else {}))
        if shape == "coloured":
            e.als_carry_q(True)
        return e
    if kind == "alstrain":
        return engine.Engine(p, task=L.TASK_REGRESSION, solver=L.SOLVER_ALS, num_factor=16, mode=L.MODE_SEQUENTIAL, l2_w1=0.1, l2_v=0.1)
    raise KeyError(consumer)


def _assert_form(e, m, consumer, shape):
    """the form the case is about, by the info call of the test that owns the shape (before the change)"""
    kind = consumer.split(":")[0]
    if kind == "group":
        assert e.group_info()["replicas"] == 2 and e.group_info()["share_one_device"]
    if kind not in ("vsweep", "alstrain"):
        return
    levels, largest, approx, _ = e.als_plan(m)
    if shape == "colwalk":
        assert not approx and levels == Z and e.als_level_order_form(m) == 0
    elif shape == "tiled":
        assert e.als_tiled(m)[0] == levels == Z and e.als_level_order_form(m) == 1 and e.als_tiled(m)[1] == 2048
    elif shape == "block":
        assert e.als_tiled(m)[0] == levels == Z and e.als_level_order_form(m) == 2
    elif shape in ("record", "counter", "graph"):
        assert not approx and levels > 1_000 and largest <= 256
    elif shape == "coloured":
        assert levels > 0 and e.als_plan_kind(m) == 3


def consume(e, m, consumer):
    """what the consumer returns, as a list of arrays"""
    kind = consumer.split(":")[0]
    if kind == "step":
        for b in range(3):
            e.step(m, b)
        e.sync()
        return []
    if kind == "sched":
        for _ in range(3):
            e.step(m, 0, 0)
        e.sync()
        return []
    if kind == "query":
        return [e.predict(m), e.contrib(m), *e.interactions(m, 3)]
    if kind == "seqtrain":
        return [np.array([e.train(m, 500)])]
    if kind == "group":
        return [np.array([e.train(m, 2 * 500 * 2)]), e.predict(m)]
    if kind == "alstrain":
        e.als_train(m, 2, with_v=True)
        return []
    k, p = 16, m.p
    g = np.random.default_rng(4).normal(0, 1, m.n)
    lam, mu = np.linspace(1.0, 2.0, k), np.linspace(-0.05, 0.05, k)
    z = np.random.default_rng(8).normal(0, 1, (k, p))
    out = []
    for normals in (None, None, z, z):           # two plain sweeps, then two with the caller's normals (the Gibbs form)
        g = e.als_vsweep(m, g, alpha=1.1, v_lambda=lam, v_mu=mu, std_normals=normals)
        out.append(g.copy())
    return out


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def sched_counter():
    """fmx_debug_rows_sched_launches: launches that took the scheduled form, launches turned away at the stage size, schedule builds"""
    import ctypes
    from fmwr_amd import _lib as L
    a = (ctypes.c_int64 * 3)()
    L.check(L.lib().fmx_debug_rows_sched_launches(a))
    return np.array(list(a), np.int64)


def run(consumer, shape, which, warm):
    """(bits of the consumer's output and of the parameters, (flags, layout), the schedule counters of every consume)"""
    m = upload(shape, start_of(which, shape))
    k = 16 if consumer.split(":")[0] in ("vsweep", "alstrain", "sched") else 8
    counts = []
    w0, w, v = util.params(m.p, k, 17, stdev=0.1, fp32=False)
    e = _engine(consumer, shape, m.p)
    e.set_params(w0, w, v)
    if warm:
        _assert_form(e, m, consumer, shape)
        c0 = sched_counter()
        first = consume(e, m, consumer)
        counts.append(sched_counter() - c0)
        assert not first or any(np.any(np.asarray(x) != 0) for x in first)
        change(m, which, shape)
        e.set_params(w0, w, v)
    else:
        change(m, which, shape)
    c0 = sched_counter()
    out = consume(e, m, consumer)
    counts.append(sched_counter() - c0)
    gw0, gw, gv = e.get_params()
    res = [_bits(x) for x in out + [np.array([gw0]), gw, gv]], state(m), counts
    assert np.all(np.isfinite(gw)) and np.all(np.isfinite(gv))
    e.close(); m.close()
    return res


# ------------------------------------------------------------------------------------------------------------------------------ the table
STEPS = ["step:sgd:32", "step:sgd:64", "step:ftrl:32", "step:ftrl:64"]
ALS_FORMS = ["colwalk", "tiled", "block", "record", "counter", "coloured", "graph"]
PAIRS = ([(c, "ragged", ch) for c in STEPS for ch in "abcdf"]                          # the plans and their copies of the values (bval)
         + [(c, "fields", ch) for c in STEPS for ch in "abcdef"]                       # the per-field builder; (d) makes the layout appear, (a) / (b) take it away
         + [("query", s, ch) for s in ("ragged", "fields") for ch in "abcd"] + [("query", "fields", "e")]   # no cache: unit_values read at call time
         + [("seqtrain", "ragged", ch) for ch in "abcdf"]
         + [("vsweep", s, ch) for s in ALS_FORMS for ch in "abcd"] + [("vsweep", "colwalk", "f")]
         + [("alstrain", "record", ch) for ch in "abdf"]
         + [("group", "group", ch) for ch in "abdf"] + [("group", "fields", "e")])        # the shards are re-cut


@pytest.mark.parametrize("consumer,shape,which", PAIRS, ids=[f"{c}-{s}-{ch}" for c, s, ch in PAIRS])
def test_a_warm_matrix_changed_in_place_equals_a_cold_one(consumer, shape, which, monkeypatch, capfd):
    for k, v in ALS_ENV.get(shape, {}).items() if consumer in ("vsweep", "alstrain") else ():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    cold, cold_state, _ = run(consumer, shape, which, warm=False)
    captured_cold = capfd.readouterr().err.count("fmx: als graph (V sweep)")
    warm, warm_state, _ = run(consumer, shape, which, warm=True)
    captured_warm = capfd.readouterr().err.count("fmx: als graph (V sweep)")
    assert warm_state == cold_state, (warm_state, cold_state)
    assert len(cold) == len(warm)
    for i, (a, b) in enumerate(zip(cold, warm)):
        assert a.shape == b.shape and np.array_equal(a, b), (consumer, shape, which, "output", i, int(np.sum(a != b)), a.size)
    if shape == "graph":
        # the V sweep's launches are captured once per (plan, buffers, VALUES): the cold run captures once, the warm run once before the change and once more
        # after it -- a graph replayed across the change would hold the freed CSC and the old unit flag
        assert (captured_cold, captured_warm) == (1, 2), (captured_cold, captured_warm)


# ------------------------------------------------------------------------------------------------------------------------------ the phase-1 schedule
# The scheduled form of phase 1 is chosen by switches that are read once per process (FMX_ROWS_SCHED=2: wherever a schedule fits), so these cases run in
# one child process, as tests/test_gpu_rows_deal.py's do, on its head-tile shape.
SCHED_CHANGES = "adf"
_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
from tests import test_gpu_matrix_changes as T
out = {}
for which in T.SCHED_CHANGES:
    cold, cold_state, cc = T.run("sched", "head", which, warm=False)
    warm, warm_state, wc = T.run("sched", "head", which, warm=True)
    same = warm_state == cold_state and len(cold) == len(warm) and all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(cold, warm))
    out[which] = dict(same=bool(same), unit=[cold_state[0]["unit_values"], warm_state[0]["unit_values"]], cold=[c.tolist() for c in cc], warm=[c.tolist() for c in wc])
print("RESULT " + json.dumps(out))
"""


@pytest.fixture(scope="module")
def sched_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("FMX_") or k == "FMX_LIB_PATH"}
    env.update({"FMX_ROWS_SCHED": "2", "FMX_ROWS_SCHED_POLICY": "deal"})
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=root, capture_output=True, text=True, timeout=300)
    lines = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    return json.loads(lines[-1][len("RESULT "):])


@pytest.mark.parametrize("which", list(SCHED_CHANGES))
def test_the_phase1_schedule_follows_an_in_place_change(sched_runs, which):
    """counters per consume: [launches in the scheduled form, launches turned away at the stage size, schedule builds]; three steps over two tiles each"""
    r = sched_runs[which]
    assert r["same"], r
    before, after = r["warm"]
    if which == "a":        # one-hot -> real: the schedule ran, and must not be used afterwards (rows_sched_build skips matrices that are not one-hot)
        assert before[0] > 0 and before[2] == 1 and after == [0, 0, 0] and r["cold"] == [[0, 0, 0]] and r["unit"] == [0, 0], r
    elif which == "d":      # real -> one-hot: nothing to run before; afterwards the schedule is built and taken, warm as cold
        assert before == [0, 0, 0] and after[0] > 0 and after == r["cold"][0] and r["unit"] == [1, 1], r
    else:                   # other labels: the schedule does not depend on them and stays; the warm run builds none again
        assert before[0] > 0 and before[2] == 1 and after[0] == before[0] and after[2] == 0 and r["cold"][0] == before, r
