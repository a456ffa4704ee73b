"""The driver parses bench.py's LAST stdout line; round 5's line had grown to 26.7 KB and came back unparsed (BENCH_r05.parsed = null).
driver_line() is the compaction: fed round 5's full line (profiles/r05c_bench_default.json) it must fit LINE_LIMIT and keep every key the
contract names (metric / value / config.workload / roofline / cpu_baseline)."""
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _full():
    return json.load(open(os.path.join(ROOT, "profiles", "r05c_bench_default.json")))


def test_driver_line_fits_and_keeps_the_contract_keys():
    full = _full()
    assert len(json.dumps(full)) > 20_000                     # the line that was not parsed
    line = bench.driver_line(full)
    text = json.dumps(line)
    assert len(text) <= bench.LINE_LIMIT <= 4000
    assert "\n" not in text
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["config"]["workload"].startswith("synthetic 10000000x1000000")
    assert "model" not in line["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "dominant_kernel", "algorithmic_bytes_per_example"):
        assert k in line["roofline"], k
    assert abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-4
    for k in ("value", "unit", "cores", "kind", "sample", "cpu_model"):
        assert k in line["cpu_baseline"], k
    assert abs(line["value"] - full["value"]) / full["value"] < 1e-5
    assert abs(line["ms_per_step"] - full["ms_per_step"]) / full["ms_per_step"] < 1e-5
    oc = line["other_configs"]
    assert set(oc) == set(full["other_configs"])
    for name, e in oc.items():
        assert set(e) <= {"value", "ms_per_step", "frac", "frac_basis", "effective_frac", "traffic_ratio", "cpu_value"}, name
        assert e["value"] > 0 and 0 < e["frac"] <= 1.0


def test_driver_line_sheds_before_it_overflows():
    full = _full()
    full["other_configs"] = {f"side_{i}": dict(v) for i in range(12) for v in full["other_configs"].values()}   # 12 x 7 summary entries: past the budget
    line = bench.driver_line(full)
    assert len(json.dumps(line)) <= bench.LINE_LIMIT
    assert "roofline" in line and "cpu_baseline" in line


def test_emit_puts_one_line_on_stdout_and_the_details_on_stderr(tmp_path, monkeypatch):
    from contextlib import redirect_stderr
    monkeypatch.setenv("FMX_BENCH_DETAILS_DIR", str(tmp_path))
    monkeypatch.delenv("FMX_BENCH_DETAILS", raising=False)
    out, err = io.StringIO(), io.StringIO()
    with redirect_stdout(out), redirect_stderr(err):
        bench.emit(_full())
    # stdout: the ONE line, whole, parseable as it stands -- however the driver reads it
    text = out.getvalue()
    assert text.count("\n") == 1 and len(text) <= bench.LINE_LIMIT + 1
    last = json.loads(text)
    assert last["metric"] and last["roofline"]["frac"] > 0 and last["cpu_baseline"]["value"] > 0
    # stderr: the details, line by line, none longer than the driver's own line may be; they add up to the full object, which is also in the file
    lines = err.getvalue().strip().split("\n")
    assert len(lines) > 10 and all(ln.startswith("DETAILS ") for ln in lines) and max(len(ln) for ln in lines) <= bench.LINE_LIMIT
    full = json.load(open(tmp_path / "bench_details.json"))
    assert bench.details_from_lines(lines) == full == _full()
    # FMX_BENCH_DETAILS=stdout: the details ahead of the line on stdout, the line still last; =off: the line alone
    monkeypatch.setenv("FMX_BENCH_DETAILS", "stdout")
    out = io.StringIO()
    with redirect_stdout(out):
        bench.emit(_full())
    ls = out.getvalue().strip().split("\n")
    assert json.loads(ls[-1])["value"] == last["value"] and all(ln.startswith("DETAILS ") for ln in ls[:-1])


def test_a_plain_run_times_the_headline_and_full_keeps_the_rest():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_extras and a.no_other_configs and a.cpu_rows == 0
    f = bench.parse(["--full"])
    assert (f.steps, f.warmup, f.no_extras, f.no_other_configs, f.cpu_rows) == (40, 5, False, False, 5_000_000)
    assert bench.parse(["--full", "--solver", "mcmc"]).cpu_rows == 4_000_000
    # --steps is the number of timed steps for every solver: the sweeps' shorter defaults apply only when neither count is given
    assert (bench.parse(["--solver", "mcmc"]).steps, bench.parse(["--solver", "mcmc"]).warmup) == (5, 1)
    m = bench.parse(["--solver", "mcmc", "--steps", "40", "--warmup", "5"])
    assert (m.steps, m.warmup) == (40, 5)
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)


class _Rows:
    """the two calls model_outputs() makes of an engine"""
    def __init__(self, k):
        self.k = k

    def get_rows(self, ids):
        ids = np.asarray(ids, np.float64)
        return ids * 0.5, np.stack([ids + f for f in range(self.k)])

    def get_w0(self):
        return 0.25


def test_dump_outputs_are_float_seeded_and_under_64_mb(tmp_path):
    for p, k, fp64 in ((1_000_000, 16, False), (33_000_000, 32, False), (1_000_000, 16, True), (1_000_000, 64, False), (20_000, 16, False)):
        d = tmp_path / f"{p}_{k}_{int(fp64)}"
        a = bench.parse(["--dump-outputs", str(d)])
        out = bench.model_outputs(a, _Rows(k), p, k, fp64)
        bench.dump_outputs(a, out)
        files = {f.name: np.load(f) for f in d.iterdir()}
        assert set(files) == {"w0.npy", "feature_ids.npy", "w.npy", "v.npy"}
        assert all(x.dtype == (np.float64 if fp64 or n in ("w0.npy", "feature_ids.npy") else np.float32) for n, x in files.items())
        ids = files["feature_ids.npy"]
        assert np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < p
        assert files["v.npy"].shape == (k, len(ids)) and np.array_equal(files["w.npy"], (ids * 0.5).astype(files["w.npy"].dtype))
        # the sweeps add a residual sample of DUMP_ROWS rows and their ids
        assert sum(f.stat().st_size for f in d.iterdir()) + bench.DUMP_ROWS * 16 < 64e6
        if p == 20_000:
            assert np.array_equal(ids, np.arange(p))
        again = bench.model_outputs(bench.parse(["--dump-outputs", str(d)]), _Rows(k), p, k, fp64)
        assert np.array_equal(again["feature_ids"], ids)
    owned = bench.model_outputs(a, _Rows(16), 1_000_000, 16, False, owner=(1, 4))["feature_ids"]
    assert len(owned) > 0 and np.all(owned % 4 == 1)
