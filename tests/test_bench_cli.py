"""bench.py's command line: a plain run measures the headline figure only,
`--full` adds the rest, `--dump-outputs DIR` writes what the last timed solve
handed back, identically from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["error_distance_list", "error_list", "error_list_user", "fnorm_trace", "result", "x"]


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def _fake_solve(n, m, M):
    rng = np.random.default_rng(3)
    last = types.SimpleNamespace(
        x=rng.standard_normal(n), fnorm_trace=rng.standard_normal(5),
        result={"success": 1, "outer_iterations": 4, "error_rms": 0.25, "time_solve_s": 0.1})
    prob = types.SimpleNamespace(num_residuals=m, num_obs=M)
    # the caller's buffers may be longer than the problem needs
    outs = (rng.standard_normal(m + 3), rng.standard_normal(m + 3), rng.standard_normal(M + 1))
    return prob, last, outs


def test_dump_outputs_writes_the_callers_arrays(tmp_path):
    bench = _bench()
    prob, last, outs = _fake_solve(7, 10, 5)
    bench.dump_outputs(str(tmp_path), prob, last, outs)
    assert sorted(f[:-4] for f in os.listdir(tmp_path) if f.endswith(".npy")) == NAMES
    np.testing.assert_array_equal(np.load(tmp_path / "x.npy"), last.x)
    np.testing.assert_array_equal(np.load(tmp_path / "error_list.npy"), outs[0][:10])
    np.testing.assert_array_equal(np.load(tmp_path / "error_list_user.npy"), outs[1][:10])
    np.testing.assert_array_equal(np.load(tmp_path / "error_distance_list.npy"), outs[2][:5])
    fields = json.load(open(tmp_path / "result_fields.json"))
    assert "time_solve_s" not in fields  # wall-clock fields differ from run to run
    rec = dict(zip(fields, np.load(tmp_path / "result.npy")))
    assert rec == {"error_rms": 0.25, "outer_iterations": 4.0, "success": 1.0}
    assert all(np.load(tmp_path / (n + ".npy")).dtype == np.float64 for n in NAMES)


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 14)
    prob, last, outs = _fake_solve(3000, 4000, 2000)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), prob, last, outs)
    bench.dump_outputs(str(b), prob, last, outs)
    total = sum(np.load(a / f).nbytes for f in os.listdir(a) if f.endswith(".npy"))
    assert total <= 1 << 14
    idx = np.load(a / "x_index.npy").astype(np.int64)
    assert idx.size > 1 and np.all(np.diff(idx) > 0)
    np.testing.assert_array_equal(np.load(a / "x.npy"), last.x[idx])
    for f in os.listdir(a):  # the sample is fixed
        if f.endswith(".npy"):
            np.testing.assert_array_equal(np.load(a / f), np.load(b / f))


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr


def _run(tmp, *extra):
    # a C4 window of 8 frames: a few milliseconds per solve
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
           "--warmup", "1", "--frames", "8", "--scale", "0.016", *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=str(tmp))
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_and_dump(tmp_path):
    d = [_run(tmp_path, "--dump-outputs", str(tmp_path / k)) for k in ("a", "b")]
    for line in d:
        assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False
        assert line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "residuals/s" and line["dtype"] == "f64"
        assert line["higher_is_better"] is True
        # measured only with --full
        assert line["roofline"] is None and line["reduced_cholesky"] is None
        assert line["cpu_baseline"] is None and line["device_resident"] is None
    cfg = d[0]["config"]
    for n in NAMES:
        a, b = np.load(tmp_path / "a" / (n + ".npy")), np.load(tmp_path / "b" / (n + ".npy"))
        assert a.dtype == np.float64 and np.all(np.isfinite(a))
        np.testing.assert_array_equal(a, b)
    assert np.load(tmp_path / "a" / "x.npy").size == cfg["parameters"]
    assert np.load(tmp_path / "a" / "error_list.npy").size == cfg["residuals"]
    assert np.load(tmp_path / "a" / "error_distance_list.npy").size == cfg["observations"]
    fields = json.load(open(tmp_path / "a" / "result_fields.json"))
    rec = dict(zip(fields, np.load(tmp_path / "a" / "result.npy")))
    assert rec["error_rms"] == d[0]["final_rms_px"]
    assert rec["outer_iterations"] == d[0]["lm_iterations_per_solve"]


@pytest.mark.gpu
def test_full_run_fills_the_rest(tmp_path):
    line = _run(tmp_path, "--full", "--no-traffic", "--no-cpu-baseline")
    assert line["full"] is True and line["steps"] == 3
    assert line["device_resident"]["ms_per_step"] > 0
    assert line["roofline"]["bound"] in ("hbm", "mfma")
    assert line["reduced_cholesky"]["reduced_dim"] > 0
