"""Host side of the deviation metrics: the result lines of
``SolveResult.error_metric_strings`` parse back through a restatement of
mmSolver's ``_string_get_error_per_frame`` / ``_string_get_error_per_marker_per_frame``
(solveresult.py:201-244), the solve-node summary follows
``create_deviation_attrs_on_node`` (adjust_results_helpers.cpp:213-268), and
``abi.MmbaErrorMetrics`` has the header's layout.  No device here."""
import collections
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import (RESULT_SPLIT_CHAR, SolveResult, deviation_summary,
                                            solve_node_summary)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mmba.h")


def parse(lines):
    """solveresult.py: key=value lines -> per-frame dict, per-marker per-frame dict."""
    per_frame, per_marker = {}, collections.defaultdict(dict)
    for key, value in (ln.split("=", 1) for ln in lines):
        v = value.split("#")
        if key == "error_per_frame":
            per_frame[float(v[0])] = float(v[1])
        elif key == "error_per_marker_per_frame":
            per_marker[v[0]][float(v[1])] = float(v[2])
    return per_frame, per_marker


def host_metrics(prob, ed):
    """The dict ``Solver.error_metrics()`` returns, restated on the host."""
    F, K = prob.num_frames, prob.num_markers
    mt = {"frame_count": np.zeros(F, np.int32), "frame_avg": np.zeros(F),
          "frame_max": np.zeros(F), "frame_max_marker": np.full(F, -1, np.int32),
          "marker_count": np.zeros(K, np.int32), "marker_avg": np.zeros(K),
          "marker_max": np.zeros(K), "marker_max_frame": np.full(K, -1, np.int32)}
    for i, d in enumerate(ed):
        for ax, g, key in (("frame", prob.obs_frame[i], prob.obs_marker[i]),
                           ("marker", prob.obs_marker[i], prob.obs_frame[i])):
            mt[ax + "_count"][g] += 1
            mt[ax + "_avg"][g] += d
            if d > mt[ax + "_max"][g]:
                mt[ax + "_max"][g] = d
                mt["frame_max_marker" if ax == "frame" else "marker_max_frame"][g] = key
    for ax in ("frame", "marker"):
        n = mt[ax + "_count"]
        mt[ax + "_avg"] = np.where(n > 0, mt[ax + "_avg"] / np.maximum(n, 1), 0.0)
    return mt


def make_result(prob, ed, fetched=True):
    return SolveResult(x=np.asarray(prob.x0), fvec=None, err_user=None,
                       err_dist=ed if fetched else None, result={}, fnorm_trace=np.zeros(0),
                       problem=prob, metrics=host_metrics(prob, ed))


def scene():
    """Frames 3 and 6 lose every observation."""
    prob = S.make_config(3, frames=8, scale=0.001)
    keep = ~np.isin(np.asarray(prob.obs_frame), (3, 6))
    prob.obs_marker = np.asarray(prob.obs_marker)[keep]
    prob.obs_frame = np.asarray(prob.obs_frame)[keep]
    ed = np.random.default_rng(5).uniform(0.01, 30.0, int(keep.sum()))
    return prob, ed


def sig6(v):
    return float("%g" % v)  # the lines carry numberToString's 6 significant digits (B10)


def test_strings_round_trip():
    prob, ed = scene()
    frames = 1001 + np.arange(prob.num_frames)
    names = ["mkr_%03d_MKR" % k for k in range(prob.num_markers)]
    res = make_result(prob, ed)
    lines = res.error_metric_strings(frame_numbers=frames, marker_names=names)
    assert all(ln.count("=") == 1 and RESULT_SPLIT_CHAR == "#" for ln in lines)
    per_frame, per_marker = parse(lines)
    mt = res.metrics
    seen = [f for f in range(prob.num_frames) if mt["frame_count"][f] > 0]
    assert sorted(per_frame) == [float(frames[f]) for f in seen]
    for f in seen:
        assert per_frame[float(frames[f])] == sig6(mt["frame_avg"][f])
    assert sum(len(v) for v in per_marker.values()) == prob.num_obs
    for i in range(prob.num_obs):
        got = per_marker[names[prob.obs_marker[i]]][float(frames[prob.obs_frame[i]])]
        assert got == sig6(ed[i])
    # default labels: the indices
    pf, pm = parse(res.error_metric_strings())
    assert sorted(pf) == [float(f) for f in seen]
    assert set(pm) == {"marker_%d" % k for k in set(prob.obs_marker)}


def test_frames_without_observations_are_omitted():
    prob, ed = scene()
    lines = make_result(prob, ed).error_metric_strings()
    per_frame, _ = parse(lines)
    assert 3.0 not in per_frame and 6.0 not in per_frame
    assert len(per_frame) == prob.num_frames - 2


def test_device_resident_solve_has_no_per_marker_lines():
    prob, ed = scene()
    lines = make_result(prob, ed, fetched=False).error_metric_strings()
    assert lines and all(ln.startswith("error_per_frame=") for ln in lines)
    assert parse(lines)[0] == parse(make_result(prob, ed).error_metric_strings())[0]


def test_result_strings_unchanged():
    r = dict(success=1, reason_number=2, error_final=1.5, error_avg=1.0, error_max=2.0,
             error_min=0.5, iterations=3, function_evals=4, jacobian_evals=2, user_interrupted=0)
    res = SolveResult(x=None, fvec=None, err_user=None, err_dist=None, result=r,
                      fnorm_trace=None)
    assert res.metrics is None
    lines = res.result_strings()
    assert lines[-1] == "user_interrupted=0" and len(lines) == 10
    assert not any(ln.startswith("error_per") for ln in lines)


def summary_restated(frames, values):
    """create_deviation_attrs_on_node over one series."""
    count, avg, vmax, fmax = 0, 0.0, -0.0, -1.0
    for f, v in zip(frames, values):
        avg += v
        count += 1
        if v > vmax:
            vmax, fmax = v, f
    if count > 0:
        avg = avg / float(count)
    return avg, vmax, int(fmax)


def test_solve_node_summary():
    prob, ed = scene()
    mt = host_metrics(prob, ed)
    frames = 1001 + np.arange(prob.num_frames)
    has = mt["frame_count"] > 0
    assert solve_node_summary(mt, frames) == summary_restated(frames[has], mt["frame_avg"][has])
    assert solve_node_summary(mt) == summary_restated(np.arange(prob.num_frames)[has],
                                                      mt["frame_avg"][has])
    # a marker's own series gives its three attributes
    k = int(prob.obs_marker[0])
    sel = np.asarray(prob.obs_marker) == k
    avg, vmax, fmax = deviation_summary(np.asarray(prob.obs_frame)[sel], ed[sel])
    assert (vmax, fmax) == (mt["marker_max"][k], mt["marker_max_frame"][k])
    assert abs(avg - mt["marker_avg"][k]) <= 1e-15 * avg
    # nothing above 0: maximum 0 at frame -1; nothing at all: average 0 too
    assert deviation_summary([4, 5], [0.0, 0.0]) == (0.0, 0.0, -1)
    assert deviation_summary([], []) == (0.0, 0.0, -1)


def test_struct_layout_matches_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu",'
           'sizeof(mmba_error_metrics));' % HEADER)
    for name, _ in abi.MmbaErrorMetrics._fields_:
        src += 'printf(" %%zu",offsetof(mmba_error_metrics,%s));' % name
    src += "}"
    d = tempfile.mkdtemp()
    try:
        open(os.path.join(d, "s.c"), "w").write(src)
        subprocess.check_call(["gcc", os.path.join(d, "s.c"), "-o", os.path.join(d, "s")])
        got = [int(v) for v in subprocess.check_output([os.path.join(d, "s")]).split()]
    finally:
        shutil.rmtree(d)
    assert got == [C.sizeof(abi.MmbaErrorMetrics)] + \
        [getattr(abi.MmbaErrorMetrics, name).offset for name, _ in abi.MmbaErrorMetrics._fields_]


def test_symbols_listed():
    for name in ("mmba_plan_error_metrics", "mmba_debug_error_metrics"):
        assert name in abi.EXPORTED_SYMBOLS
