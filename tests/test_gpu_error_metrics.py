"""Per-frame and per-marker deviation metrics reduced on the device
(mmba_plan_error_metrics) against a numpy restatement of
ErrorMetricsResult::fill (adjust_results.h:392-463) and
create_deviation_attrs_on_node (adjust_results_helpers.cpp:213-246):
sequential float64 sums in observation order, max from 0 with >, the first
observation among equal maxima.

Tolerance (derived): a sum of n non-negative doubles in any order errs by at
most (n - 1) 2^-53 relative; the sequential restatement errs by the same
bound and each side divides once, so |avg_gpu - avg_ref| <= n 2^-52 avg_ref
with n the segment's count.  Counts, maxima and arg-maxima are compared
exactly, on inputs asserted to have no ties."""
import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd._lib import MmbaError
from mayamatchmovesolver_amd.solver import Context, Solver, debug_error_metrics

from test_gpu_sharded import CASES, run_sharded

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in abi.MmbaErrorMetrics._fields_]


def restate(F, K, mk, fr, ed):
    """fill + create_deviation_attrs_on_node, observation by observation."""
    cnt = np.zeros(F + K, dtype=np.int32)
    tot = np.zeros(F + K)
    mx = np.zeros(F + K)
    arg = np.full(F + K, -1, dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for i in range(len(ed)):
            d = ed[i]
            for g, key in ((fr[i], mk[i]), (F + mk[i], fr[i])):
                cnt[g] += 1
                tot[g] += d
                if d > mx[g]:
                    mx[g] = d
                    arg[g] = key
        avg = np.where(cnt > 0, tot / np.maximum(cnt, 1), 0.0)
    return {"frame_count": cnt[:F], "frame_avg": avg[:F], "frame_max": mx[:F],
            "frame_max_marker": arg[:F], "marker_count": cnt[F:], "marker_avg": avg[F:],
            "marker_max": mx[F:], "marker_max_frame": arg[F:]}


def assert_no_ties(F, K, mk, fr, ed):
    """Every segment's positive maximum is reached by one observation."""
    mk, fr, ed = np.asarray(mk), np.asarray(fr), np.asarray(ed)
    for keys, n in ((fr, F), (mk, K)):
        for g in range(n):
            v = ed[keys == g]
            if v.size and np.nanmax(v) > 0:
                assert np.count_nonzero(v == np.nanmax(v)) == 1, g


def compare(got, ref, exact_avg=False):
    for ax, arg in (("frame", "frame_max_marker"), ("marker", "marker_max_frame")):
        np.testing.assert_array_equal(got[ax + "_count"], ref[ax + "_count"])
        np.testing.assert_array_equal(got[ax + "_max"], ref[ax + "_max"])
        np.testing.assert_array_equal(got[arg], ref[arg])
        a, b, n = got[ax + "_avg"], ref[ax + "_avg"], ref[ax + "_count"]
        if exact_avg:
            np.testing.assert_array_equal(a, b)
            continue
        fin = np.isfinite(b)
        np.testing.assert_array_equal(a[~fin], b[~fin])  # NaN and inf propagate alike
        err = np.abs(a[fin] - b[fin])
        bound = n[fin] * 2.0 ** -52 * b[fin]
        print(ax, "avg: max err / bound", np.max(err / np.maximum(bound, 1e-300), initial=0.0))
        assert np.all(err <= bound), (ax, np.max(err - bound))


def same_bits(a, b, names=NAMES):
    for n in names:
        assert a[n].tobytes() == b[n].tobytes(), n


def marker_major(F, K, seen):
    """errorToMarkerList's order: marker by marker, frames ascending."""
    mk, fr = [], []
    for k in range(K):
        for f in range(F):
            if seen(k, f):
                mk.append(k)
                fr.append(f)
    return np.array(mk, dtype=np.int32), np.array(fr, dtype=np.int32)


def decades(n, seed):
    """Deviations over 12 decades: the order of a sum matters at the bound."""
    rng = np.random.default_rng(seed)
    return 10.0 ** rng.uniform(-6.0, 6.0, n)


L_FRAMES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 129, 257, 1000]
N_MARKERS = [0, 1, 63, 64, 65, 300]
# frame segments at the lengths where the lane-group width changes (16 | 17,
# 128 | 129) and one past 2^11 entries
L_WIDTHS = [15, 16, 17, 127, 128, 129, 2100]


@pytest.fixture(scope="module")
def case_i():
    F, K = 12, 1000
    mk, fr = marker_major(F, K, lambda k, f: k < L_FRAMES[f])
    ed = decades(mk.size, 11)
    assert_no_ties(F, K, mk, fr, ed)
    return F, K, mk, fr, ed, restate(F, K, mk, fr, ed)


def test_hook_frames_long_markers_short(case_i, gpu_ctx):
    F, K, mk, fr, ed, ref = case_i
    # marker k is seen in the frames with L > k: 11 of them down to 1 (the
    # last frame sees every marker; empty marker segments: the next tests)
    assert sorted(set(ref["marker_count"])) == list(range(1, 12))
    assert list(ref["frame_count"]) == L_FRAMES
    got = debug_error_metrics(gpu_ctx, F, K, mk, fr, ed)
    compare(got, ref)
    # (iv) the same list again: the same bits
    same_bits(debug_error_metrics(gpu_ctx, F, K, mk, fr, ed), got)


def test_hook_markers_long_frames_short(gpu_ctx):
    F, K = 300, 6
    mk, fr = marker_major(F, K, lambda k, f: f < N_MARKERS[k])
    ed = decades(mk.size, 12)
    assert_no_ties(F, K, mk, fr, ed)
    ref = restate(F, K, mk, fr, ed)
    assert list(ref["marker_count"]) == N_MARKERS
    compare(debug_error_metrics(gpu_ctx, F, K, mk, fr, ed), ref)


def test_hook_width_thresholds(gpu_ctx):
    F, K = len(L_WIDTHS), max(L_WIDTHS)
    mk, fr = marker_major(F, K, lambda k, f: k < L_WIDTHS[f])
    ed = decades(mk.size, 13)
    assert_no_ties(F, K, mk, fr, ed)
    ref = restate(F, K, mk, fr, ed)
    assert list(ref["frame_count"]) == L_WIDTHS
    compare(debug_error_metrics(gpu_ctx, F, K, mk, fr, ed), ref)


def test_hook_nan_inf_zero_ties(gpu_ctx):
    """A NaN propagates into avg and never becomes max; an all-zero segment
    and an unobserved one have max 0 and arg-max -1; among equal maxima the
    lowest observation index wins (lowest marker of a frame, lowest frame of a
    marker)."""
    nan, inf = float("nan"), float("inf")
    # rows: markers 0..4 (marker 5 unobserved); columns: frames 0..3 (frame 4 unobserved)
    table = [[1.0, 2.0, 0.0, inf],
             [nan, 5.0, 0.0, 1.0],
             [3.0, 5.0, 0.0, 2.0],
             [7.0, 1.0, 0.0, 7.0],
             [0.5, 4.0, 0.0, 7.0]]
    F, K = 5, 6
    mk, fr = marker_major(F, K, lambda k, f: k < 5 and f < 4)
    ed = np.array([table[k][f] for k, f in zip(mk, fr)])
    got = debug_error_metrics(gpu_ctx, F, K, mk, fr, ed)
    ref = restate(F, K, mk, fr, ed)
    for n in NAMES:
        np.testing.assert_array_equal(got[n], ref[n], err_msg=n)  # (NaN == NaN here)
    assert np.isnan(got["frame_avg"][0]) and np.isnan(got["marker_avg"][1])
    assert got["frame_max"][0] == 7.0 and got["frame_max_marker"][0] == 3
    assert got["marker_max"][1] == 5.0 and got["marker_max_frame"][1] == 1
    assert got["frame_avg"][3] == inf and got["frame_max"][3] == inf
    assert got["frame_max_marker"][3] == 0
    # ties: frame 1 (markers 1 and 2 at 5.0), marker 3 (frames 0 and 3 at 7.0)
    assert got["frame_max_marker"][1] == 1 and got["marker_max_frame"][3] == 0
    # the all-zero frame 2 and the unobserved frame 4 / marker 5
    for f in (2, 4):
        assert (got["frame_avg"][f], got["frame_max"][f], got["frame_max_marker"][f]) == (0, 0, -1)
    assert list(got["frame_count"]) == [5, 5, 5, 5, 0]
    assert (got["marker_count"][5], got["marker_avg"][5], got["marker_max"][5],
            got["marker_max_frame"][5]) == (0, 0, 0, -1)


def test_hook_null_members_and_bad_keys(case_i, gpu_ctx):
    F, K, mk, fr, ed, ref = case_i
    full = debug_error_metrics(gpu_ctx, F, K, mk, fr, ed)
    for names in (["frame_avg"], ["marker_max_frame", "frame_count"], []):
        part = debug_error_metrics(gpu_ctx, F, K, mk, fr, ed, members=names)
        assert sorted(part) == sorted(names)
        same_bits(part, full, names)
    bad = fr.copy()
    bad[3] = F
    with pytest.raises(MmbaError) as e:
        debug_error_metrics(gpu_ctx, F, K, mk, bad, ed)
    assert e.value.code == abi.MMBA_ERR_INVALID


# --- plans -------------------------------------------------------------------

SCENES = {
    "c2": lambda: S.make_config(1, frames=8, scale=0.1),
    "c4": lambda: S.make_config(3, frames=8, scale=0.001),
    "c5": lambda: S.make_config(4, frames=8, scale=0.05),
    "c5_rs": lambda: S.make_config(4, frames=8, scale=0.05, rolling_shutter=0.5),
    "enabled": lambda: S.known_scene("enabled_multi_f5"),
    "b4": lambda: S.b4_scene(),
}


def scene_options(name, prob):
    if name == "enabled":
        return S.known_options("enabled_multi_f5")
    return S.config_options(prob, iterations=8)


def restate_problem(prob, ed):
    mk, fr = np.asarray(prob.obs_marker), np.asarray(prob.obs_frame)
    assert_no_ties(prob.num_frames, prob.num_markers, mk, fr, ed)
    return restate(prob.num_frames, prob.num_markers, mk, fr, ed)


@pytest.mark.parametrize("name", list(SCENES))
def test_plan_metrics(name, gpu_ctx):
    prob = SCENES[name]()
    opt = scene_options(name, prob)
    if name == "c5":  # two cameras per frame: a frame's segment spans two camera-frames
        assert len(set(zip(np.asarray(prob.obs_frame),
                           np.asarray(prob.mkr_cam)[np.asarray(prob.obs_marker)]))) == \
            2 * prob.num_frames
    if name == "enabled":  # markers with disabled frames
        assert prob.num_obs < prob.num_markers * prob.num_frames
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        with pytest.raises(MmbaError) as e:  # before any call
            s.error_metrics()
        assert e.value.code == abi.MMBA_ERR_INVALID
        _f, _eu, ed, _st = s.measure(prob.x0)
        got = s.error_metrics()
        compare(got, restate_problem(prob, ed))
        same_bits(s.error_metrics(), got)
        np.testing.assert_array_equal(s.outputs()[2], ed)  # the list it reduced
        out = s.solve()
        got = s.error_metrics()
        compare(got, restate_problem(prob, out.err_dist))
        np.testing.assert_array_equal(s.outputs()[2], out.err_dist)
        # device-resident outputs: the same solve, the same dict, no lists
        dev = s.solve(fetch=False, metrics=True)
        assert dev.err_dist is None and dev.fvec is None
        same_bits(dev.metrics, got)
        for names in (["marker_avg"], ["frame_max", "frame_max_marker"]):
            same_bits(s.error_metrics(members=names), got, names)
        s.reproject(prob.x0)
        with pytest.raises(MmbaError) as e:
            s.error_metrics()
        assert e.value.code == abi.MMBA_ERR_INVALID
        s.measure(prob.x0)
        s.error_metrics()
        try:
            s.solve_per_frame()
        except MmbaError as pf:  # (a scene whose parameters chain the frames)
            assert pf.code == abi.MMBA_ERR_UNSUPPORTED
        with pytest.raises(MmbaError) as e:
            s.error_metrics()
        assert e.value.code == abi.MMBA_ERR_INVALID
    finally:
        s.close()


def test_b4_keys_follow_marker_i(gpu_ctx):
    """On a B4-remapped plan observation i is keyed by obs_marker[i], not by
    the flat marker whose geometry it borrows."""
    prob = S.b4_scene()
    opt = S.config_options(prob, iterations=8)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        ed = s.measure(prob.x0)[2]
        got = s.error_metrics()
    finally:
        s.close()
    mk = np.asarray(prob.obs_marker)
    for k in range(prob.num_markers):
        assert got["marker_max"][k] == np.max(ed[mk == k])
        assert got["marker_count"][k] == np.count_nonzero(mk == k)


# --- shards ------------------------------------------------------------------

def unsharded(prob, opt, ctx):
    s = Solver(prob, opt, context=ctx)
    try:
        ed = s.measure(prob.x0)[2]
        return ed, s.error_metrics()
    finally:
        s.close()


def measure_metrics(s):
    s.measure(s.problem.x0)
    return s.error_metrics(), s.kernel_stats()["shards_replicated"]


def check_sharded(got, ref, ed, prob):
    same_bits(got, ref, [n for n in NAMES if n.startswith("frame")])
    compare(got, ref)
    compare(got, restate_problem(prob, ed))


@pytest.fixture(scope="module")
def shard_case(gpu_ctx):
    idx, kw, n = CASES[0]
    prob = S.make_config(idx, **kw)
    opt = S.config_options(prob)
    ed, ref = unsharded(prob, opt, gpu_ctx)
    return prob, opt, n, ed, ref


def test_sharded_collective(shard_case):
    prob, opt, n, ed, ref = shard_case
    outs = run_sharded(prob, opt, n, call=measure_metrics)
    assert [rep for _m, rep in outs] == [0] * n
    # tracks cross the boundary: a marker observed on both shards
    from mayamatchmovesolver_amd.solver import shard_layout
    b = shard_layout(prob, n)[0][1]
    fr, mk = np.asarray(prob.obs_frame), np.asarray(prob.obs_marker)
    assert set(mk[fr < b]) & set(mk[fr >= b])
    for m, _rep in outs[1:]:
        same_bits(m, outs[0][0])
    check_sharded(outs[0][0], ref, ed, prob)


def test_multi_device_plan(shard_case):
    prob, opt, n, ed, ref = shard_case
    ctx = Context.multi([0] * n)
    try:
        s = Solver(prob, opt, context=ctx)
        try:
            assert s.num_shards == n
            with pytest.raises(MmbaError) as e:
                s.error_metrics()
            assert e.value.code == abi.MMBA_ERR_INVALID
            got, rep = measure_metrics(s)
            assert rep == 0
            same_bits(s.error_metrics(), got)
        finally:
            s.close()
    finally:
        ctx.close()
    check_sharded(got, ref, ed, prob)


def test_replicated_rolling_shutter(gpu_ctx):
    prob = S.make_config(4, frames=12, scale=0.05, rolling_shutter=0.5)
    opt = S.config_options(prob, iterations=6)
    _ed, ref = unsharded(prob, opt, gpu_ctx)
    outs = run_sharded(prob, opt, 2, call=measure_metrics)
    assert [rep for _m, rep in outs] == [1, 1]
    for m, _rep in outs:
        same_bits(m, ref)
