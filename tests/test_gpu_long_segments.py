"""The long-segment (C2-class) LM path at small shapes.

Plans with more than 1024 observations per camera-frame on average, a uniform
6 or 7 parameters per camera-frame and no global parameter form their
camera-frame normal equations with k_ne_cf_split<PC, 4, 4>: four workgroups
per camera-frame (part p takes observations o0 + 256 p + t, then every 1024th),
partial sums stored write-through, the last arriver (per camera-frame
monotonic ticket) adds them in part order and runs the lmder epilogue.  The
scenes below reach that kernel with a few thousand observations, at the
segment tails, part boundaries and empty parts where it can go wrong, and
hold the whole solve to the CPU oracle at the project's bar (1e-6 on x and on
every ||f||, test_gpu_parity.check_solve).

The oracle's own x moves by <= 3.6e-9 (||f|| by <= 5e-10) under 1-ulp
perturbations of x0 on every scene and solver type (8 seeds, as
tests/golden/envelopes.py perturbs), with the same counts, and the Jacobian
has no undetermined direction, so the 1e-6 bar applies as it stands; dropping one boundary observation moves the oracle's x by > 1e-5
(test_boundary_observation_moves_the_oracle, CPU), so a kernel that drops or
duplicates one fails the bar.

mmba_kernel_stats.ne_split_launches counts the kernel's launches on a plan:
every parity test asserts from the dispatch (Plan::jac, launch_ne) whether it
must have run.
"""
import dataclasses
import functools

import numpy as np
import pytest

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, host_array

from test_gpu_parity import check_solve

gpu = pytest.mark.gpu

LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF
SOLVER_TYPES = [pytest.param(LMDER, id="lmder"), pytest.param(LMDIF, id="lmdif")]

# name: (make_config(1, ...) keywords, observations kept per frame or None,
#        observations per frame, parameters per camera-frame)
SCENES = {
    # parts 0-3 get 257 / 256 / 256 / 256 observations plus a tail
    "even2": (dict(frames=2, scale=0.25), None, [1250, 1250], 7),
    # 26 observations past one full stride: only part 0 loops twice
    "even3": (dict(frames=3, scale=0.21), None, [1050, 1050, 1050], 7),
    # frame 1: one observation in the second stride; frame 2: parts 1-3 empty
    "uneven_a": (dict(frames=3, scale=0.7), [3500, 1025, 40], [3500, 1025, 40], 7),
    # frame 1 ends one short of part 1's second stride; frame 2: 7 lanes of wave 0
    "uneven_b": (dict(frames=3, scale=0.7), [3500, 1279, 7], [3500, 1279, 7], 7),
    # 5000 observations per shard at 2 shards (> 1024 x 4 camera-frames), but 14
    # camera-frame rows per shard: the plan builder replicates it (test_two_shards);
    # shard6: 21 rows and 7500 observations per shard (> 1024 x 6), sharded
    "shard4": (dict(frames=4, scale=0.5), None, [2500] * 4, 7),
    "shard6": (dict(frames=6, scale=0.5), None, [2500] * 6, 7),
    # focal length locked: the <6, 4, 4> instantiation
    "pc6": (dict(frames=3, scale=0.21, solve_focal=False), None, [1050, 1050, 1050], 6),
}
PARITY_SCENES = ["even2", "even3", "uneven_a", "uneven_b", "pc6"]


def keep_first(prob, keep):
    """prob with only the first keep[f] observations of frame f (observation order)."""
    idx = np.sort(np.concatenate([np.flatnonzero(prob.obs_frame == f)[:k]
                                  for f, k in enumerate(keep)]))
    return dataclasses.replace(prob, obs_marker=prob.obs_marker[idx].copy(),
                               obs_frame=prob.obs_frame[idx].copy(),
                               obs_xy=prob.obs_xy.reshape(-1, 2)[idx].ravel().copy(),
                               obs_weight=prob.obs_weight[idx].copy())


@functools.lru_cache(maxsize=None)
def scene(name):
    kw, keep, _, _ = SCENES[name]
    prob = S.make_config(1, **kw)
    return prob if keep is None else keep_first(prob, keep)


def options(prob, solver_type):
    return S.config_options(prob, solver_type=solver_type)


class OneSolve:
    """check_solve's ``oracle`` argument: the scene's one oracle solve, shared."""

    def __init__(self, ref):
        self.ref = ref

    def solve(self, prob, opt):
        return self.ref


@pytest.fixture(scope="module")
def ref(oracle):
    """(scene name, solver type) -> the oracle's solve, computed once and left unchanged."""
    cache = {}

    def get(name, solver_type):
        key = (name, solver_type)
        if key not in cache:
            prob = scene(name)
            cache[key] = oracle.solve(prob, options(prob, solver_type))
            for a in cache[key]:
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        return OneSolve(cache[key])
    return get


def rel_x(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-3)))


def solve_with_stats(s, **kw):
    out = s.solve(**kw)
    out.kernel_stats = s.kernel_stats()
    return out


def gpu_solve(prob, opt, ctx, **kw):
    s = Solver(prob, opt, context=ctx)
    try:
        return solve_with_stats(s, **kw)
    finally:
        s.close()


def assert_same_bits(a, b, what=""):
    for k in ("x", "fnorm_trace", "fvec", "err_dist"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg="%s %s" % (what, k))


# ---- CPU: the scenes are what the header says, and keep their power ----

@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_shapes(name):
    """Observations per frame, parameters per camera-frame and launch_ne's
    split condition (M > 1024 ncf; per shard of two for shard4 / shard6, even
    counting every camera-frame) as the table above states them."""
    _, _, counts, pc = SCENES[name]
    prob = scene(name)
    F = prob.num_frames
    assert np.bincount(prob.obs_frame, minlength=F).tolist() == counts
    assert prob.num_params == pc * F
    assert sorted(np.bincount(prob.param_frame, minlength=F).tolist()) == [pc] * F
    assert prob.num_bundles > 0 and prob.num_obs > 1024 * F
    if name in ("shard4", "shard6"):
        assert prob.num_obs // 2 > 1024 * F


BOUNDARY = [pytest.param(1, -1, id="last_of_frame1"), pytest.param(1, 1024, id="frame1_1024"),
            pytest.param(0, -1, id="last_of_frame0"), pytest.param(0, 1023, id="frame0_1023"),
            pytest.param(2, -1, id="last_of_frame2")]


@pytest.fixture(scope="module")
def uneven_a_base(oracle):
    prob = scene("uneven_a")
    return oracle.solve(prob, options(prob, LMDER))


@pytest.mark.parametrize("frame,index", BOUNDARY)
def test_boundary_observation_moves_the_oracle(frame, index, oracle, uneven_a_base):
    """One segment-tail or part-boundary observation of uneven_a given zero
    weight moves the oracle's x by more than 1e-5 (measured: >= 3.1e-5), ten
    times the parity bar: a normal-equation kernel that drops or duplicates
    one such observation cannot pass test_parity.  This is what keeps the
    scenes' power if ``synthetic`` changes."""
    prob = scene("uneven_a")
    i = int(np.flatnonzero(prob.obs_frame == frame)[index])
    w = prob.obs_weight.copy()
    assert w[i] != 0.
    w[i] = 0.
    dropped = dataclasses.replace(prob, obs_weight=w)
    x = oracle.solve(dropped, options(dropped, LMDER))[0]
    moved = rel_x(x, uneven_a_base[0])
    print("uneven_a frame %d index %d zero-weighted: oracle x moves %.3g" % (frame, index, moved))
    assert moved > 1e-5


# ---- GPU ----

_parity_x = {}  # (scene, solver type, split pin) -> x, for the split-versus-unsplit report


@gpu
@pytest.mark.parametrize("split", [pytest.param(-1, id="split"), pytest.param(0, id="unsplit")])
@pytest.mark.parametrize("solver_type", SOLVER_TYPES)
@pytest.mark.parametrize("name", PARITY_SCENES)
def test_parity(name, solver_type, split, ref, gpu_ctx, paths):
    """Whole solve against the oracle at 1e-6 (counts, every ||f||, x) through
    k_ne_cf_split<PC, 4, 4> (default) and, with PATH_NE_CF_SPLIT = 0, through
    the unsplit k_ne_cf_u<PC, 4, 0> on the same scene (summation order is the
    only difference).

    The counter: Plan::jac fuses the lmder bookkeeping whenever the LM loop
    calls it (``lm`` non-null) on an epilogue-fusable plan without attribute
    rows -- lmdif's loop passes ``lm`` exactly as lmder's does and ``central``
    plays no part -- so both solver types hand launch_ne the partial buffers
    and every Jacobian of the solve must count: ne_split_launches equals the
    outer iterations by default and is 0 with the path pinned off."""
    if split >= 0:
        paths(abi.PATH_NE_CF_SPLIT, split)
    prob = scene(name)
    out, (_, rr) = check_solve(prob, options(prob, solver_type), ref(name, solver_type), gpu_ctx,
                               run=solve_with_stats)
    n = out.kernel_stats["ne_split_launches"]
    if split == 0:
        assert n == 0
    else:
        assert n > 0 and n == rr.outer_iterations
    _parity_x[(name, solver_type, split)] = out.x
    other = _parity_x.get((name, solver_type, -1 - split))
    if other is not None:
        print("split vs unsplit x: %s type %d: %.3g" % (name, solver_type, rel_x(out.x, other)))


_default_runs = {}


def default_run(name, solver_type, ctx):
    key = (name, solver_type)
    if key not in _default_runs:
        prob = scene(name)
        _default_runs[key] = gpu_solve(prob, options(prob, solver_type), ctx)
    return _default_runs[key]


@gpu
@pytest.mark.parametrize("key,same_bits", [(abi.PATH_RED_BD, True), (abi.PATH_TRIAL_RECORDS, True)],
                         ids=["red_bd", "trial_records"])
@pytest.mark.parametrize("solver_type", SOLVER_TYPES)
@pytest.mark.parametrize("name", ["uneven_a", "pc6"])
def test_pinned_forms(name, solver_type, key, same_bits, ref, gpu_ctx, paths):
    """The C2 route's alternatives, each pinned off and held to the oracle at
    1e-6: the epilogue's reduction as its own k_reduce_multi launch instead of
    riding in the one-launch block-diagonal solve (PATH_RED_BD = 0:
    k_bd_direct's extra workgroups run "k_reduce_multi's arithmetic,
    reduce_row_block"), and the trial point's records from k_trial_prep +
    k_records instead of k_trial_prep_rec (PATH_TRIAL_RECORDS = 0: "its base
    and variant records, as k_records builds them").  The code describes both
    as the same operations, so x, the ||f|| trace, fvec and err_dist are also
    bit-equal to the default run."""
    base = default_run(name, solver_type, gpu_ctx)
    paths(key, 0)
    prob = scene(name)
    out, _ = check_solve(prob, options(prob, solver_type), ref(name, solver_type), gpu_ctx,
                         run=solve_with_stats)
    assert out.kernel_stats["ne_split_launches"] == base.kernel_stats["ne_split_launches"] > 0
    if same_bits:
        assert_same_bits(out, base, "pin %d = 0 against the default" % key)


@gpu
@pytest.mark.parametrize("pre", [0, 1])
@pytest.mark.parametrize("solver_type", SOLVER_TYPES)
@pytest.mark.parametrize("name", ["uneven_a", "pc6"])
def test_kernel_handback(name, solver_type, pre, ref, gpu_ctx, paths):
    """Page-locked output lists through k_handback_host's host-mapped stores
    (PATH_HANDBACK_DMA = 0) without and with its speculative launch behind
    each decided trial (PATH_PRE_HANDBACK = 0 / 1): the solve against the
    oracle at 1e-6, and the lists -- moved, not computed -- equal to the
    default run's, every entry rewritten."""
    base = default_run(name, solver_type, gpu_ctx)
    paths(abi.PATH_HANDBACK_DMA, 0)
    paths(abi.PATH_PRE_HANDBACK, pre)
    prob = scene(name)
    m, M = prob.num_residuals, prob.num_obs
    pin = (host_array(m), host_array(m), host_array(M))
    for a in pin:
        a[:] = np.nan
    out, _ = check_solve(prob, options(prob, solver_type), ref(name, solver_type), gpu_ctx,
                         run=lambda s: solve_with_stats(s, out=pin))
    assert out.kernel_stats["ne_split_launches"] > 0
    handed = out.kernel_stats["pre_handbacks"]
    if pre == 0:
        assert handed == 0
    elif out.result["reason_number"] in (1, 2, 3, 5, 6, 7, 8):
        assert handed == 1  # ended by the tests after a trial: stored behind it
    np.testing.assert_array_equal(pin[0], base.fvec)
    np.testing.assert_array_equal(pin[1], base.err_user)
    np.testing.assert_array_equal(pin[2], base.err_dist)
    np.testing.assert_array_equal(out.x, base.x)


@gpu
@pytest.mark.parametrize("solver_type", SOLVER_TYPES)
@pytest.mark.parametrize("name", ["uneven_b", "even2"])
def test_deterministic_and_ticket_reuse(name, solver_type, gpu_ctx):
    """Three solves on one plan (the per-camera-frame tickets keep counting:
    last arriver when old % 4 == 3) and one on a fresh plan: x, the ||f||
    trace, fvec and err_dist bit-identical -- the part-order sum does not
    depend on which workgroup arrives last, nor on what earlier launches left
    in the tickets and partial buffers."""
    prob = scene(name)
    opt = options(prob, solver_type)
    s = Solver(prob, opt, context=gpu_ctx)
    try:
        runs = [solve_with_stats(s) for _ in range(3)]
    finally:
        s.close()
    fresh = gpu_solve(prob, opt, gpu_ctx)
    per_solve = fresh.kernel_stats["ne_split_launches"]
    assert per_solve == fresh.result["outer_iterations"] > 1
    assert [r.kernel_stats["ne_split_launches"] for r in runs] == [k * per_solve for k in (1, 2, 3)]
    for k, r in enumerate(runs[1:] + [fresh]):
        assert_same_bits(r, runs[0], "run %d" % (k + 1))


@gpu
@pytest.mark.parametrize("name", ["uneven_a", "pc6"])
def test_interleaved_measure_and_jacobian(name, gpu_ctx):
    """solve, measure, jacobian, solve on one plan: neither call runs the
    split kernel (measure forms no Jacobian; the dense Jacobian hook calls
    Plan::jac without the LM state, which does not fuse), so the counter
    stands still between the solves, and the second solve finds tickets and
    partial buffers it can use: bit-equal to the first."""
    prob = scene(name)
    s = Solver(prob, options(prob, LMDER), context=gpu_ctx)
    try:
        first = solve_with_stats(s)
        s.measure(prob.x0 + 1e-3)
        J = s.jacobian(prob.x0 + 2e-3)
        assert np.all(np.isfinite(J)) and np.any(J)
        assert s.kernel_stats()["ne_split_launches"] == first.kernel_stats["ne_split_launches"] > 0
        second = solve_with_stats(s)
    finally:
        s.close()
    assert second.kernel_stats["ne_split_launches"] == 2 * first.kernel_stats["ne_split_launches"]
    assert_same_bits(second, first, "second solve")


@gpu
@pytest.mark.parametrize("name,shards", [("shard4", None), ("shard6", 2)])
def test_two_shards(name, shards, ref):
    """A plan on a two-device context (the device named twice: the in-process
    transport) against the oracle at 1e-6: counts, every ||f||, x.

    shard4 (2 frames, 5000 observations per shard) turns out not to shard: the
    plan builder wants 2 bw + 8 = 20 camera-frame rows per shard and two
    frames have 14, so it is replicated and its first shard solves the whole
    problem (shards_replicated = 1, one shard).  shard6 (3 frames, 21 rows and
    7500 observations per shard, more than 1024 x all 6 camera-frames) is
    sharded, and is the one that runs a shard's normal equations with the
    other shard's camera-frames in the grid (the ``own_cf`` early return).
    What the split counter reads (a group reports its first shard's) is
    printed, not asserted."""
    prob = scene(name)
    ctx = Context.multi([0, 0])
    try:
        assert ctx.num_devices == 2
        seen = {}

        def run(s):
            seen["shards"] = s.num_shards
            return solve_with_stats(s)
        out, (_, rr) = check_solve(prob, options(prob, LMDER), ref(name, LMDER), ctx, run=run)
    finally:
        ctx.close()
    print("%s on 2 devices: %d shard(s), shards_replicated %d, ne_split_launches %d, outer "
          "iterations %d" % (name, seen["shards"], out.kernel_stats["shards_replicated"],
                             out.kernel_stats["ne_split_launches"], rr.outer_iterations))
    if shards is not None:
        assert seen["shards"] == shards and out.kernel_stats["shards_replicated"] == 0
