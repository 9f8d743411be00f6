"""What a re-solve with nudged markers pays before its solve starts, one
process, on the synthetic configs (default: full C4 and full C2):

  plan_create   Solver(prob, opt): mmba_plan_create alone -- what a changed
                obs_xy / obs_weight cost while both were part of the shim's
                cache key
  refresh       set_attr_values + set_marker_values on the cached plan -- what
                they cost now (validation, packing, the square roots of the
                weights, one upload per array, one k_marker_set launch)

Each: --warmup calls, then --calls timed calls, the median.  After the timed
refreshes one solve on the refreshed plan is compared, bit for bit, with one on
a plan freshly built from the same values.  Prints each timing, then one JSON
line per config."""
import argparse
import dataclasses
import json
import time

import numpy as np

from mayamatchmovesolver_amd import synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver

ap = argparse.ArgumentParser()
ap.add_argument("--configs", type=int, nargs="+", default=[3, 1],
                help="BASELINE.json configs index (3: C4, 1: C2)")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--iterations", type=int, default=2, help="of the compared solves")
args = ap.parse_args()
assert args.calls >= 5 and args.warmup >= 2

ctx = Context(0)


def timed(tag, call):
    for _ in range(args.warmup):
        call()
    ts = []
    for i in range(args.calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t0)
        print("%-12s call %d %.3f ms" % (tag, i, 1e3 * ts[-1]), flush=True)
    return dict(median_ms=round(1e3 * float(np.median(ts)), 3), min_ms=round(1e3 * min(ts), 3),
                max_ms=round(1e3 * max(ts), 3))


for index in args.configs:
    prob = S.make_config(index, scale=args.scale)
    opt = S.config_options(prob, iterations=args.iterations)
    rng = np.random.Generator(np.random.PCG64(index))
    M = prob.num_obs
    p2 = dataclasses.replace(prob, obs_xy=prob.obs_xy + 1e-3 * rng.standard_normal(2 * M),
                             obs_weight=prob.obs_weight * rng.uniform(0.5, 2.0, M))
    tag = "C%d" % (index + 1)
    print("%s: %d frames, %d observations, %d parameters" %
          (tag, prob.num_frames, M, prob.num_params), flush=True)

    def create():
        Solver(prob, opt, context=ctx).close()

    created = timed("plan_create", create)

    sv = Solver(prob, opt, context=ctx)
    sv.solve()  # a cached plan has solved before

    def refresh():
        sv.set_attr_values(p2.attr_values)
        sv.set_marker_values(p2.obs_xy, p2.obs_weight, p2.mkr_frame_xy)

    refreshed = timed("refresh", refresh)
    got = sv.solve()
    sv.close()
    fresh_sv = Solver(p2, opt, context=ctx)
    want = fresh_sv.solve()
    fresh_sv.close()
    same = bool(np.array_equal(got.x, want.x) and np.array_equal(got.fvec, want.fvec) and
                np.array_equal(got.fnorm_trace, want.fnorm_trace))
    print(json.dumps(dict(config=tag, scale=args.scale, frames=int(prob.num_frames), obs=M,
                          params=prob.num_params, upload_mb=round(24e-6 * M, 2),
                          plan_create=created, refresh=refreshed,
                          ratio=round(created["median_ms"] / refreshed["median_ms"], 1),
                          refreshed_solve_equals_fresh=same)), flush=True)
ctx.close()
