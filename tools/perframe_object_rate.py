"""Frames/s of a per-frame object solve (synthetic.object_scene, the camera
fixed, six pose parameters per frame), one process:

  one_launch        Solver(prob, opt, per_frame=True).solve_per_frame() on one
                    cached plan: every frame in one k_batch_lm launch (the
                    object form, mmba_batch_obj.hip)
  per_frame_plans   solve_per_frame(prob, opt, max_concurrency=8) with
                    MMBA_PATH_PERFRAME_BATCH = 0: one plan per frame on eight
                    host threads -- what a library without the object form
                    runs for this scene (the yardstick)

Each: --warmup calls, then --calls timed calls; frames/s from the median call
time (the one-launch call time is the launch plus the copies of x and the
results: the plan's kernel statistics do not cover k_batch_lm).  Both paths'
results are compared per frame.  Prints each timing, then one JSON line."""
import argparse
import json
import time

import numpy as np

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, set_path, solve_per_frame

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=240)
ap.add_argument("--bundles", type=int, default=40)
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--concurrency", type=int, default=8)
args = ap.parse_args()
assert args.calls >= 5 and args.warmup >= 2

ctx = Context(0)
prob = S.object_scene(frames=args.frames, bundles=args.bundles)
opt = S.object_options()
F = prob.num_frames


def timed(tag, call):
    for _ in range(args.warmup):
        out = call()
    ts = []
    for i in range(args.calls):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = call()
        ts.append(time.perf_counter() - t0)
        print("%-16s call %d %.3f ms %.0f frames/s" % (tag, i, 1e3 * ts[-1], F / ts[-1]),
              flush=True)
    med = float(np.median(ts))
    return out, dict(median_ms=round(1e3 * med, 3), min_ms=round(1e3 * min(ts), 3),
                     max_ms=round(1e3 * max(ts), 3), frames_per_s=round(F / med, 1))


sv = Solver(prob, opt, context=ctx, per_frame=True)
n0 = sv.batch_launches()
(x1, r1), one = timed("one_launch", sv.solve_per_frame)
assert sv.batch_launches() == n0 + args.warmup + args.calls
sv.close()

set_path(abi.PATH_PERFRAME_BATCH, 0)
n0 = Solver.batch_launches()
(x2, r2), many = timed("per_frame_plans", lambda: solve_per_frame(
    prob, opt, max_concurrency=args.concurrency, context=ctx))
assert Solver.batch_launches() == n0
set_path(abi.PATH_PERFRAME_BATCH, -1)
ctx.close()

same = all(a["reason_number"] == b["reason_number"] and a["iterations"] == b["iterations"]
           for a, b in zip(r1, r2))
dx = float(np.max(np.abs(x1 - x2) / np.maximum(np.abs(x2), 1e-3)))
print(json.dumps(dict(frames=F, params=prob.num_params, obs=prob.num_obs,
                      evals=sum(r["function_evals"] for r in r1), one_launch=one,
                      per_frame_plans=many,
                      speedup=round(one["frames_per_s"] / many["frames_per_s"], 1),
                      same_reasons_and_counts=same, max_rel_dx=dx)))
