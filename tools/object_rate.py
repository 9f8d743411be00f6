"""LM it/s and the Jacobian / residual pass times of object-tracking solves
(synthetic.object_scene), one process.

Default: an object shot of a size a user runs -- 240 frames, 200 bundles under
the object -- once with the camera fixed and once with it solved, each with
the object records (MMBA_PATH_OBJ_REC = 1) and with the chain walk (0).  The
two plans are timed alternately, every timing a window of at least
--min-seconds of back-to-back solves after a warm-up, --repeats times; then
kernel_stats' jac_ms_avg / resid_ms_avg of each from a timed pass of its own.

--small F: the small scene instead (F frames, 6 bundles, camera fixed), with
the object parameters as global parameters (the form of every plan that has
no in-block form: 5 frames is the largest a library without it builds) and,
where the library has the key, in the camera-frame blocks (MMBA_PATH_OBJ_CF =
1), alternated the same way.

Prints each timing, then median and min..max per plan, then one JSON line."""
import argparse
import json
import time

import numpy as np

from mayamatchmovesolver_amd import abi, synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, set_path

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=240)
ap.add_argument("--bundles", type=int, default=200)
ap.add_argument("--small", type=int, default=0)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--min-seconds", type=float, default=1.0)
args = ap.parse_args()

OBJ_CF = getattr(abi, "PATH_OBJ_CF", None)
OBJ_REC = getattr(abi, "PATH_OBJ_REC", None)
ctx = Context(0)
report = {}


def plan(prob, opt, pins):
    for k, v in pins.items():
        set_path(k, v)
    try:
        return Solver(prob, opt, context=ctx)
    finally:
        for k in pins:
            set_path(k, -1)


def window(sv):
    """Back-to-back solves for at least --min-seconds: (iterations, seconds, solves)."""
    ctx.synchronize()
    t0 = time.perf_counter()
    it = n = 0
    while True:
        it += sv.solve(fetch=False).result["outer_iterations"]
        n += 1
        if n % 4 == 0 or n == 1:
            ctx.synchronize()
            if time.perf_counter() - t0 >= args.min_seconds:
                break
    ctx.synchronize()
    return it, time.perf_counter() - t0, n


def compare(tag, prob, opt, plans):
    svs = {k: plan(prob, opt, pins) for k, pins in plans.items()}
    rates = {k: [] for k in svs}
    iters = {}
    for k, sv in svs.items():  # warm-up
        for _ in range(3):
            iters[k] = sv.solve(fetch=False).result["outer_iterations"]
    for rep in range(args.repeats):
        for k, sv in svs.items():
            it, dt, n = window(sv)
            rates[k].append(it / dt)
            print("%s rep %d %-10s %.3f ms/solve %.1f it/s (%d solves)" %
                  (tag, rep, k, 1e3 * dt / n, it / dt, n), flush=True)
    out = dict(frames=prob.num_frames, params=prob.num_params, obs=prob.num_obs)
    for k, sv in svs.items():
        sv.set_timing(True)
        for _ in range(4):
            sv.solve(fetch=False)
        st = sv.kernel_stats()
        v = rates[k]
        out[k] = dict(median=round(float(np.median(v)), 1), min=round(min(v), 1),
                      max=round(max(v), 1), iterations=iters[k],
                      reduced_dim=st["reduced_dim"],
                      jac_ms_avg=round(st["jac_ms_avg"], 4),
                      resid_ms_avg=round(st["resid_ms_avg"], 4))
        print("%s %-10s median %.1f it/s (%.1f .. %.1f), %d iterations/solve, jac %.4f ms, "
              "resid %.4f ms" % (tag, k, np.median(v), min(v), max(v), iters[k],
                                 st["jac_ms_avg"], st["resid_ms_avg"]), flush=True)
        sv.close()
    report[tag] = out


if args.small:
    prob = S.object_scene(frames=args.small, bundles=6)
    plans = {"globals": {} if OBJ_CF is None else {OBJ_CF: 0}}
    if OBJ_CF is not None:
        plans["in_block"] = {OBJ_CF: 1}
    compare("small_f%d" % args.small, prob, S.object_options(), plans)
else:
    for cam in (False, True):
        prob = S.object_scene(frames=args.frames, bundles=args.bundles, solve_camera=cam)
        compare("f%d_b%d_%s" % (args.frames, args.bundles, "cam_solved" if cam else "cam_fixed"),
                prob, S.object_options(), {"records": {OBJ_REC: 1}, "chain_walk": {OBJ_REC: 0}})
ctx.close()
print(json.dumps(report))
