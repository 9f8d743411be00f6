"""LM it/s of repeated solves on the full C2 and C4 scenes, one process, three
ways of getting the results out, alternated over several repeats:
  (a) lists   -- the three per-residual lists handed back into page-locked arrays
  (b) device  -- solve(fetch=False): everything stays in HBM
  (c) metrics -- solve(fetch=False) + error_metrics(): per-frame / per-marker
                 deviation metrics reduced on the device
Prints each repeat, then median and min..max per mode, then one JSON line.
With --metrics-only N: N measure + error_metrics calls on one config and
nothing else (a kernel trace of its own)."""
import argparse
import json
import time

import numpy as np

from mayamatchmovesolver_amd import synthetic as S
from mayamatchmovesolver_amd.solver import Context, Solver, host_array

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="1,3")
ap.add_argument("--steps", default="200,20", help="solves per timing, one per config")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--metrics-only", type=int, default=0)
args = ap.parse_args()

ctx = Context(0)
report = {}
cfgs = [int(c) for c in args.configs.split(",")]
steps_of = dict(zip(cfgs, [int(v) for v in args.steps.split(",")]))
for cfg in cfgs:
    steps = steps_of.get(cfg, 20)
    prob = S.make_config(cfg)
    opt = S.config_options(prob)
    sv = Solver(prob, opt, context=ctx)
    m, M = prob.num_residuals, prob.num_obs
    if args.metrics_only:
        sv.measure(prob.x0)
        for _ in range(args.metrics_only):
            sv.error_metrics()
        sv.close()
        continue
    outs = (host_array(m), host_array(m), host_array(M))
    modes = {
        "lists": lambda: sv.solve(out=outs),
        "device": lambda: sv.solve(fetch=False),
        "metrics": lambda: sv.solve(fetch=False, metrics=True),
    }
    for fn in modes.values():  # warm-up
        for _ in range(2):
            fn()
    rates = {k: [] for k in modes}
    for rep in range(args.repeats):
        for k, fn in modes.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            it = 0
            for _ in range(steps):
                it += fn().result["outer_iterations"]
            ctx.synchronize()
            dt = time.perf_counter() - t0
            rates[k].append(it / dt)
            print("C%d rep %d %-8s %.3f ms/solve %.1f it/s" %
                  (cfg + 1, rep, k, 1e3 * dt / steps, it / dt), flush=True)
    # the metrics call alone, behind a solve that left its outputs in HBM
    sv.solve(fetch=False)
    t0 = time.perf_counter()
    for _ in range(50):
        sv.error_metrics()
    call_us = 1e6 * (time.perf_counter() - t0) / 50
    report["C%d" % (cfg + 1)] = dict(
        frames=prob.num_frames, markers=prob.num_markers, obs=M, steps=steps,
        error_metrics_call_us=round(call_us, 1),
        **{k: dict(median=round(float(np.median(v)), 1), min=round(min(v), 1),
                   max=round(max(v), 1)) for k, v in rates.items()})
    for k, v in rates.items():
        print("C%d %-8s median %.1f it/s (%.1f .. %.1f)" %
              (cfg + 1, k, np.median(v), min(v), max(v)), flush=True)
    print("C%d error_metrics() alone: %.1f us/call" % (cfg + 1, call_us), flush=True)
    sv.close()
ctx.close()
if report:
    print(json.dumps(report))
