#!/usr/bin/env python3
"""The oracle's own x envelope on the per-frame object cases of
tests/test_gpu_perframe_object.py (the method of tools/object_envelope.py,
applied to tests.test_gpu_perframe.oracle_per_frame): every frame solved, then
solved again from x0 perturbed by ~1 ulp (relative 1e-15, 3 seeds); the
envelope is the largest relative change of any x component (floor 1e-3) the
frames' write-backs leave.  A case whose envelope exceeds 1e-7 cannot carry
the tests' 1e-6 bar with margin and is replaced by another seed; the bar is
not widened.

Run from the repo root (CPU only):
    python tools/perframe_object_envelope.py > profiles/r15_perframe_object/envelope.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mayamatchmovesolver_amd import synthetic as S  # noqa: E402
from oracle import refcpu as R  # noqa: E402
from tests.test_gpu_perframe import oracle_per_frame  # noqa: E402
from tests.test_perframe_object_host import CASES  # noqa: E402


def row(tag, prob, opt, after=-1, seeds=3):
    t = time.time()
    x, rr = oracle_per_frame(prob, opt, R, interrupt_after=after)
    env, x0 = 0.0, np.array(prob.x0, dtype=float)
    evals = []
    try:
        for seed in range(seeds):
            rng = np.random.default_rng(seed)
            prob.x0 = x0 * (1.0 + 1e-15 * rng.standard_normal(x0.size))
            xp, rp = oracle_per_frame(prob, opt, R, interrupt_after=after)
            env = max(env, float(np.max(np.abs(xp - x) / np.maximum(np.abs(x), 1e-3))))
            evals.append(sum(r.function_evals for r in rp))
    finally:
        prob.x0 = x0
    print("%-28s n=%3d frames=%2d solved=%2d reasons=%s better=%s evals=%4d envelope=%.1e "
          "perturbed evals=%s (%.1f s)" % (
              tag, prob.num_params, prob.num_frames, len(rr),
              "".join("%d" % r.reason_number if r.reason_number >= 0 else "i" for r in rr),
              "".join("%d" % r.error_is_better for r in rr),
              sum(r.function_evals for r in rr), env, ",".join("%d" % e for e in evals),
              time.time() - t), flush=True)
    return x


def main():
    print("# oracle x envelope, per-frame solves of the object scenes "
          "(synthetic.object_options: lmder delta 1e-4, lmdif delta 1e-8; tol 1e-6)")
    for name in sorted(CASES):
        build, kw, _sizes, after = CASES[name]
        row(name, build(), S.object_options(**kw), after)
    # the reuse test's third call: the scene written back at the first call's
    # x + 0.01 (the oracle's x stands in for the device's, equal to 1e-6)
    from tests.test_gpu_plan_cache import written_back
    prob = CASES["above_cap-dag-lmder"][0]()
    opt = S.object_options()
    x, _ = oracle_per_frame(prob, opt, R)
    row("above_cap restarted x+0.01", written_back(prob, x + 0.01), opt)
    # left out of the tests: two objects under lmdif
    row("two_objects lmdif (unused)", CASES["two_objects"][0](),
        S.object_options(solver_type=S.abi.SOLVER_TYPE_CMINPACK_LMDIF))


if __name__ == "__main__":
    main()
