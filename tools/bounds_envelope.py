#!/usr/bin/env python3
"""The oracle's own x envelope on the bounded scenes of tests/test_gpu_bounds.py
(tests/test_bounds_host.py holds each to 1e-7): every case of its SOLVES is
solved from x0 and from nextafter(x0); the envelope is the largest change of
any x component, in external values relative to 1 + |x| and in internal values
relative to max(|x|, 1e-3) (the measure the device's x is compared in).  A
scene above 1e-7 gets another with_bounds seed or fewer iterations; the bar
is not widened.

Run from the repo root (CPU only):
    python tools/bounds_envelope.py > profiles/r14_bounds/bounds_envelope.txt
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mayamatchmovesolver_amd import synthetic as S  # noqa: E402
from tests import test_bounds_host as H  # noqa: E402


def main():
    print("# oracle x envelope on the bounded twins (synthetic.with_bounds), 1 ulp of x0")
    print("# case: scene (with_bounds seed) n / negative-step columns at x0 / frozen; reason, "
          "evaluations, ||f|| first -> last; envelope external, internal")
    for case in sorted(H.SOLVES):
        name = H.SOLVES[case][0]
        prob, opt = H.scene(name), H.options(case)
        t = time.time()
        x, _f, _eu, _ed, res, tr = H.oracle_solve(case)
        ext, internal = H.envelope(prob, opt, x)
        print("%-22s %-20s seed %2d n=%4d flipped=%3d frozen=%3d reason=%d evals=%3d "
              "||f||=%.6e -> %.6e envelope=%.1e external %.1e internal (%.1f s)" % (
                  case, name, H.SCENES[name][1], prob.num_params,
                  int(S.flipped_columns(prob, 1e-4).sum()), int((S.bound_kinds(prob) == 1).sum()),
                  res.reason_number, res.function_evals, tr[0], tr[-1], ext, internal,
                  time.time() - t), flush=True)
    prob = H.scene("c4_f257")
    print("%-22s %-20s seed %2d n=%4d flipped=%3d frozen=%3d (first iteration only: no solve)" % (
        "c4_f257", "c4_f257", H.SCENES["c4_f257"][1], prob.num_params,
        int(S.flipped_columns(prob, 1e-4).sum()), int((S.bound_kinds(prob) == 1).sum())))


if __name__ == "__main__":
    main()
