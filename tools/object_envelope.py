#!/usr/bin/env python3
"""The oracle's own x envelope on the object-tracking scenes of
tests/test_gpu_object.py (the method of tools/wide_arrow_envelope.py: solve,
then solve again from x0 perturbed by ~1 ulp, relative 1e-15, 3 seeds; the
envelope is the largest relative change of any x component, floor 1e-3).  A
scene whose envelope exceeds 1e-7 cannot carry the tests' 1e-6 bar with
margin and is replaced by another seed; the bar is not widened.

Run from the repo root (CPU only):
    python tools/object_envelope.py > profiles/r13_object/object_envelope.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mayamatchmovesolver_amd import abi, synthetic as S  # noqa: E402
from oracle import refcpu as R  # noqa: E402
from wide_arrow_envelope import row  # noqa: E402

DAG, MMSG = abi.SCENE_GRAPH_MODE_MAYA_DAG, abi.SCENE_GRAPH_MODE_MM_SCENE_GRAPH
LMDER, LMDIF = abi.SOLVER_TYPE_CMINPACK_LMDER, abi.SOLVER_TYPE_CMINPACK_LMDIF


def main():
    print("# oracle x envelope on the object scenes (synthetic.object_options: lmder delta 1e-4, lmdif delta 1e-8; tol 1e-6)")
    for name, kw in S.OBJECT_TEST_SCENES.items():
        for mode in (DAG, MMSG):
            for st in (LMDER, LMDIF):
                if name != "above_cap" and (mode, st) != (DAG, LMDER):
                    continue  # the tests solve the other scenes with the defaults
                row("%s mode %d solver %d" % (name, mode, st), S.object_scene(**kw),
                    S.object_options(mode, st))
    # the plan-cache test's second solve: the scene written back at the first
    # solve's x + 0.01 (the oracle's first solve stands in for the device's,
    # which agrees with it to 1e-6)
    from tests.test_gpu_plan_cache import written_back
    prob = S.object_scene(**S.OBJECT_TEST_SCENES["above_cap"])
    x = R.solve(prob, S.object_options())[0]
    row("above_cap restarted at x + 0.01", written_back(prob, x + 0.01), S.object_options())


if __name__ == "__main__":
    main()
