#!/usr/bin/env python3
"""Whole-solve fixtures of the shared animated lens beyond NGMAX frames
(tests/golden/lens_shared/*.npz; tests/test_gpu_lens_shared.py).

Two cameras on one 3DE-classic lens with its distortion keyed per frame, over
more frames than NGMAX: the oracle's full run costs n FD columns per outer
iteration (about a minute on 50 frames), too slow to repeat per test.  As in
tests/golden/make_full_golden.py a fixture holds the generator call and a
SHA-256 digest of the generated problem instead of the scene; the test
regenerates the scene from its seed, checks the digest, and compares the
oracle's outputs: x, fvec, the ||f|| trace and the SolverResult counters.

``exp_x_envelope``: how far the oracle's own x moves when x0 is perturbed by
~1 ulp (relative 1e-15), over exactly the seeds registered in
tests/golden/envelopes.py -- from the oracle only, never from a GPU run.

    python tests/golden/make_lens_shared.py            # every missing fixture
    python tests/golden/make_lens_shared.py c5_f50_lens_anim_2cam
"""
from __future__ import annotations

import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "lens_shared")
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from mayamatchmovesolver_amd import synthetic as S  # noqa: E402
from tests.golden.envelopes import SEEDS  # noqa: E402
from tests.golden.make_full_golden import RES_FIELDS, problem_digest  # noqa: E402

# name: make_config(4, lens_model="classic_animated", ...) arguments.
# Scale 0.08, not the 0.05 of the structure and step tests: at 0.05 the run's
# third and fourth evaluations are wild trial points (||f|| = 7.7e265, then
# 7.3e3 from 3.6e3) where the oracle's own ||f|| moves by 9e-4 and 7e-3 under
# a 1-ulp change of x0 (seeds 1000-1002), so no fp64 implementation holds that
# trace at 1e-6.  At 0.08 the run is 16 evaluations and the oracle's ||f||
# moves by less than 7e-10 at every one of them (at 0.1 the run is 94
# evaluations, a quarter of an hour per oracle run).
CASES = {
    "c5_f50_lens_anim_2cam": dict(frames=50, scale=0.08, cameras=2),
}

def make_problem(name):
    return S.make_config(4, lens_model="classic_animated", **CASES[name])


def fixture_names():
    if not os.path.isdir(OUT):
        return []
    return sorted(f[:-4] for f in os.listdir(OUT) if f.endswith(".npz"))


def _run(job):
    """One oracle run: seed < 0 from x0 itself, else from x0 moved by ~1 ulp."""
    from oracle import refcpu as R
    name, seed = job
    prob = make_problem(name)
    x0 = prob.x0
    if seed >= 0:
        rng = np.random.default_rng(seed)
        x0 = prob.x0 * (1.0 + 1e-15 * rng.standard_normal(prob.x0.size))
    x, fvec, _eu, _ed, res, tr = R.solve(prob, S.config_options(prob), x0=x0)
    return seed, x, fvec, tr, res.as_dict()


def make(name, jobs=9):
    prob = make_problem(name)
    with ProcessPoolExecutor(jobs) as ex:
        runs = {r[0]: r for r in ex.map(_run, [(name, s) for s in (-1,) + SEEDS])}
    _s, x, fvec, tr, rd = runs[-1]
    scale = np.maximum(np.abs(x), 1e-3)
    env = max(float(np.max(np.abs(runs[s][1] - x) / scale)) for s in SEEDS)
    d = {"digest": np.array(problem_digest(prob)), "exp_x": x, "exp_fvec": fvec, "exp_trace": tr,
         "exp_x_envelope": np.array(env), "envelope_runs": np.array(len(SEEDS)),
         "envelope_seeds": np.array(SEEDS)}
    for f in RES_FIELDS:
        d["res_" + f] = np.array(rd[f])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    print("%-24s n=%d reason=%d trace=%d x-envelope=%.2e (%d runs)  %.0f KB" % (
        name, x.size, rd["reason_number"], tr.size, env, len(SEEDS),
        os.path.getsize(path) / 1024), flush=True)


def load(name):
    """(problem, options, fixture dict); raises if the regenerated scene's
    digest differs from the one the oracle ran on."""
    d = dict(np.load(os.path.join(OUT, name + ".npz"), allow_pickle=False))
    prob = make_problem(name)
    if problem_digest(prob) != str(d["digest"]):
        raise RuntimeError("%s: regenerated scene differs from the fixture's" % name)
    return prob, S.config_options(prob), d


if __name__ == "__main__":
    for n in sys.argv[1:] or [c for c in CASES if c not in fixture_names()]:
        make(n)
