#!/usr/bin/env python3
"""Observed temporal order of the Newmark march of the dense-array solver (Solver.wave_start / wave_step) on the CPU oracle.

A smooth manufactured solution with time-dependent source and wall data on the unit cube, Dirichlet walls:
    u = cos(3 t) S(x, y, z),  S = sin(x + 0.5) cos(y) exp(-z)  (so div grad S = -S),  alpha = 1 + x / 2,  beta = 1,
    f = alpha u_tt + sigma alpha u_t - b div grad u = (-9 alpha cos(3 t) - 3 sigma alpha sin(3 t) + b cos(3 t)) S,   g(t) = u on the walls.
The error at t = T is taken against a march of the same grid with a far smaller dt, so that the spatial error, which is the same in both,
drops out and the temporal error is what is left.  Prints one JSON line: the errors for dt, dt/2, dt/4 and the two observed orders per rule.

    python tools/user_wave_order.py [--n 32] [--T 0.5] [--steps 4] [--fine 256]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hpgmg_amd.problem import Solver  # noqa: E402
from hpgmg_testlib import Backend  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32)
    ap.add_argument("--T", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--fine", type=int, default=256)
    args = ap.parse_args()
    n, T, b = args.n, args.T, 1.0
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    c = (np.arange(n) + 0.5) / n
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    S = lambda x, y, z: np.sin(x + 0.5) * np.cos(y) * np.exp(-z)  # noqa: E731
    alpha, Sc = np.ascontiguousarray(1.0 + 0.5 * x), S(x, y, z)
    betas = [np.ones(shape) for shape in ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))]

    def march(rule, steps):
        beta, gamma, sigma = rule
        dt = T / steps
        with Solver(n, bc="dirichlet", a=1.0, b=b, lib=lib) as s:
            s.set_coefficients(alpha, *betas)
            src = lambda t: np.ascontiguousarray((-9.0 * alpha * np.cos(3.0 * t) - 3.0 * sigma * alpha * np.sin(3.0 * t) + b * np.cos(3.0 * t)) * Sc)  # noqa: E731
            wall = lambda t: s.boundary_from(lambda x, y, z: np.cos(3.0 * t) * S(x, y, z))  # noqa: E731
            s.wave_start(np.ascontiguousarray(Sc), np.zeros((n, n, n)), src(0.0), boundary=wall(0.0), dt=dt, beta=beta, gamma=gamma, damping=sigma)
            for k in range(1, steps + 1):
                info = s.wave_step(src(k * dt), boundary=wall(k * dt), rtol=1e-11)
                assert info.converged
            return s.get_solution()

    res = {"n": n, "T": T, "reference_steps": args.fine}
    for rule in ((0.25, 0.5, 0.0), (0.25, 0.5, 0.7), (0.3025, 0.6, 0.0)):
        ref = march((0.25, 0.5, rule[2]), args.fine)
        errs = [float(np.abs(march(rule, args.steps * m) - ref).max()) for m in (1, 2, 4)]
        res["beta_%g_gamma_%g_sigma_%g" % rule] = {"dt": [T / (args.steps * m) for m in (1, 2, 4)], "error": errs, "spatial_error": float(np.abs(ref - np.cos(3.0 * T) * Sc).max()),
                                                   "order": [float(np.log2(errs[i] / errs[i + 1])) for i in range(2)]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
