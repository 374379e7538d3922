#!/usr/bin/env python3
"""Times the Neumann / mixed-wall path of the user-problem API at 256^3, config 2's shape (7-pt Helmholtz, Chebyshev, 2^3 boxes of 128^3),
against the all-Dirichlet boundary-value path in the same process, the calls alternating: the masked face-array pack against the plain pack;
set_rhs_dirichlet and the boundary F-cycle of a solver with Neumann side walls against those of the Dirichlet solver; then, separately, six
Neumann walls with Poisson, which goes through the mean shift and gives up the fused bottom solve and tails.  Device arrays; hipEvent pairs on
the library's launch stream around each call.  One JSON line of medians in ms.

    python tools/user_neumann_timing.py [--n 256] [--repeats 7]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver  # noqa: E402

SIDES = ("dirichlet", "dirichlet", "neumann", "neumann", "neumann", "neumann")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    n = args.n
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(0) == 0
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()

    def once(fn):
        K.hpgmg_hip_event_record(e0)
        assert fn() in (0, None)
        K.hpgmg_hip_event_record(e1)
        return K.hpgmg_hip_event_elapsed_ms(e0, e1)

    def pair(fa, fb):                     # alternate the two calls, after one warm-up of each
        fa(), fb()
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(once(fa))
            tb.append(once(fb))
        return statistics.median(ta), statistics.median(tb)

    rng = np.random.default_rng(0)
    alpha = 1.0 + rng.random((n, n, n))
    betas = [1.0 + rng.random(s) for s in ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))]
    f = rng.random((n, n, n)) - 0.5
    g = rng.random((6, n, n)) - 0.5
    dev = []

    def put(a):
        p = K.hpgmg_hip_malloc(a.nbytes)
        assert p and K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    d_alpha, d_betas, d_f, d_g = put(alpha), [put(b) for b in betas], put(f), put(g)
    w, info, shift = H.WHERE_PLUGIN, H.UserInfo(), ctypes.c_double()

    def fmg(S):
        def run():
            assert lib.hpgmg_user_set_rhs_dirichlet(S, d_f, d_g, w, ctypes.byref(shift)) == 0
            return once(lambda: lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, w, ctypes.byref(info)))
        return run

    def alternate(fa, fb):
        fa(), fb()
        ta, tb = [], []
        for _ in range(args.repeats):
            ta.append(fa())
            tb.append(fb())
        return statistics.median(ta), statistics.median(tb)

    res = {"n": n, "repeats": args.repeats}
    with Solver(n, bc="dirichlet", smoother="cheby", a=1.0, b=1.0, lib=lib) as d, Solver(n, bc=SIDES, smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
        D, S = d._ptr, s._ptr
        for P in (D, S):
            assert lib.hpgmg_user_set_coefficients(P, d_alpha, *d_betas, w) == 0
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(D), 0)       # the packs: on the Dirichlet solver's level, beta_j (restored below)
        wall = lib.hpgmg_vector_alloc(6 * n * n)
        res["pack_face_ms"], res["pack_walls_ms"] = pair(
            lambda: lib.hpgmg_dense_pack(L, H.VECTOR_BETA_J, d_betas[1], w, H.DENSE_FACE_J, H.DENSE_CHECK_POSITIVE),
            lambda: lib.hpgmg_dense_pack_walls(L, H.VECTOR_BETA_J, d_betas[1], w, H.DENSE_FACE_J, H.DENSE_CHECK_POSITIVE, 60, wall))
        lib.hpgmg_vector_free(wall)
        assert lib.hpgmg_user_set_coefficients(D, d_alpha, *d_betas, w) == 0
        res["set_rhs_dirichlet_ms"], res["set_rhs_mixed_ms"] = pair(
            lambda: lib.hpgmg_user_set_rhs_dirichlet(D, d_f, d_g, w, ctypes.byref(shift)),
            lambda: lib.hpgmg_user_set_rhs_dirichlet(S, d_f, d_g, w, ctypes.byref(shift)))
        res["fmg_dirichlet_ms"], res["fmg_mixed_ms"] = alternate(fmg(D), fmg(S))
        res["fmg_mixed_over_dirichlet"] = res["fmg_mixed_ms"] / res["fmg_dirichlet_ms"]
    with Solver(n, bc="dirichlet", smoother="cheby", a=0.0, b=1.0, lib=lib) as d, Solver(n, bc="neumann", smoother="cheby", a=0.0, b=1.0, lib=lib) as s:
        D, S = d._ptr, s._ptr
        for P in (D, S):
            assert lib.hpgmg_user_set_coefficients(P, None, *d_betas, w) == 0
        res["poisson_set_rhs_dirichlet_ms"], res["poisson_set_rhs_six_neumann_ms"] = pair(
            lambda: lib.hpgmg_user_set_rhs_dirichlet(D, d_f, d_g, w, ctypes.byref(shift)),
            lambda: lib.hpgmg_user_set_rhs_dirichlet(S, d_f, d_g, w, ctypes.byref(shift)))
        res["poisson_fmg_dirichlet_ms"], res["poisson_fmg_six_neumann_ms"] = alternate(fmg(D), fmg(S))
        res["poisson_six_neumann_over_dirichlet"] = res["poisson_fmg_six_neumann_ms"] / res["poisson_fmg_dirichlet_ms"]
    for p in dev:
        K.hpgmg_hip_free(p)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
