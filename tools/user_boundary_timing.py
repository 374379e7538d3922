#!/usr/bin/env python3
"""Times the boundary-value path of the user-problem API (hpgmg_user_set_rhs_dirichlet, HPGMG_USER_FMG after it) at 256^3, config 2's
shape (7-pt Helmholtz, Chebyshev, 2^3 boxes of 128^3), against the homogeneous calls on the same solver: one pack against one lifted pack
launch, set_rhs against set_rhs_dirichlet (which also builds every level's g_l and phi_l), and the homogeneous F-cycle against the boundary
F-cycle.  Then Robin walls next to Neumann ones on two solvers with Dirichlet i-walls: set_coefficients against
set_coefficients_robin (which adds a kappa check, a store launch per level and a second rebuild per coarse level), and the two F-cycles.
Device arrays; hipEvent pairs on the library's launch stream around each call, the calls alternating.  One JSON line of medians in ms.

    python tools/user_boundary_timing.py [--n 256] [--repeats 7]
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

    res = {"n": n, "repeats": args.repeats}
    with Solver(n, bc="dirichlet", smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
        S, info, shift, w = s._ptr, H.UserInfo(), ctypes.c_double(), H.WHERE_PLUGIN
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        assert lib.hpgmg_user_set_coefficients(S, put(alpha), *[put(b) for b in betas], w) == 0
        d_f, d_g = put(f), put(g)
        d_g0 = lib.hpgmg_vector_alloc(6 * n * n)
        lib.hpgmg_vector_copy(d_g0, d_g, 6 * n * n)
        res["pack_ms"], res["pack_lifted_ms"] = pair(
            lambda: lib.hpgmg_dense_pack(L, H.VECTOR_F, d_f, w, H.DENSE_CELL, H.DENSE_CHECK_FINITE),
            lambda: lib.hpgmg_dense_pack_lifted(L, H.VECTOR_F, d_f, w, d_g0, 1.0))
        lib.hpgmg_vector_free(d_g0)
        res["set_rhs_ms"], res["set_rhs_dirichlet_ms"] = pair(
            lambda: lib.hpgmg_user_set_rhs(S, d_f, w, ctypes.byref(shift)),
            lambda: lib.hpgmg_user_set_rhs_dirichlet(S, d_f, d_g, w, ctypes.byref(shift)))

        def fmg(boundary):
            def run():
                if boundary:
                    lib.hpgmg_user_set_rhs_dirichlet(S, d_f, d_g, w, ctypes.byref(shift))
                else:
                    lib.hpgmg_user_set_rhs(S, d_f, w, ctypes.byref(shift))
                return once(lambda: lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, w, ctypes.byref(info)))
            return run
        plain, bnd = fmg(False), fmg(True)
        plain(), bnd()
        tp, tb = [], []
        for _ in range(args.repeats):
            tp.append(plain())
            tb.append(bnd())
        res["fmg_homogeneous_ms"], res["fmg_boundary_ms"] = statistics.median(tp), statistics.median(tb)
        res["fmg_boundary_over_homogeneous"] = res["fmg_boundary_ms"] / res["fmg_homogeneous_ms"]
    neumann = ("dirichlet", "dirichlet") + ("neumann",) * 4
    robin = ("dirichlet", "dirichlet") + ("convective",) * 4
    with Solver(n, bc=neumann, smoother="cheby", a=1.0, b=1.0, lib=lib) as sn, Solver(n, bc=robin, smoother="cheby", a=1.0, b=1.0, lib=lib) as sr:
        SN, SR, info, shift, w = sn._ptr, sr._ptr, H.UserInfo(), ctypes.c_double(), H.WHERE_PLUGIN
        d_alpha, d_betas, d_kappa = put(alpha), [put(b) for b in betas], put(1.0 + rng.random((6, n, n)))
        res["set_coefficients_neumann_ms"], res["set_coefficients_robin_ms"] = pair(
            lambda: lib.hpgmg_user_set_coefficients(SN, d_alpha, *d_betas, w),
            lambda: lib.hpgmg_user_set_coefficients_robin(SR, d_alpha, *d_betas, d_kappa, w))

        def fmg_walls(P):
            def run():
                assert lib.hpgmg_user_set_rhs_dirichlet(P, d_f, d_g, w, ctypes.byref(shift)) == 0
                return once(lambda: lib.hpgmg_user_solve(P, H.USER_FMG, 1e-10, None, w, ctypes.byref(info)))
            return run
        fn_, fr_ = fmg_walls(SN), fmg_walls(SR)
        fn_(), fr_()
        tn, tr = [], []
        for _ in range(args.repeats):
            tn.append(fn_())
            tr.append(fr_())
        res["fmg_neumann_ms"], res["fmg_robin_ms"] = statistics.median(tn), statistics.median(tr)
        res["fmg_robin_over_neumann"] = res["fmg_robin_ms"] / res["fmg_neumann_ms"]
    for p in dev:
        K.hpgmg_hip_free(p)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
