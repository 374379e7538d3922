#!/usr/bin/env python3
"""Times the user-problem API (hpgmg_amd/problem.py, hpgmg_user_* of include/hpgmg_fv.h) at 256^3, config 2's shape (7-pt Helmholtz,
Chebyshev, 2^3 boxes of 128^3): set_coefficients, set_rhs, solve (one F-cycle) and get_solution, with host (NumPy) and device input, plus
one pack and one unpack launch alone.  hipEvent pairs on the library's launch stream around each call; every call synchronises before it
returns, so the pair brackets all of its device work.  Prints one JSON line of medians in ms.

    python tools/user_problem_timing.py [--n 256] [--repeats 5]
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
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    n = args.n
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(0) == 0
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()

    def timed(fn):
        out = []
        for _ in range(args.repeats):
            K.hpgmg_hip_event_record(e0)
            fn()
            K.hpgmg_hip_event_record(e1)
            out.append(K.hpgmg_hip_event_elapsed_ms(e0, e1))
        return statistics.median(out)

    rng = np.random.default_rng(0)
    alpha = 1.0 + rng.random((n, n, n))
    betas = [1.0 + rng.random(s) for s in ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))]
    f = rng.random((n, n, n)) - 0.5
    u = np.empty((n, n, n))
    dev = []

    def put(a):
        p = K.hpgmg_hip_malloc(a.nbytes)
        assert p and K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    res = {"n": n, "repeats": args.repeats}
    with Solver(n, bc="dirichlet", smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
        S, info, shift = s._ptr, H.UserInfo(), ctypes.c_double()
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        d_alpha, d_b = put(alpha), [put(b) for b in betas]
        d_f, d_u = put(f), K.hpgmg_hip_malloc(u.nbytes)
        dev.append(d_u)
        for where, A, Bs, F, U in (("host", alpha.ctypes.data, [b.ctypes.data for b in betas], f.ctypes.data, u.ctypes.data),
                                   ("device", d_alpha, d_b, d_f, d_u)):
            w = H.WHERE_HOST if where == "host" else H.WHERE_PLUGIN
            res[f"set_coefficients_{where}_ms"] = timed(lambda: lib.hpgmg_user_set_coefficients(S, A, *Bs, w))
            res[f"set_rhs_{where}_ms"] = timed(lambda: lib.hpgmg_user_set_rhs(S, F, w, ctypes.byref(shift)))
            res[f"solve_fmg_{where}_ms"] = timed(lambda: lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, w, ctypes.byref(info)))
            res[f"get_solution_{where}_ms"] = timed(lambda: lib.hpgmg_user_get_solution(S, U, w))
            res[f"pack_one_field_{where}_ms"] = timed(lambda: lib.hpgmg_dense_pack(L, H.VECTOR_F, F, w, H.DENSE_CELL, H.DENSE_CHECK_FINITE))
            res[f"unpack_one_field_{where}_ms"] = timed(lambda: lib.hpgmg_dense_unpack(L, H.VECTOR_U, U, w))
        res["fmg_residual"] = "%1.15e" % info.norm_of_residual
    for p in dev:
        K.hpgmg_hip_free(p)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
