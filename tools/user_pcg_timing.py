#!/usr/bin/env python3
"""Times method="pcg" of the user-problem API at 256^3, 7-pt Helmholtz, Chebyshev, 2^3 boxes of 128^3, on device arrays:
a solve of --iters iterations, and one iteration's parts alone -- the V-cycle (zero_vector + MGVCycle) and the three fused passes
(hpgmg_pcg_apply_dot / _update / _dot) -- next to the eight passes the reference-faithful MGPCG loop issues around its V-cycle on the same
level (apply_op, dot, two add_vectors, residual, norm, dot, add_vectors: the operators, unchanged), timed one by one and as one bracket around the whole sequence.  hipEvent pairs on the library's launch
stream around each call; every scalar is fetched before its call returns, so a pair brackets all of the call's device work.  Prints one JSON
line: medians in ms, and each fused pass's achieved GB/s for its compulsory traffic per cell (apply_dot 48 B: p, three betas, alpha in, Ap out;
update 48 B: four reads, two writes; dot 16 B).  method="fpcg"  next to it: a solve of the same iterations, and its one pass
hpgmg_pcg_dot2 (r.z and Ap.z, 24 B) next to two hpgmg_pcg_dot calls on the same vectors.

    python tools/user_pcg_timing.py [--n 256] [--repeats 7] [--iters 10] [--cli]
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--cli", action="store_true", help="also run hpgmg-fv --helmholtz --mgpcg 7 8 in a child process (n = 256)")
    args = ap.parse_args()
    n = args.n
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(0) == 0
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()
    lib.MGVCycle.restype, lib.MGVCycle.argtypes = None, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int]

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
    dev = []

    def put(a):
        p = K.hpgmg_hip_malloc(a.nbytes)
        assert p and K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    a, b, cells = 1.0, 1.0, float(n) ** 3
    res = {"n": n, "repeats": args.repeats, "iters": args.iters}
    with Solver(n, bc="dirichlet", smoother="cheby", a=a, b=b, lib=lib) as s:
        S, info, shift, val, val2 = s._ptr, H.UserInfo(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        hs = lib.hpgmg_user_solver_of(S)
        L, G = lib.hpgmg_solver_level(hs, 0), lib.hpgmg_solver_mg(hs)
        w = H.WHERE_PLUGIN
        assert lib.hpgmg_user_set_coefficients(S, put(alpha), *[put(x) for x in betas], w) == 0
        assert lib.hpgmg_user_set_rhs(S, put(f), w, ctypes.byref(shift)) == 0
        assert lib.hpgmg_user_set_max_iterations(S, args.iters) == 0
        solve = lambda: lib.hpgmg_user_solve(S, H.USER_PCG, 1e-300, None, w, ctypes.byref(info))  # noqa: E731  (never converges: all iterations run)
        solve()                                                   # grows the levels; warms every launch
        res["solve_ms"] = timed(solve)
        res["iterations"] = info.vcycles
        res["per_iteration_ms"] = res["solve_ms"] / info.vcycles
        fsolve = lambda: lib.hpgmg_user_solve(S, H.USER_FPCG, 1e-300, None, w, ctypes.byref(info))  # noqa: E731  (method="fpcg")
        fsolve()                                                  # its segments have a key of their own: captured here
        res["fpcg_solve_ms"] = timed(fsolve)
        res["fpcg_iterations"] = info.vcycles
        res["fpcg_per_iteration_ms"] = res["fpcg_solve_ms"] / info.vcycles
        x, r, p = H.VECTOR_U, H.VECTOR_R, lib.hpgmg_vectors_reserved()
        Ap, z, F, T = p + 1, p + 2, H.VECTOR_F, H.VECTOR_TEMP
        res["vcycle_ms"] = timed(lambda: (lib.zero_vector(L, z), lib.MGVCycle(G, z, r, a, b, 0), K.hpgmg_hip_sync()))
        res["pcg_apply_dot_ms"] = timed(lambda: lib.hpgmg_pcg_apply_dot(L, Ap, p, a, b, ctypes.byref(val)))
        res["pcg_update_ms"] = timed(lambda: lib.hpgmg_pcg_update(L, x, r, p, Ap, 1e-9, ctypes.byref(val)))
        res["pcg_dot_ms"] = timed(lambda: lib.hpgmg_pcg_dot(L, r, z, ctypes.byref(val)))
        # fpcg's one pass for r.z and Ap.z (24 B per cell, one fold, one wait) next to the two pcg_dot calls it replaces (32 B, two of each)
        res["pcg_dot2_ms"] = timed(lambda: lib.hpgmg_pcg_dot2(L, r, Ap, z, ctypes.byref(val), ctypes.byref(val2)))
        res["pcg_dot_twice_ms"] = timed(lambda: (lib.hpgmg_pcg_dot(L, r, z, ctypes.byref(val)), lib.hpgmg_pcg_dot(L, Ap, z, ctypes.byref(val2))))
        res["pcg_axpy_ms"] = timed(lambda: (lib.add_vectors(L, p, 1.0, z, 0.5, p), K.hpgmg_hip_sync()))
        res["pcg_outside_vcycle_ms"] = res["pcg_apply_dot_ms"] + res["pcg_update_ms"] + res["pcg_dot_ms"] + res["pcg_axpy_ms"]
        res["fpcg_outside_vcycle_ms"] = res["pcg_apply_dot_ms"] + res["pcg_update_ms"] + res["pcg_dot2_ms"] + res["pcg_axpy_ms"]
        for key, bytes_per_cell in (("pcg_apply_dot", 48), ("pcg_update", 48), ("pcg_dot", 16), ("pcg_dot2", 24)):
            res[key + "_GBps"] = bytes_per_cell * cells / (res[key + "_ms"] * 1e-3) / 1e9
        # the passes MGPCG issues per iteration around the V-cycle (mg.c), one by one
        parts = {
            "apply_op": lambda: (lib.apply_op(L, Ap, p, a, b), K.hpgmg_hip_sync()),
            "dot": lambda: lib.dot(L, Ap, p),
            "add_vectors": lambda: (lib.add_vectors(L, x, 1.0, x, 1e-9, p), K.hpgmg_hip_sync()),
            "residual": lambda: (lib.residual(L, T, x, F, a, b), K.hpgmg_hip_sync()),
            "norm": lambda: lib.norm(L, T),
        }
        res["mgpcg_parts_ms"] = {k: timed(fn) for k, fn in parts.items()}

        def mgpcg_body():                                        # MGPCG's loop body without its V-cycle, in its order, one bracket around all of it
            lib.apply_op(L, Ap, p, a, b)
            lib.dot(L, Ap, p)
            lib.add_vectors(L, x, 1.0, x, 1e-9, p)
            lib.add_vectors(L, r, 1.0, r, -1e-9, Ap)
            lib.residual(L, T, x, F, a, b)
            lib.norm(L, T)
            lib.dot(L, r, z)
            lib.add_vectors(L, p, 1.0, z, 0.5, p)
            K.hpgmg_hip_sync()

        def pcg_body():                                          # MGPCGSolve's, likewise
            lib.hpgmg_pcg_apply_dot(L, Ap, p, a, b, ctypes.byref(val))
            lib.hpgmg_pcg_update(L, x, r, p, Ap, 1e-9, ctypes.byref(val))
            lib.hpgmg_pcg_dot(L, r, z, ctypes.byref(val))
            lib.add_vectors(L, p, 1.0, z, 0.5, p)
            K.hpgmg_hip_sync()

        def fpcg_body():                                         # MGFPCGSolve's: dot2 in place of dot
            lib.hpgmg_pcg_apply_dot(L, Ap, p, a, b, ctypes.byref(val))
            lib.hpgmg_pcg_update(L, x, r, p, Ap, 1e-9, ctypes.byref(val))
            lib.hpgmg_pcg_dot2(L, r, Ap, z, ctypes.byref(val), ctypes.byref(val2))
            lib.add_vectors(L, p, 1.0, z, 0.5, p)
            K.hpgmg_hip_sync()

        res["mgpcg_outside_vcycle_ms"] = timed(mgpcg_body)
        res["fpcg_outside_vcycle_one_bracket_ms"] = timed(fpcg_body)
        res["pcg_outside_vcycle_one_bracket_ms"] = timed(pcg_body)
    for q in dev:
        K.hpgmg_hip_free(q)
    if args.cli and n == 256:
        # the reference-faithful loop as the benchmark executable runs it (hpgmg-fv --helmholtz --mgpcg 7 8: the same 256^3 level, the benchmark's own
        # coefficients, two solves): host wall time of the second solve over its iterations, V-cycle included -- to set against per_iteration_ms
        exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hpgmg_amd", "bin", "hpgmg-fv")
        out = subprocess.run([exe, "--helmholtz", "--mgpcg", "7", "8"], capture_output=True, text=True, timeout=300).stdout
        solves = out.split("MGPCG...")[1:]
        if len(solves) >= 2:
            iters = len(re.findall(r"iter=", solves[1]))
            secs = re.search(r"done \(([0-9.]+) seconds\)", solves[1])
            if iters and secs:
                res["mgpcg_cli_iterations"] = iters
                res["mgpcg_cli_per_iteration_ms"] = 1e3 * float(secs.group(1)) / iters
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
