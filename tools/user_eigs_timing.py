#!/usr/bin/env python3
"""Times Solver.eigs at 256^3, 7-pt Helmholtz, Chebyshev, 2^3 boxes of 128^3, k = 4 and extra = 2 (m = 6, S = [X, W, P] of 18
columns), on device arrays: an iteration (the difference of two calls with other iteration limits), its parts alone -- the V-cycle with its two
copies, apply_op, hpgmg_block_residual, the two Gram requests and the four combinations -- and each block kernel next to the existing launches it
replaces, in the same process: the 18 x 18 Gram request against the same entries from hpgmg_pcg_dot calls, the combination of 18 vectors into 6
against scale_vector / add_vectors chains.  hipEvent pairs on the library's launch stream around each call, medians of --repeats.  Prints one JSON line:
milliseconds, the bytes each form moves per cell and the TB/s that makes.

    python tools/user_eigs_timing.py [--n 256] [--repeats 5]
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

TILE = 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    n, k, extra = args.n, 4, 2
    m = k + extra
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(0) == 0
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()
    c_int, c_dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    for name in ("MGPreconditionerBegin", "MGPreconditionerApply"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = None, [vp, c_int, c_int, c_int, c_dbl, c_dbl]

    def timed(fn):
        out = []
        for _ in range(args.repeats):
            K.hpgmg_hip_event_record(e0)
            fn()
            K.hpgmg_hip_sync()
            K.hpgmg_hip_event_record(e1)
            K.hpgmg_hip_sync()
            out.append(K.hpgmg_hip_event_elapsed_ms(e0, e1))
        return statistics.median(out)

    rng = np.random.default_rng(0)
    alpha = 1.0 + rng.random((n, n, n))
    betas = [1.0 + rng.random(s) for s in ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))]
    dev = []

    def put(a):
        p = K.hpgmg_hip_malloc(a.nbytes)
        assert p and K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    a, b, cells = 1.0, 1.0, float(n) ** 3
    res = {"n": n, "repeats": args.repeats, "k": k, "extra": extra, "tile": TILE}
    tbps = lambda bytes_per_cell, ms: bytes_per_cell * cells / (ms * 1e-3) / 1e12  # noqa: E731
    with Solver(n, bc="dirichlet", smoother="cheby", a=a, b=b, lib=lib) as s:
        S = s._ptr
        hs = lib.hpgmg_user_solver_of(S)
        L, G = lib.hpgmg_solver_level(hs, 0), lib.hpgmg_solver_mg(hs)
        assert lib.hpgmg_user_set_coefficients(S, put(alpha), *[put(x) for x in betas], H.WHERE_PLUGIN) == 0
        modes = K.hpgmg_hip_malloc(k * n ** 3 * 8)
        dev.append(modes)
        lam, info = (c_dbl * k)(), H.UserEigInfo()
        run = lambda iters: lib.hpgmg_user_eigs(S, k, extra, 1e-300, iters, None, H.WHERE_PLUGIN, lam, modes, ctypes.byref(info))  # noqa: E731  (never converges)
        assert run(2) == 0                                       # grows the levels; warms every launch
        t2, t6 = timed(lambda: run(2)), timed(lambda: run(6))
        res["eigs_2_iterations_ms"], res["eigs_6_iterations_ms"], res["iteration_ms"] = t2, t6, (t6 - t2) / 4.0
        # what a call costs besides its iterations: the default start block (formed on the host, m uploads), the first and the last Rayleigh-Ritz, 2 m applies, the unpack
        res["outside_iterations_ms"] = t2 - 2.0 * res["iteration_ms"]
        K.hpgmg_hip_event_record(e0)
        assert lib.hpgmg_user_eigs(S, k, extra, 1e-6, 60, None, H.WHERE_PLUGIN, lam, modes, ctypes.byref(info)) == 0
        K.hpgmg_hip_event_record(e1)
        K.hpgmg_hip_sync()
        res["eigs_rtol_1e-6"] = {"ms": K.hpgmg_hip_event_elapsed_ms(e0, e1), "iterations": info.iterations, "vcycles": info.vcycles, "converged": bool(info.converged),
                                 "lam": list(lam), "residuals": list(info.residuals[:k])}
        # the block's vectors: the last 6 m of the finest level, column j at 6 j: X, AX, W, AW, P, AP
        lv = (c_int * H.INFO_COUNT)()
        lib.hpgmg_level_info(L, lv)
        base = lv[H.INFO_NUM_VECTORS] - 6 * m
        X, AX, W, AW, P, AP = ([base + 6 * j + q for j in range(m)] for q in range(6))
        Sx, ASx = X + W + P, AX + AW + AP
        ids = lambda v: (c_int * len(v))(*v)  # noqa: E731
        Gm, val = (c_dbl * (len(Sx) ** 2))(), c_dbl()
        z, r = lib.hpgmg_vectors_reserved() + 2, H.VECTOR_R
        lib.MGPreconditionerBegin(G, 0, z, r, a, b)
        mu, rmax, mxmax = (c_dbl * m)(*([30.0] * m)), (c_dbl * m)(), (c_dbl * m)()
        C = (c_dbl * (18 * 6))(*(rng.random(18 * 6) - 0.5))
        parts = {
            "vcycle_with_copies": lambda: (lib.scale_vector(L, r, 1.0, AW[0]), lib.MGPreconditionerApply(G, 0, z, r, a, b), lib.scale_vector(L, W[0], 1.0, z)),
            "apply_op": lambda: lib.apply_op(L, AW[0], W[0], a, b),
            "block_residual_6": lambda: lib.hpgmg_block_residual(L, ids(AW), ids(AX), ids(X), m, H.VECTOR_ALPHA, mu, rmax, mxmax),
            "block_gram_18x18": lambda: lib.hpgmg_block_gram(L, ids(Sx), 18, ids(ASx), 18, -1, Gm),
            "block_gram_18_weighted_symmetric": lambda: lib.hpgmg_block_gram(L, ids(Sx), 18, ids(Sx), 18, H.VECTOR_ALPHA, Gm),
            "block_gram_18_symmetric": lambda: lib.hpgmg_block_gram(L, ids(Sx), 18, ids(Sx), 18, -1, Gm),
            "block_combine_18_to_6": lambda: lib.hpgmg_block_combine(L, ids(AW), 6, ids(Sx), 18, C),
            "block_combine_12_to_6": lambda: lib.hpgmg_block_combine(L, ids(AW), 6, ids(W + P), 12, C),
        }
        ms = {name: timed(fn) for name, fn in parts.items()}

        def dots(pairs):
            for i, j in pairs:
                lib.hpgmg_pcg_dot(L, i, j, ctypes.byref(val))

        def chains(outs, ins):
            for j, vo in enumerate(outs):
                lib.scale_vector(L, vo, C[j], ins[0])
                for i, vi in enumerate(ins[1:]):
                    lib.add_vectors(L, vo, 1.0, vo, C[6 * (i + 1) + j], vi)

        ms["pcg_dot_x324"] = timed(lambda: dots([(i, j) for i in Sx for j in ASx]))
        ms["pcg_dot_x171"] = timed(lambda: dots([(Sx[i], Sx[j]) for i in range(18) for j in range(i, 18)]))
        ms["axpy_chain_18_to_6"] = timed(lambda: chains(AW, Sx))
        res["ms"] = ms
        # bytes per cell: a T x T tile costs 2 T loads (T on a diagonal tile of a symmetric request; one more for the weight)
        tiles = (18 // TILE) ** 2
        sym = 18 // TILE * (18 // TILE + 1) // 2
        traffic = {"block_gram_18x18": 8 * tiles * 2 * TILE, "pcg_dot_x324": 16 * 324,
                   "block_gram_18_symmetric": 8 * (18 // TILE * TILE + (sym - 18 // TILE) * 2 * TILE), "pcg_dot_x171": 16 * 171,
                   "block_gram_18_weighted_symmetric": 8 * (18 // TILE * (TILE + 1) + (sym - 18 // TILE) * (2 * TILE + 1)),
                   "block_combine_18_to_6": 8 * (18 + 6), "axpy_chain_18_to_6": 6 * (16 + 17 * 24), "block_combine_12_to_6": 8 * (12 + 6),
                   "block_residual_6": 8 * 6 * 4, "apply_op": 48}
        res["bytes_per_cell"] = traffic
        res["TBps"] = {name: tbps(v, ms[name]) for name, v in traffic.items()}
        res["gram_flops_TF"] = {"block_gram_18x18": 2 * 324 * cells / (ms["block_gram_18x18"] * 1e-3) / 1e12}
        na = m                                                    # every column active
        per_iter = {"vcycles": na * ms["vcycle_with_copies"], "applies": na * ms["apply_op"],
                    "block_kernels": ms["block_residual_6"] + ms["block_gram_18x18"] + ms["block_gram_18_weighted_symmetric"] + 2 * ms["block_combine_18_to_6"] + 2 * ms["block_combine_12_to_6"]}
        total = sum(per_iter.values())
        res["iteration_parts_ms"] = per_iter
        res["iteration_shares"] = {name: v / total for name, v in per_iter.items()}
    for q in dev:
        K.hpgmg_hip_free(q)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
