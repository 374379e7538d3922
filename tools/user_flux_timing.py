#!/usr/bin/env python3
"""Times Solver.flux's entry point (hpgmg_user_flux of include/hpgmg_fv.h) at 256^3, config 2's shape (7-pt Helmholtz, 2^3 boxes
of 128^3, Dirichlet walls with boundary values): the whole call with host (NumPy) and device arrays, the flux pass alone
(hpgmg_dense_unpack_flux on the vector the call has packed: one launch for the three arrays), and in the same run apply and one device pack
to set them beside.  hipEvent pairs on the library's launch stream around each call; every call synchronises before it returns, so the pair
brackets all of its device work.  Prints one JSON line of medians in ms, and the pass's rate against its minimum traffic of 56 B per cell
(u, three betas in, three fluxes out).

    python tools/user_flux_timing.py [--n 256] [--repeats 9]
"""
import argparse
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
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    n = args.n
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(0) == 0
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()

    def timed(fn):
        out = []
        for _ in range(args.repeats + 1):                      # the first run allocates (staging buffer, validation word): not counted
            K.hpgmg_hip_event_record(e0)
            assert fn() == 0
            K.hpgmg_hip_event_record(e1)
            out.append(K.hpgmg_hip_event_elapsed_ms(e0, e1))
        return statistics.median(out[1:])

    rng = np.random.default_rng(0)
    alpha = 1.0 + rng.random((n, n, n))
    shapes = ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))
    betas = [1.0 + rng.random(s) for s in shapes]
    u, g = rng.random((n, n, n)) - 0.5, rng.random((6, n, n)) - 0.5
    y, q = np.empty((n, n, n)), [np.empty(s) for s in shapes]
    dev = []

    def put(a):
        p = K.hpgmg_hip_malloc(a.nbytes)
        assert p and K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        dev.append(p)
        return p

    res = {"n": n, "repeats": args.repeats}
    with Solver(n, bc="dirichlet", smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
        S = s._ptr
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        x_id = lib.hpgmg_vectors_reserved()                    # the solver's operand vector
        s.set_coefficients(alpha, *betas)
        d_u, d_g, d_y, d_q = put(u), put(g), put(y), [put(a) for a in q]
        for where, U, G, Y, Q in (("host", u.ctypes.data, g.ctypes.data, y.ctypes.data, [a.ctypes.data for a in q]), ("device", d_u, d_g, d_y, d_q)):
            w = H.WHERE_HOST if where == "host" else H.WHERE_PLUGIN
            res[f"flux_{where}_ms"] = timed(lambda: lib.hpgmg_user_flux(S, U, G, *Q, w))
            res[f"apply_{where}_ms"] = timed(lambda: lib.hpgmg_user_apply_dirichlet(S, U, G, Y, w))
        # the pass alone, on the operand the last flux call left (packed, ghost zones exchanged), and one device pack
        assert lib.hpgmg_user_flux(S, d_u, d_g, *d_q, H.WHERE_PLUGIN) == 0
        res["flux_pass_device_ms"] = timed(lambda: lib.hpgmg_dense_unpack_flux(L, x_id, d_g, 1.0, 0, None, None, *d_q, H.WHERE_PLUGIN))
        res["pack_one_field_device_ms"] = timed(lambda: lib.hpgmg_dense_pack(L, x_id, d_u, H.WHERE_PLUGIN, H.DENSE_CELL, H.DENSE_CHECK_FINITE))
    cells = float(n) ** 3
    res["flux_pass_min_bytes"] = 56.0 * cells
    res["flux_pass_TBps"] = 56.0 * cells / (res["flux_pass_device_ms"] * 1e-3) / 1e12
    res["pack_one_field_TBps"] = 16.0 * cells / (res["pack_one_field_device_ms"] * 1e-3) / 1e12      # 8 B in, 8 B out per cell (padding not counted)
    for p in dev:
        K.hpgmg_hip_free(p)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
