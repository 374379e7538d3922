#!/usr/bin/env python3
"""Times the user-problem API (hpgmg_amd/problem.py, hpgmg_user_* of include/hpgmg_fv.h) at 256^3, config 2's shape (7-pt Helmholtz,
Chebyshev, 2^3 boxes of 128^3): set_coefficients, set_rhs, solve (one F-cycle) and get_solution, with host (NumPy) and device input, plus
one pack and one unpack launch alone.  hipEvent pairs on the library's launch stream around each call; every call synchronises before it
returns, so the pair brackets all of its device work.  Prints one JSON line of medians in ms.

The time march, device arrays only: one step() of a backward-Euler and of a Crank-Nicolson march; the only route to the
backward-Euler update without a march -- a torch-formed right-hand side a alpha u + f, then solve(rhs, u0=u) into u, from the same state (skipped
without torch).  These three are timed alike, with the host clock between device synchronisations, since torch works on a stream of its own.  Then
the two passes of kernels/dense_step.hip alone (hook calls in a row between an event pair: step_rate's figure includes its fold launch and the
host's wait for the value) as ms and as 48 B per cell per second; set_shift.

The wave march, device arrays only, timed like the time march: one wave_step() of the average-acceleration rule; the same update
without a march from the same start -- torch forms the predictor and the right-hand side, solve(rhs, u0=predictor) into u, torch forms the acceleration
and the velocity (skipped without torch); the three passes of kernels/dense_wave.hip alone per hook call, against 72 / 64 / 48 B per cell
(wave_correct's and wave_init's figures include their fold launch and the host's wait for the two sums).

    python tools/user_problem_timing.py [--n 256] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

try:                      # before the project's libraries load: one HIP runtime per process (hpgmg_amd/problem.py)
    import torch
except ImportError:
    torch = None

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
        march_timing(args, lib, K, s, res, timed, d_f, d_u, f, alpha)
        wave_timing(args, lib, K, s, res, timed, d_f, d_u, f, alpha)
    for p in dev:
        K.hpgmg_hip_free(p)
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


def march_timing(args, lib, K, s, res, timed, d_f, d_u, f, alpha):
    """The time march on the solver whose coefficients are set from device arrays (module docstring)."""
    n, S, W = s.n, s._ptr, H.WHERE_PLUGIN
    dt, rtol = 1e-3, 1e-6
    L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
    info, rate = H.UserInfo(), ctypes.c_double()
    assert K.hpgmg_hip_memcpy_h2d(d_u, f.ctypes.data, f.nbytes) == 0                      # the state to start from: any finite field
    res["step_rtol"], res["step_dt"] = rtol, dt
    for theta in (0.5, 1.0):               # theta = 1 (backward Euler) last: the one update the route without a march can also make
        assert lib.hpgmg_user_start(S, d_u, d_f, None, W, dt, theta) == H.USER_OK
        out, cycles = [], []
        for _ in range(args.repeats + 1):                                                   # the first is the warm-up
            K.hpgmg_hip_sync()
            t0 = time.perf_counter()
            assert lib.hpgmg_user_step(S, d_f, None, W, 0.0, 0.0, rtol, ctypes.byref(info), ctypes.byref(rate)) == H.USER_OK
            K.hpgmg_hip_sync()
            out.append((time.perf_counter() - t0) * 1e3)
            cycles.append(info.vcycles)
        res[f"step_theta_{theta}_ms"] = statistics.median(out[1:])
        res[f"step_theta_{theta}_vcycles"] = cycles[1:]
    # the two passes alone, on the march's own vectors (their values do not matter to the time)
    nv = (ctypes.c_int * H.INFO_COUNT)()
    lib.hpgmg_level_info(L, nv)
    uold_id, w_id, calls = nv[H.INFO_NUM_VECTORS] - 2, nv[H.INFO_NUM_VECTORS] - 1, 20
    a, c = 1.0 / (theta * dt), (1.0 - theta) / theta

    def rhs_calls():
        for _ in range(calls):
            lib.hpgmg_step_rhs(L, H.VECTOR_F, H.VECTOR_U, uold_id, w_id, a, 0.0)
        K.hpgmg_hip_sync()

    def rate_calls():
        for _ in range(calls):
            lib.hpgmg_step_rate(L, w_id, H.VECTOR_TEMP, H.VECTOR_U, uold_id, a, c, ctypes.byref(rate))
    for name, fn in (("step_rhs", rhs_calls), ("step_rate", rate_calls)):
        fn()
        ms = timed(fn) / calls
        res[f"{name}_call_ms"] = ms
        res[f"{name}_TB_per_s"] = 48.0 * n ** 3 / (ms * 1e-3) / 1e12
    shifts = iter(range(1, 1000))
    res["set_shift_ms"] = timed(lambda: lib.hpgmg_user_set_shift(S, a + next(shifts)))
    if torch is None:
        res["torch_route_ms"] = None
        return
    dev = torch.device("cuda", torch.cuda.current_device())
    t_alpha, t_f, t_u = torch.from_numpy(alpha).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(f).to(dev)
    s.set_shift(1.0 / dt)
    out, cycles = [], []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rhs = s.a * t_alpha * t_u + t_f
        _, i = s.solve(rhs, rtol=rtol, u0=t_u, out=t_u)
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        cycles.append(i.vcycles)
    res["torch_route_ms"] = statistics.median(out[1:])
    res["torch_route_vcycles"] = cycles[1:]


def wave_timing(args, lib, K, s, res, timed, d_f, d_u, f, alpha):
    """The wave march on the same solver, after march_timing (module docstring): d_u holds the start state and, as a second array, the start velocity."""
    n, S, W = s.n, s._ptr, H.WHERE_PLUGIN
    dt, rtol, beta, gamma, sigma = 1e-3, 1e-6, 0.25, 0.5, 0.0
    L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
    info = H.UserWaveInfo()
    assert K.hpgmg_hip_memcpy_h2d(d_u, f.ctypes.data, f.nbytes) == 0
    res["wave_rtol"], res["wave_dt"] = rtol, dt
    assert lib.hpgmg_user_wave_start(S, d_u, d_u, d_f, None, W, dt, beta, gamma, sigma, ctypes.byref(info)) == H.USER_OK
    q0 = np.empty((n, n, n))
    assert lib.hpgmg_user_get_acceleration(S, q0.ctypes.data, H.WHERE_HOST) == H.USER_OK
    out, cycles, energy = [], [], []
    for _ in range(args.repeats + 1):                                                   # the first is the warm-up
        K.hpgmg_hip_sync()
        t0 = time.perf_counter()
        assert lib.hpgmg_user_wave_step(S, d_f, None, W, 0.0, rtol, ctypes.byref(info)) == H.USER_OK
        K.hpgmg_hip_sync()
        out.append((time.perf_counter() - t0) * 1e3)
        cycles.append(info.vcycles)
        energy.append(info.kinetic + info.potential)
    res["wave_step_ms"] = statistics.median(out[1:])
    res["wave_step_vcycles"] = cycles[1:]
    res["wave_step_energy"] = energy[1:]
    # the three passes alone, on the march's own vectors (their values do not matter to the time)
    nv = (ctypes.c_int * H.INFO_COUNT)()
    lib.hpgmg_level_info(L, nv)
    uold_id, v_id, q_id, calls = nv[H.INFO_NUM_VECTORS] - 3, nv[H.INFO_NUM_VECTORS] - 2, nv[H.INFO_NUM_VECTORS] - 1, 20
    a, cq, cg = s._wave_shift(dt, beta, gamma, sigma), 1.0 / (beta * dt * dt), gamma * dt
    sums = (ctypes.c_double * 2)()
    took = {}

    def predict_calls():
        for _ in range(calls):
            took["wave_predict"] = lib.hpgmg_wave_predict(L, H.VECTOR_U, uold_id, v_id, H.VECTOR_F, q_id, dt, 0.0, 0.0, a, sigma)
        K.hpgmg_hip_sync()

    def correct_calls():
        for _ in range(calls):
            took["wave_correct"] = lib.hpgmg_wave_correct(L, q_id, v_id, H.VECTOR_U, uold_id, H.VECTOR_F, H.VECTOR_TEMP, a, cq, cg, sums)

    def init_calls():
        for _ in range(calls):
            took["wave_init"] = lib.hpgmg_wave_init(L, q_id, H.VECTOR_TEMP, H.VECTOR_U, v_id, H.VECTOR_F, a, sigma, sums)
    for name, fn, nbytes in (("wave_predict", predict_calls, 72.0), ("wave_correct", correct_calls, 64.0), ("wave_init", init_calls, 48.0)):
        fn()
        ms = timed(fn) / calls
        assert took[name] == 1, (name, took)                                          # the kernel ran, not the portable form
        res[f"{name}_call_ms"] = ms
        res[f"{name}_TB_per_s"] = nbytes * n ** 3 / (ms * 1e-3) / 1e12
    if torch is None:
        res["wave_torch_route_ms"] = None
        return
    dev = torch.device("cuda", torch.cuda.current_device())
    t_alpha, t_f = torch.from_numpy(alpha).to(dev), torch.from_numpy(f).to(dev)
    t_u, t_v, t_q = torch.from_numpy(f).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(q0).to(dev)
    s.set_shift(a)
    cu, cv = dt * dt * (0.5 - beta), dt * (1.0 - gamma)
    out, cycles = [], []
    for _ in range(args.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ut = t_u + dt * t_v + cu * t_q
        vt = t_v + cv * t_q
        rhs = t_f + t_alpha * (a * ut - sigma * vt)
        _, i = s.solve(rhs, rtol=rtol, u0=ut, out=t_u)
        t_q = (t_u - ut) * cq
        t_v = vt + cg * t_q
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
        cycles.append(i.vcycles)
    res["wave_torch_route_ms"] = statistics.median(out[1:])
    res["wave_torch_route_vcycles"] = cycles[1:]


if __name__ == "__main__":
    main()
