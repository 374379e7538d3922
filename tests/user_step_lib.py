"""Helpers of the time-stepping tests (Solver.start / step / rate / set_shift): the solvers and data the tests march, the spatial
operator L(u; g) = apply(u, boundary=g) - a alpha u from the public API, the rounding scale of that difference, and a march through the C entry
points that takes its arrays from the host or from device memory.
"""
import ctypes
import hashlib

import numpy as np

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from user_flux_lib import SOLVERS, boundary_for, kappa_for
from user_problem_lib import random_coefficients

EPS = np.finfo(np.float64).eps
B = 0.7                                  # the operator's b in every march below
# L(u; g) = apply(u, g) - a alpha u cancels the a alpha u term apply added: what is left carries the rounding of both, which scales with
# rounding_scale().  ROUNDING_MEASURED is the largest  |error| / rounding_scale  seen on the CPU oracle over the scheme-identity and
# rate-consistency checks of tests/test_oracle_user_step.py (every configuration, theta and step; the tests print theirs): 0.307, reached by the
# rate check.  The tests gate at ROUNDING_FACTOR times it: the one rounding gate of the rate check and of the dt change mid-march.  The scheme
# identity alone stays below 0.058, and that check is held to ROUNDING_FACTOR times its own constant.
ROUNDING_MEASURED = 0.31
ROUNDING_MEASURED_IDENTITY = 0.058
ROUNDING_FACTOR = 10.0


def problem(name, n, seed):
    """(bc of Solver, (alpha, beta_i, beta_j, beta_k), kappa or None) of the wall configuration `name` of user_flux_lib.SOLVERS."""
    bc = "periodic" if name == "periodic" else "dirichlet"
    return SOLVERS[name], random_coefficients(n, bc, True, seed=seed), kappa_for(name, n)


def data(name, n, seed, k):
    """f and the wall data of time level k: different arrays for every k."""
    f = np.random.default_rng(seed + 10 * k).random((n, n, n)) * 4.0 - 2.0
    return f, boundary_for(name, n, seed + 10 * k + 1)


def initial(n, seed):
    return np.random.default_rng(seed + 5).random((n, n, n)) * 2.0 - 1.0


def spatial(s, alpha, u, g):
    """L(u; g) = -b div(beta grad u) with the walls' data, through the public API and the solver's current a."""
    return s.apply(u, boundary=g) - s.a * alpha * u


def rounding_scale(s, coef, *us):
    """eps (a |alpha u|_inf + 12 b max(beta) |u|_inf / h^2), over the given states."""
    alpha, betas = coef[0], coef[1:]
    top = max(np.abs(u).max() for u in us)
    au = max(np.abs(alpha * u).max() for u in us)
    return EPS * (s.a * au + 12.0 * s.b * max(x.max() for x in betas) * top / (s.h * s.h))


def rounding_gate(s, coef, *us):
    return ROUNDING_FACTOR * ROUNDING_MEASURED * rounding_scale(s, coef, *us)


def digests(steps):
    """One sha256 per step of march()'s result over u, the rate array, the info fields and the rate: what a worker process prints of its march."""
    return [hashlib.sha256(s[1].tobytes() + s[2].tobytes() + repr((s[0], s[3], s[4])).encode()).hexdigest() for s in steps]


def host_arrays():
    return (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST


def march(lib, n, box_dim, name, seed, theta, dts, rtol, device=None, spoil=None, watch=None, coef=None):
    """start at time level 0, then one step per entry of `dts` (time level k = 1, 2, ...) through the C entry points; device = DeviceArrays: every
    array lives in device memory.  spoil = (k, "f" | "g"): before step k a step with a NaN in that array is tried, and its status recorded.
    watch(k, done): called right before (done = 0) and right after (done = 1) the hpgmg_user_step call of step k (counters).
    coef: (alpha, beta_i, beta_j, beta_k) in the place of problem()'s smooth fields, which take seconds to make at 256^3.
    Returns [(status, u, rate array, info fields, rate)] per step, with ("refused", status) entries where a spoiled step was tried."""
    if coef is None:
        bc, coef, kappa = problem(name, n, seed)
    else:
        bc, kappa = SOLVERS[name], kappa_for(name, n)
    put, w = host_arrays() if device is None else (device.put, H.WHERE_PLUGIN)
    out = []

    def fetch(s, call):
        if device is None:
            a = np.full((n, n, n), 7.0)
            assert call(s._ptr, a.ctypes.data, w) == H.USER_OK
            return a
        p = device.put(np.full((n, n, n), 7.0))
        assert call(s._ptr, p, w) == H.USER_OK
        return device.get(p, (n, n, n))

    with Solver(n, box_dim=box_dim, bc=bc, a=1.0, b=B, lib=lib) as s:
        alpha, bi, bj, bk = coef
        if kappa is None:
            assert lib.hpgmg_user_set_coefficients(s._ptr, put(alpha), put(bi), put(bj), put(bk), w) == H.USER_OK
        else:
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, put(alpha), put(bi), put(bj), put(bk), put(kappa), w) == H.USER_OK
        (f, g), u0 = data(name, n, seed, 0), initial(n, seed)          # named: a host pointer must outlive the call
        assert lib.hpgmg_user_start(s._ptr, put(u0), put(f), put(g), w, dts[0], theta) == H.USER_OK
        for k, dt in enumerate(dts, start=1):
            f, g = data(name, n, seed, k)
            info, rate = H.UserInfo(), ctypes.c_double(-1.0)
            if spoil is not None and spoil[0] == k:
                bad_f, bad_g = f.copy(), None if g is None else g.copy()
                if spoil[1] == "f":
                    bad_f[n - 1, 0, n // 2] = np.nan
                else:
                    bad_g[3, n - 1, 1] = np.nan
                out.append(("refused", lib.hpgmg_user_step(s._ptr, put(bad_f), put(bad_g), w, dt, theta, rtol, ctypes.byref(info), ctypes.byref(rate))))
            pf, pg = put(f), put(g)
            if watch:
                watch(k, 0)
            st = lib.hpgmg_user_step(s._ptr, pf, pg, w, dt if k == 1 or dt != dts[k - 2] else 0.0, theta if k == 1 else 0.0, rtol,
                                     ctypes.byref(info), ctypes.byref(rate))
            if watch:
                watch(k, 1)
            fields = (info.norm_of_residual, info.norm_of_f, info.mean_shift, info.vcycles, info.converged)
            out.append((st, fetch(s, lib.hpgmg_user_get_solution), fetch(s, lib.hpgmg_user_get_rate), fields, rate.value))
            if device is not None:
                device.free()
    return out
