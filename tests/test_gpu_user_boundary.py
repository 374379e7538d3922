"""Inhomogeneous Dirichlet values on the MI355X: the HIP build (kernels/dense_boundary.hip) equals the CPU oracle bit for bit for the lifted
right-hand side, apply(boundary=) and u of both methods; torch tensors equal the NumPy path; at 256^3 a zero g is the homogeneous problem,
the boundary F-cycle meets the accuracy bound measured on the oracle, and its V-cycles stay on the fused brick and sweep-pair kernels.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays, _counters
from user_boundary_lib import exact, manufactured
from user_problem_lib import random_coefficients

pytestmark = pytest.mark.gpu

FMG_FACTOR = 1.5            # test_oracle_user_boundary.py: measured 0.89 - 0.95 on the oracle at N = 16 .. 64


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _run(lib, n, box_dim, smoother, a, coef, f, g, x, device=None):
    """F (the lifted right-hand side as packed), A0 x - T(g), u of fmg, u of mg and the infos, through the C entry points."""
    alpha, bi, bj, bk = coef
    out = {}
    with Solver(n, box_dim=box_dim, smoother=smoother, a=a, b=1.0, lib=lib) as s:
        S, info, shift = s._ptr, H.UserInfo(), ctypes.c_double()
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        D = device
        if D is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = {k: np.empty((n, n, n)) for k in ("F", "y", "u_fmg", "u_mg")}
            ptr = {k: v.ctypes.data for k, v in outs.items()}
        else:
            put, w = D.put, H.WHERE_PLUGIN
            ptr = {k: D.empty(f.nbytes) for k in ("F", "y", "u_fmg", "u_mg")}
        assert lib.hpgmg_user_set_coefficients(S, put(alpha), put(bi), put(bj), put(bk), w) == 0
        pf, pg = put(f), put(g)
        for method, key in ((H.USER_FMG, "u_fmg"), (H.USER_MG, "u_mg")):
            assert lib.hpgmg_user_set_rhs_dirichlet(S, pf, pg, w, ctypes.byref(shift)) == 0
            if key == "u_fmg":
                assert lib.hpgmg_dense_unpack(L, H.VECTOR_F, ptr["F"], w) == 0
            assert lib.hpgmg_user_solve(S, method, 1e-10, None, w, ctypes.byref(info)) == 0
            out[key + "_info"] = (info.norm_of_residual, info.norm_of_f, info.vcycles)
            assert lib.hpgmg_user_get_solution(S, ptr[key], w) == 0
        assert lib.hpgmg_user_apply_dirichlet(S, put(x), pg, ptr["y"], w) == 0
        for k in ("F", "y", "u_fmg", "u_mg"):
            out[k] = outs[k] if D is None else D.get(ptr[k], f.shape)
    return out


CASES = [  # n, box_dim, smoother, a, entry
    (64, 32, "cheby", 1.0, "host"),
    (64, 32, "cheby", 0.0, "device"),
    (64, 32, "gsrb", 1.0, "device"),
    (64, 32, "jacobi", 0.0, "host"),
    (48, 16, "cheby", 0.0, "host"),
    (48, 16, "gsrb", 0.0, "host"),
    (48, 16, "jacobi", 1.0, "device"),
]


@pytest.mark.parametrize("n,box_dim,smoother,a,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, smoother, a, entry):
    hip, oracle, K = libs
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=500 + n + len(smoother) + int(a))
    rng = np.random.default_rng(n + 1)
    f, x, g = rng.random((n, n, n)) - 0.3, rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 4.0 - 2.0
    ref = _run(oracle, n, box_dim, smoother, a, coef, f, g, x)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = _run(hip, n, box_dim, smoother, a, coef, f, g, x, device=D)
    finally:
        if D:
            D.free()
    for key in ("F", "y", "u_fmg", "u_mg"):
        assert np.array_equal(got[key], ref[key]), key
    assert got["u_fmg_info"] == ref["u_fmg_info"] and got["u_mg_info"] == ref["u_mg_info"]


def test_torch_tensors(libs):
    """A child process that imports torch first: boundary= with tensors equals the NumPy path bitwise."""
    worker = os.path.join(ROOT, "tests", "user_boundary_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr


def test_helmholtz_256_manufactured_on_the_fast_path(libs):
    hip, _, K = libs
    n = 256
    alpha, bi, bj, bk, f, u_star = manufactured(n, 1.0, 1.0)
    with Solver(n, smoother="cheby", a=1.0, b=1.0, lib=hip) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u_h, info_h = s.solve(f, method="fmg")
        u_z, info_z = s.solve(f, method="fmg", boundary=np.zeros((6, n, n)))
        assert np.array_equal(u_z, u_h) and info_z.residual == info_h.residual
        g = s.boundary_from(exact)
        before = _counters(hip, K)
        u_fmg, info = s.solve(f, method="fmg", boundary=g)
        after = _counters(hip, K)
        u_mg, info_mg = s.solve(f, method="mg", rtol=1e-12, boundary=g)
    assert after[0] > before[0], "no brick visits: the boundary F-cycle's V-cycles left the fused kernels"
    assert after[1] > before[1], "no sweep-pair launches: the boundary F-cycle's V-cycles left the fused Chebyshev kernels"
    assert info.vcycles == 1 and info_mg.converged
    e_fmg, e_mg = np.abs(u_fmg - u_star).max(), np.abs(u_mg - u_star).max()
    print(f"256^3 manufactured: F-cycle error {e_fmg:.3e}, V-cycles {e_mg:.3e}, ratio {e_fmg / e_mg:.3f}")
    assert e_fmg <= FMG_FACTOR * e_mg, (e_fmg, e_mg)
