"""Robin walls on the MI355X: the HIP build (kernels/dense_boundary.hip boundary_check_kappa_kernel, boundary_store_walls_kernel
and the kappa forms of the lifted pack, the flux and the interpolation correction) equals the CPU oracle bit for bit for the lifted right-hand
side, apply(boundary=), every level's beta vectors and eigenvalue estimate, and u of fmg, mg and pcg; kappa = 0 gives the Neumann solver's
bytes; torch tensors equal the NumPy path.

Shapes: N = 64 in boxes of 32 (2^3 boxes: every box touches three walls) and N = 48 in boxes of 16 (3^3 boxes: boxes on zero, one, two and
three walls, and a 3^3 bottom level).
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
from test_gpu_user_problem import DeviceArrays
from user_problem_lib import random_coefficients
from user_robin_lib import ALL, CORNERS, kappa_of, level_walls, neumann_of

pytestmark = pytest.mark.gpu

KEYS = ("F", "y", "u_fmg", "u_mg", "u_pcg")


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _run(lib, n, box_dim, faces, smoother, a, coef, kappa, f, g, x, device=None):
    """F (the lifted right-hand side as packed), A_R x - T(g), u of fmg, mg and pcg with their infos, and every level's beta vectors and
    eigenvalue estimate, through the C entry points.  kappa None: the plain set_coefficients (a solver without a Robin face)."""
    alpha, bi, bj, bk = coef
    out = {}
    with Solver(n, box_dim=box_dim, bc=faces, smoother=smoother, a=a, b=1.0, lib=lib) as s:
        S, info, shift = s._ptr, H.UserInfo(), ctypes.c_double()
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        D = device
        if D is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = {k: np.empty((n, n, n)) for k in KEYS}
            ptr = {k: v.ctypes.data for k, v in outs.items()}
        else:
            put, w = D.put, H.WHERE_PLUGIN
            ptr = {k: D.empty(f.nbytes) for k in KEYS}
        if kappa is None:
            assert lib.hpgmg_user_set_coefficients(S, put(alpha), put(bi), put(bj), put(bk), w) == 0
        else:
            assert lib.hpgmg_user_set_coefficients_robin(S, put(alpha), put(bi), put(bj), put(bk), put(kappa), w) == 0
        out["levels"] = level_walls(lib, s)
        pf, pg = put(f), put(g)
        assert lib.hpgmg_user_set_max_iterations(S, 30) == 0
        for method, key, rtol in ((H.USER_FMG, "u_fmg", 1e-10), (H.USER_MG, "u_mg", 1e-10), (H.USER_PCG, "u_pcg", 1e-8)):
            assert lib.hpgmg_user_set_rhs_dirichlet(S, pf, pg, w, ctypes.byref(shift)) == 0
            if key == "u_fmg":
                assert lib.hpgmg_dense_unpack(L, H.VECTOR_F, ptr["F"], w) == 0
            assert lib.hpgmg_user_solve(S, method, rtol, None, w, ctypes.byref(info)) == 0
            out[key + "_info"] = (info.norm_of_residual, info.norm_of_f, info.vcycles, info.mean_shift, info.converged)
            assert lib.hpgmg_user_get_solution(S, ptr[key], w) == 0
        assert lib.hpgmg_user_apply_dirichlet(S, put(x), pg, ptr["y"], w) == 0
        for k in KEYS:
            out[k] = outs[k] if D is None else D.get(ptr[k], f.shape)
    return out


def _same(got, ref):
    for key in KEYS:
        assert got[key].tobytes() == ref[key].tobytes(), key
    for key in ("u_fmg_info", "u_mg_info", "u_pcg_info"):
        assert got[key] == ref[key], key
    assert len(got["levels"]) == len(ref["levels"]) >= 3
    for l, ((vecs, eig), (vecs_ref, eig_ref)) in enumerate(zip(got["levels"], ref["levels"])):
        assert eig == eig_ref, l
        for axis, (boxes, boxes_ref) in enumerate(zip(vecs, vecs_ref)):
            for (low, v), (low_ref, v_ref) in zip(boxes, boxes_ref):
                assert low == low_ref and v.tobytes() == v_ref.tobytes(), (l, axis, low)      # whole padded boxes: walls, interior and ghosts


def _inputs(n, a, seed):
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=seed)
    rng = np.random.default_rng(n + 2)
    return coef, rng.random((n, n, n)) - 0.3, rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 4.0 - 2.0


CASES = [  # n, box_dim, walls, smoother, a, entry: Chebyshev on both walls, shapes, operators and entries; one GSRB and one Jacobi case
    (64, 32, CORNERS, "cheby", 1.0, "host"),
    (64, 32, CORNERS, "cheby", 0.0, "device"),
    (64, 32, ALL, "cheby", 0.0, "host"),
    (64, 32, ALL, "cheby", 1.0, "device"),
    (64, 32, ALL, "gsrb", 1.0, "host"),
    (48, 16, CORNERS, "cheby", 0.0, "host"),
    (48, 16, CORNERS, "cheby", 1.0, "device"),
    (48, 16, ALL, "cheby", 1.0, "host"),
    (48, 16, ALL, "cheby", 0.0, "device"),
    (48, 16, CORNERS, "jacobi", 0.0, "device"),
]


@pytest.mark.parametrize("n,box_dim,walls,smoother,a,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, walls, smoother, a, entry):
    hip, oracle, K = libs
    coef, f, x, g = _inputs(n, a, 800 + n + len(smoother) + int(a))
    kappa = kappa_of(n, walls)
    ref = _run(oracle, n, box_dim, walls, smoother, a, coef, kappa, f, g, x)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = _run(hip, n, box_dim, walls, smoother, a, coef, kappa, f, g, x, device=D)
    finally:
        if D:
            D.free()
    _same(got, ref)
    assert ref["u_mg_info"][4] and ref["u_pcg_info"][4]
    assert ref["u_fmg_info"][3] == 0.0                         # kappa > 0: six Robin walls are not singular, nothing is subtracted


@pytest.mark.parametrize("walls,a", [(CORNERS, 1.0), (ALL, 0.0)])
def test_kappa_zero_gives_the_neumann_solvers_bytes(libs, walls, a):
    hip, _, K = libs
    n, box_dim = 48, 16
    coef, f, x, g = _inputs(n, a, 900 + int(a))
    D = DeviceArrays(K)
    try:
        ref = _run(hip, n, box_dim, neumann_of(walls), "cheby", a, coef, None, f, g, x, device=D)
        got = _run(hip, n, box_dim, walls, "cheby", a, coef, np.zeros((6, n, n)), f, g, x, device=D)
    finally:
        D.free()
    _same(got, ref)
    if walls == ALL and a == 0.0:
        assert ref["u_fmg_info"][3] != 0.0                     # the singular case went through the mean shift


def test_bad_kappa_is_reported_from_the_device(libs):
    """hpgmg_boundary_check_kappa's kernel: not finite anywhere, negative on a Robin face only, and the any-positive bit."""
    hip, _, K = libs
    n = 48
    D = DeviceArrays(K)
    try:
        with Solver(n, box_dim=16, bc=CORNERS, lib=hip) as s:
            L = hip.hpgmg_solver_level(hip.hpgmg_user_solver_of(s._ptr), 0)
            mask = sum(1 << f for f, kind in enumerate(CORNERS) if kind == "convective")
            any_positive = ctypes.c_int(-1)
            for face, value, status, positive in ((0, -1.0, H.DENSE_OUT_OF_RANGE, 0), (1, -1.0, 0, 0), (1, np.nan, H.DENSE_NOT_FINITE, 0),
                                                  (3, np.inf, H.DENSE_NOT_FINITE, 0), (4, 2.0, 0, 1), (2, 2.0, 0, 0)):
                kappa = np.zeros((6, n, n))
                kappa[face, n - 1, n - 1] = value
                for where, p in ((H.WHERE_HOST, kappa.ctypes.data), (H.WHERE_PLUGIN, D.put(kappa))):
                    assert hip.hpgmg_boundary_check_kappa(L, p, where, mask, ctypes.byref(any_positive)) == status, (face, value)
                    assert any_positive.value == positive, (face, value)
    finally:
        D.free()


def test_torch_tensors(libs):
    """A child process that imports torch first: Robin walls with tensors equal the NumPy path bitwise, and mixed kinds are refused."""
    worker = os.path.join(ROOT, "tests", "user_robin_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
