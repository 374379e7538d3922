"""method="pcg" on the MI355X (kernels/pcg.hip): each of the three fused passes equals the portable form of the CPU oracle bit
for bit -- vectors and sums, whose order is a function of the level's geometry alone -- and so do whole solves: u, the iteration count and the
residual, for every smoother and wall kind, from host arrays, device arrays and (a child process that imports torch first) tensors.
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
from user_neumann_lib import SIDES
from user_pcg_lib import contrast_problem
from user_problem_lib import random_coefficients

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _hooks(lib, n, box_dim, a, coef, vectors, alpha_cg, bc="dirichlet"):
    """The three passes on random vectors of the finest level of a user solver: what each leaves, and whether the plugin's kernel took it."""
    out = {}
    with Solver(n, box_dim=box_dim, bc=bc, a=a, b=0.9, lib=lib) as s:
        s.set_coefficients(*coef)
        s.solve(np.ones((n, n, n)), method="pcg", max_iter=1)            # grows the levels by the three vectors of the method
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0)
        p_id = lib.hpgmg_vectors_reserved()
        Ap_id, z_id = p_id + 1, p_id + 2
        ids = {"x": H.VECTOR_U, "r": H.VECTOR_R, "p": p_id, "z": z_id}

        def put(name):
            assert lib.hpgmg_dense_pack(L, ids[name], vectors[name].ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0

        def get(vid):
            v = np.empty((n, n, n))
            assert lib.hpgmg_dense_unpack(L, vid, v.ctypes.data, H.WHERE_HOST) == 0
            return v

        for name in ids:
            put(name)
        value = ctypes.c_double()
        out["took_apply_dot"] = lib.hpgmg_pcg_apply_dot(L, Ap_id, p_id, a, 0.9, ctypes.byref(value))
        out["pAp"], out["Ap"] = value.value, get(Ap_id)
        out["took_update"] = lib.hpgmg_pcg_update(L, H.VECTOR_U, H.VECTOR_R, p_id, Ap_id, alpha_cg, ctypes.byref(value))
        out["rmax"], out["x"], out["r"] = value.value, get(H.VECTOR_U), get(H.VECTOR_R)
        out["took_dot"] = lib.hpgmg_pcg_dot(L, H.VECTOR_R, z_id, ctypes.byref(value))
        out["rz"] = value.value
    return out


# rows shorter than a wave; 3^3 boxes; 2^3 boxes; one box with rows longer than a wave
@pytest.mark.parametrize("n,box_dim", [(16, 8), (48, 16), (64, 32), (128, 128)])
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_each_pass_equals_the_oracle(libs, n, box_dim, a):
    hip, oracle, _ = libs
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=900 + n + int(a))
    rng = np.random.default_rng(n + int(10 * a))
    vectors = {name: rng.random((n, n, n)) * 2.0 - 1.0 for name in ("x", "r", "p", "z")}
    ref = _hooks(oracle, n, box_dim, a, coef, vectors, 0.37)
    got = _hooks(hip, n, box_dim, a, coef, vectors, 0.37)
    assert (got["took_apply_dot"], got["took_update"], got["took_dot"]) == (1, 1, 1)
    assert (ref["took_apply_dot"], ref["took_update"], ref["took_dot"]) == (0, 0, 0)
    for key in ("Ap", "x", "r"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("pAp", "rmax", "rz"):
        assert got[key] == ref[key], (key, got[key], ref[key])
    assert ref["rmax"] == np.abs(ref["r"]).max() and ref["pAp"] != 0.0 and ref["rz"] != 0.0


# the neighbour paths of the stencil pass that Dirichlet walls do not take: a periodic wrap (2^3 boxes, and one box that is its own neighbour), Neumann walls
@pytest.mark.parametrize("n,box_dim,bc,a", [(32, 16, "periodic", 1.3), (16, 16, "periodic", 0.0), (48, 16, SIDES, 0.0)])
def test_each_pass_equals_the_oracle_on_other_walls(libs, n, box_dim, bc, a):
    hip, oracle, _ = libs
    coef = random_coefficients(n, "periodic" if bc == "periodic" else "dirichlet", a != 0.0, seed=950 + n + int(a))
    rng = np.random.default_rng(2 * n + int(10 * a))
    vectors = {name: rng.random((n, n, n)) * 2.0 - 1.0 for name in ("x", "r", "p", "z")}
    ref = _hooks(oracle, n, box_dim, a, coef, vectors, -0.21, bc=bc)
    got = _hooks(hip, n, box_dim, a, coef, vectors, -0.21, bc=bc)
    assert (got["took_apply_dot"], got["took_update"], got["took_dot"]) == (1, 1, 1)
    for key in ("Ap", "x", "r"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("pAp", "rmax", "rz"):
        assert got[key] == ref[key], (key, got[key], ref[key])


def _solve(lib, n, box_dim, bc, smoother, a, coef, f, g, device=None):
    with Solver(n, box_dim=box_dim, bc=bc, smoother=smoother, a=a, b=1.0, lib=lib) as s:
        if device is None:
            s.set_coefficients(*coef)
            u, info = s.solve(f, method="pcg", rtol=1e-9, max_iter=40, boundary=g)
            return u, info
        # device arrays through the C entry points
        D, S, info, shift = device, s._ptr, H.UserInfo(), ctypes.c_double()
        assert lib.hpgmg_user_set_coefficients(S, *[D.put(c) for c in coef], H.WHERE_PLUGIN) == 0
        if g is None:
            assert lib.hpgmg_user_set_rhs(S, D.put(f), H.WHERE_PLUGIN, ctypes.byref(shift)) == 0
        else:
            assert lib.hpgmg_user_set_rhs_dirichlet(S, D.put(f), D.put(g), H.WHERE_PLUGIN, ctypes.byref(shift)) == 0
        assert lib.hpgmg_user_set_max_iterations(S, 40) == 0
        assert lib.hpgmg_user_solve(S, H.USER_PCG, 1e-9, None, H.WHERE_PLUGIN, ctypes.byref(info)) == 0
        pu = D.empty(f.nbytes)
        assert lib.hpgmg_user_get_solution(S, pu, H.WHERE_PLUGIN) == 0
        from hpgmg_amd.problem import SolveInfo
        return D.get(pu, f.shape), SolveInfo(info.norm_of_residual, info.norm_of_f, info.vcycles, bool(info.converged), info.mean_shift)


CASES = [  # n, box_dim, bc, smoother, a, boundary values, entry
    (64, 32, "dirichlet", "cheby", 1.0, True, "host"),
    (64, 32, "periodic", "gsrb", 0.0, False, "device"),
    (64, 32, SIDES, "jacobi", 0.0, True, "host"),
    (48, 16, "periodic", "cheby", 1.3, False, "host"),
    (48, 16, SIDES, "gsrb", 0.0, True, "device"),
    (48, 16, "dirichlet", "jacobi", 1.0, True, "host"),
]


@pytest.mark.parametrize("n,box_dim,bc,smoother,a,boundary,entry", CASES)
def test_whole_solves_equal_the_oracle(libs, n, box_dim, bc, smoother, a, boundary, entry):
    hip, oracle, K = libs
    shape_bc = "periodic" if bc == "periodic" else "dirichlet"
    coef = random_coefficients(n, shape_bc, a != 0.0, seed=700 + n + len(smoother) + int(a))
    rng = np.random.default_rng(n + 3)
    f = rng.random((n, n, n)) - 0.3
    g = rng.random((6, n, n)) * 2.0 - 1.0 if boundary else None
    u_ref, ref = _solve(oracle, n, box_dim, bc, smoother, a, coef, f, g)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        u, info = _solve(hip, n, box_dim, bc, smoother, a, coef, f, g, device=D)
    finally:
        if D:
            D.free()
    assert ref.vcycles >= 2          # (48^3 periodic Helmholtz stops at its 40 iterations: the parity holds for a solve that ends either way)
    assert np.array_equal(u, u_ref)
    assert (info.vcycles, info.residual, info.norm_f, info.converged, info.mean_shift) == (ref.vcycles, ref.residual, ref.norm_f, ref.converged, ref.mean_shift)


def test_contrast_problem_converges_in_the_oracles_count(libs):
    hip, oracle, _ = libs
    bi, bj, bk, f = contrast_problem(64, 100.0)
    infos = []
    for lib in (oracle, hip):
        with Solver(64, box_dim=32, lib=lib) as s:
            s.set_coefficients(None, bi, bj, bk)
            _, mg = s.solve(f, method="mg", rtol=1e-8)
            _, info = s.solve(f, method="pcg", rtol=1e-8, max_iter=50)
        assert not mg.converged and info.converged
        infos.append(info)
    print(f"contrast 100 at 64^3: {infos[1].vcycles} iterations, rel {infos[1].residual / infos[1].norm_f:.3e}")
    assert infos[1].vcycles == infos[0].vcycles and infos[1].residual == infos[0].residual


def test_torch_tensors(libs):
    """A child process that imports torch first: method="pcg" on tensors equals the NumPy path bitwise."""
    worker = os.path.join(ROOT, "tests", "user_pcg_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
