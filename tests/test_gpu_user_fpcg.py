"""method="fpcg" on the MI355X (kernels/pcg.hip pcg_dot2_kernel / pcg_fold2_kernel): the one pass for r.z and Ap.z equals the
portable form of the CPU oracle bit for bit, both values, and two hpgmg_pcg_dot calls; whole fpcg solves equal the oracle's -- u, the iteration
count and the residual -- whichever way they end; and method="pcg", whose fold kernel stands next to the new one, still equals the oracle.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver, SolveInfo
from hpgmg_testlib import Backend
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


def _dot2(lib, n, box_dim, vectors, same=False):
    """hpgmg_pcg_dot2 on random vectors of the finest level of a user solver, and the two hpgmg_pcg_dot calls it stands for."""
    with Solver(n, box_dim=box_dim, a=1.0, b=0.9, lib=lib) as s:
        s.solve(np.ones((n, n, n)), method="fpcg", max_iter=1)           # grows the levels by the three vectors of the method
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0)
        p_id = lib.hpgmg_vectors_reserved()
        ids = {"a": H.VECTOR_R, "c": p_id + 1, "b": p_id + 2}
        for name, vid in ids.items():
            assert lib.hpgmg_dense_pack(L, vid, vectors[name].ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0
        c_id = ids["a"] if same else ids["c"]
        ab, cb, one, two = (ctypes.c_double() for _ in range(4))
        took = lib.hpgmg_pcg_dot2(L, ids["a"], c_id, ids["b"], ctypes.byref(ab), ctypes.byref(cb))
        lib.hpgmg_pcg_dot(L, ids["a"], ids["b"], ctypes.byref(one))
        lib.hpgmg_pcg_dot(L, c_id, ids["b"], ctypes.byref(two))
    return took, ab.value, cb.value, one.value, two.value


# rows shorter than a wave (75 % idle lanes); 3^3 boxes; 2^3 boxes; one box with rows longer than a wave (512 workgroups); and 11^3 boxes of 8:
# 1331 workgroup values, more than the fold's 1024 lanes and no multiple of its chunk = 2 -- the in-place part of the fold and its ragged end
@pytest.mark.parametrize("n,box_dim", [(16, 8), (48, 16), (64, 32), (128, 128), (88, 8)])
def test_dot2_equals_the_oracle_and_two_dots(libs, n, box_dim):
    hip, oracle, _ = libs
    rng = np.random.default_rng(300 + n)
    vectors = {name: rng.random((n, n, n)) * 2.0 - 1.0 for name in ("a", "c", "b")}
    ref = _dot2(oracle, n, box_dim, vectors)
    got = _dot2(hip, n, box_dim, vectors)
    assert got[0] == 1 and ref[0] == 0           # the kernel took it; the oracle ran the portable form
    assert got[1] == ref[1] and got[2] == ref[2], (got, ref)
    assert got[1] == got[3] and got[2] == got[4], got
    assert ref[1] != 0.0 and ref[2] != 0.0 and ref[1] != ref[2]


def test_dot2_with_one_vector_twice(libs):
    hip, oracle, _ = libs
    n, box_dim = 48, 16
    rng = np.random.default_rng(77)
    vectors = {name: rng.random((n, n, n)) * 2.0 - 1.0 for name in ("a", "c", "b")}
    got = _dot2(hip, n, box_dim, vectors, same=True)
    ref = _dot2(oracle, n, box_dim, vectors, same=True)
    assert got[0] == 1
    assert got[1] == got[2] == got[3] == ref[1] == ref[2] != 0.0


def _solve(lib, method, n, box_dim, bc, smoother, a, coef, f, g, device=None):
    with Solver(n, box_dim=box_dim, bc=bc, smoother=smoother, a=a, b=1.0, lib=lib) as s:
        if device is None:
            s.set_coefficients(*coef)
            return s.solve(f, method=method, rtol=1e-9, max_iter=40, boundary=g)
        # device arrays through the C entry points
        D, S, info, shift = device, s._ptr, H.UserInfo(), ctypes.c_double()
        assert lib.hpgmg_user_set_coefficients(S, *[D.put(c) for c in coef], H.WHERE_PLUGIN) == 0
        if g is None:
            assert lib.hpgmg_user_set_rhs(S, D.put(f), H.WHERE_PLUGIN, ctypes.byref(shift)) == 0
        else:
            assert lib.hpgmg_user_set_rhs_dirichlet(S, D.put(f), D.put(g), H.WHERE_PLUGIN, ctypes.byref(shift)) == 0
        assert lib.hpgmg_user_set_max_iterations(S, 40) == 0
        assert lib.hpgmg_user_solve(S, {"pcg": H.USER_PCG, "fpcg": H.USER_FPCG}[method], 1e-9, None, H.WHERE_PLUGIN, ctypes.byref(info)) == 0
        pu = D.empty(f.nbytes)
        assert lib.hpgmg_user_get_solution(S, pu, H.WHERE_PLUGIN) == 0
        return D.get(pu, f.shape), SolveInfo(info.norm_of_residual, info.norm_of_f, info.vcycles, bool(info.converged), info.mean_shift)


def _problem(n, bc, a, boundary, contrast):
    if contrast:
        bi, bj, bk, f = contrast_problem(n, contrast)
        return (None, bi, bj, bk), f, None
    coef = random_coefficients(n, "periodic" if bc == "periodic" else "dirichlet", a != 0.0, seed=800 + n + int(a))
    rng = np.random.default_rng(n + 5)
    f = rng.random((n, n, n)) - 0.3
    return coef, f, (rng.random((6, n, n)) * 2.0 - 1.0 if boundary else None)


def _same(got, ref):
    (u, info), (u_ref, ref_info) = got, ref
    assert ref_info.vcycles >= 2
    assert np.array_equal(u, u_ref)
    assert (info.vcycles, info.residual, info.norm_f, info.converged, info.mean_shift) == \
           (ref_info.vcycles, ref_info.residual, ref_info.norm_f, ref_info.converged, ref_info.mean_shift)


CASES = [  # n, box_dim, bc, smoother, a, boundary values, contrast, entry
    (48, 16, "periodic", "cheby", 1.3, False, 0, "host"),          # BiCGStab at the bottom: the case the method exists for
    (64, 32, SIDES, "gsrb", 0.0, True, 0, "device"),
    (24, 8, "dirichlet", "cheby", 0.0, False, 100.0, "host"),
    (64, 32, "periodic", "jacobi", 0.0, False, 0, "host"),         # singular: the mean handling
]


@pytest.mark.parametrize("n,box_dim,bc,smoother,a,boundary,contrast,entry", CASES)
def test_whole_fpcg_solves_equal_the_oracle(libs, n, box_dim, bc, smoother, a, boundary, contrast, entry):
    hip, oracle, K = libs
    coef, f, g = _problem(n, bc, a, boundary, contrast)
    ref = _solve(oracle, "fpcg", n, box_dim, bc, smoother, a, coef, f, g)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = _solve(hip, "fpcg", n, box_dim, bc, smoother, a, coef, f, g, device=D)
    finally:
        if D:
            D.free()
    _same(got, ref)


def test_pcg_still_equals_the_oracle(libs):
    """One case of tests/test_gpu_user_pcg.py on this build: method="pcg" goes through pcg_fold_kernel, which stands next to the new two-array fold."""
    hip, oracle, _ = libs
    n, box_dim, bc, smoother, a = 64, 32, "dirichlet", "cheby", 1.0
    coef = random_coefficients(n, "dirichlet", True, seed=700 + n + len(smoother) + int(a))
    rng = np.random.default_rng(n + 3)
    f = rng.random((n, n, n)) - 0.3
    g = rng.random((6, n, n)) * 2.0 - 1.0
    _same(_solve(hip, "pcg", n, box_dim, bc, smoother, a, coef, f, g), _solve(oracle, "pcg", n, box_dim, bc, smoother, a, coef, f, g))
