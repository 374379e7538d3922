"""method="fpcg" of the user-problem API (hpgmg_amd/problem.py) on the CPU oracle: flexible conjugate gradients around the V-cycle,
beta = -(Ap.z / p.Ap) from the one pass hpgmg_pcg_dot2.

Solves are checked against SciPy's direct solve of the independent assembly, as the "pcg" tests are; on the contrast problem at N = 32 against the
"pcg" file's gate (28 / 32 iterations plus 25 %; measured 30 / 33, the counts of "pcg"); and on the grids the method exists for -- a coarsest level
BiCGStab solves to a tolerance, which makes the V-cycle vary between iterations -- against the counts measured on this oracle plus 25 %, the
project's margin for a change of summation order (not of Krylov space):

    contrast 100, N = 24, box 8, rtol 1e-8:     fpcg 33 (cheby) / 49 (gsrb);  mg stalls at 7.1e-3 / 1.5e-2;  pcg is at 1.8e-8 / 2.8e-4 after 100
    periodic Helmholtz a = 1.3, rtol 1e-10:     fpcg 20 at (24, 8) and 16 at (32, 16);  pcg is at 9.1e-4 / 7.4e-3 after 100

hpgmg_pcg_dot2 is checked against hpgmg_pcg_dot and against the NumPy restatement of the summation order of include/hpgmg_operators.h (tests/pcg_lib.py).
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from pcg_lib import dense_boxes, header_order_dot
from user_neumann_lib import ALL, SIDES, assemble_faces, lift_faces
from user_pcg_lib import contrast_problem
from user_problem_lib import assemble, random_coefficients

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8
MGPCG_ITERATIONS = {"cheby": 28, "gsrb": 32}          # the "pcg" file's gate at N = 32, contrast 100, rtol 1e-8, before its 25 %
ODD_GRID_ITERATIONS = {"cheby": 33, "gsrb": 49}       # measured: contrast 100 at N = 24, box 8, rtol 1e-8
PERIODIC_ITERATIONS = {(24, 8): 20, (32, 16): 16}     # measured: periodic Helmholtz a = 1.3, rtol 1e-10


@pytest.fixture(scope="module")
def lib():
    return Backend.oracle().lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_fpcg_solve_matches_direct_solve(lib, n, box_dim, bc, a):
    alpha, bi, bj, bk = random_coefficients(n, bc, a != 0.0, seed=3 * n + (bc == "periodic") + int(10 * a))
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(5).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, bc=bc, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="fpcg", rtol=1e-10)
    assert info.converged and info.residual < 1e-10 * info.norm_f and info.vcycles >= 1
    A = assemble(n, bc, a, b, h, alpha, bi, bj, bk).tocsc()
    singular = bc == "periodic" and a == 0.0
    rhs = (f - f.mean() if singular else f).ravel().copy()
    if singular:           # pin one cell to make the direct solve regular, then compare without the mean
        A = A.tolil(); A[0, :] = 0.0; A[0, 0] = 1.0; A = A.tocsc()
        rhs[0] = 0.0
    ref = spl.spsolve(A, rhs).reshape(n, n, n)
    if singular:
        ref, u = ref - ref.mean(), u - u.mean()
        assert info.mean_shift != 0.0
    assert _rel(u, ref) <= 1e-8


def test_fpcg_on_mixed_walls(lib):
    n, a, b = 16, 0.0, 1.0
    h = 1.0 / n
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=21)
    rng = np.random.default_rng(9)
    f, g = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=8, bc=SIDES, a=a, b=b, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="fpcg", rtol=1e-10, boundary=g)
    assert info.converged
    F = f + lift_faces(n, SIDES, b, h, bi, bj, bk, g)
    ref = spl.spsolve(assemble_faces(n, SIDES, a, b, h, None, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8


def test_fpcg_on_six_neumann_walls_poisson(lib):
    n, b = 16, 1.0
    h = 1.0 / n
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=22)
    f = np.random.default_rng(10).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=8, bc="neumann", a=0.0, b=b, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="fpcg", rtol=1e-10)
    assert info.converged and info.mean_shift != 0.0
    A = assemble_faces(n, ALL, 0.0, b, h, None, bi, bj, bk).tolil()
    rhs = (f - f.mean()).ravel().copy()
    A[0, :] = 0.0; A[0, 0] = 1.0; rhs[0] = 0.0
    ref = spl.spsolve(A.tocsc(), rhs).reshape(n, n, n)
    assert _rel(u - u.mean(), ref - ref.mean()) <= 1e-8


@pytest.fixture(scope="module")
def contrast100():
    return contrast_problem(32, 100.0)


@pytest.mark.parametrize("smoother", ["cheby", "gsrb"])
def test_contrast_problem_fpcg_converges_in_the_pcg_gate(lib, contrast100, smoother):
    bi, bj, bk, f = contrast100
    with Solver(32, box_dim=16, smoother=smoother, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="fpcg", rtol=1e-8, max_iter=50)
        r = np.abs(s.apply(u) - f).max()
    print(f"contrast 100, N = 32, {smoother}: fpcg {info.vcycles} iterations rel {info.residual / info.norm_f:.3e}")
    assert info.converged and info.residual < 1e-8 * info.norm_f
    assert info.vcycles <= 1.25 * MGPCG_ITERATIONS[smoother]
    assert abs(r - info.residual) <= 1e-12 * r


@pytest.mark.parametrize("smoother", ["cheby", "gsrb"])
def test_contrast_on_a_grid_with_an_odd_factor_only_fpcg_converges(lib, smoother):
    """Contrast 100 at N = 24 in 3^3 boxes of 8, rtol 1e-8: jumps AND a coarsest level BiCGStab solves.  Measured on this oracle: fpcg 33 (cheby) /
    49 (gsrb) iterations; mg is at 7.1e-3 / 1.5e-2 after its 20 V-cycles; pcg at 1.8e-8 / 2.8e-4 after 100 iterations."""
    bi, bj, bk, f = contrast_problem(24, 100.0)
    with Solver(24, box_dim=8, smoother=smoother, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        _, mg = s.solve(f, method="mg", rtol=1e-8)
        u, info = s.solve(f, method="fpcg", rtol=1e-8, max_iter=100)
        r = np.abs(s.apply(u) - f).max()
        if smoother == "gsrb":
            _, pcg = s.solve(f, method="pcg", rtol=1e-8, max_iter=100)
    print(f"contrast 100, N = 24, {smoother}: mg rel {mg.residual / mg.norm_f:.3e}; fpcg {info.vcycles} iterations rel {info.residual / info.norm_f:.3e}")
    assert not mg.converged
    assert info.converged and info.residual < 1e-8 * info.norm_f and info.vcycles < 100
    assert info.vcycles <= 1.25 * ODD_GRID_ITERATIONS[smoother]
    assert abs(r - info.residual) <= 1e-12 * r
    if smoother == "gsrb":             # (cheby: pcg ends at 1.8e-8, too close to the tolerance to pin either way)
        print(f"    pcg {pcg.vcycles} iterations rel {pcg.residual / pcg.norm_f:.3e}")
        assert not pcg.converged and pcg.vcycles == 100


@pytest.mark.parametrize("n,box_dim", sorted(PERIODIC_ITERATIONS))
def test_periodic_helmholtz_pcg_fails_fpcg_converges(lib, n, box_dim):
    """Periodic boxes: BiCGStab at the bottom, a V-cycle that varies.  Measured on this oracle at rtol 1e-10: fpcg 20 iterations at (24, 8) and 16 at
    (32, 16) (mg: 9 and 10 V-cycles); pcg is at 9.1e-4 and 7.4e-3 after 100."""
    a = 1.3
    coef = random_coefficients(n, "periodic", True, seed=7)
    f = np.random.default_rng(5).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, bc="periodic", a=a, b=1.0, lib=lib) as s:
        s.set_coefficients(*coef)
        _, pcg = s.solve(f, method="pcg", rtol=1e-10, max_iter=100)
        _, info = s.solve(f, method="fpcg", rtol=1e-10, max_iter=100)
    print(f"periodic Helmholtz N = {n}: pcg {pcg.vcycles} iterations rel {pcg.residual / pcg.norm_f:.3e}; fpcg {info.vcycles} rel {info.residual / info.norm_f:.3e}")
    assert not pcg.converged
    assert info.converged and info.residual < 1e-10 * info.norm_f
    assert info.vcycles <= 1.25 * PERIODIC_ITERATIONS[(n, box_dim)]


@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_dot2_equals_two_dots_and_the_headers_order(lib, n, box_dim):
    rng = np.random.default_rng(40 + n)
    va, vc, vb = (rng.random((n, n, n)) * 2.0 - 1.0 for _ in range(3))
    with Solver(n, box_dim=box_dim, lib=lib) as s:
        s.solve(np.ones((n, n, n)), method="fpcg", max_iter=1)           # grows the levels by the three vectors of the method
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0)
        p_id = lib.hpgmg_vectors_reserved()
        a_id, c_id, b_id = H.VECTOR_R, p_id + 1, p_id + 2
        for vid, v in ((a_id, va), (c_id, vc), (b_id, vb)):
            assert lib.hpgmg_dense_pack(L, vid, v.ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0
        ab, cb, one = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        assert lib.hpgmg_pcg_dot2(L, a_id, c_id, b_id, ctypes.byref(ab), ctypes.byref(cb)) == 0       # the portable form
        lib.hpgmg_pcg_dot(L, a_id, b_id, ctypes.byref(one))
        assert ab.value == one.value
        lib.hpgmg_pcg_dot(L, c_id, b_id, ctypes.byref(one))
        assert cb.value == one.value
    A, C, B = (dense_boxes(v, box_dim) for v in (va, vc, vb))
    assert ab.value == header_order_dot(A, B, box_dim) and cb.value == header_order_dot(C, B, box_dim)
    assert ab.value != 0.0 and cb.value != 0.0 and ab.value != cb.value
    assert abs(ab.value - float((va * vb).sum())) <= 1e-12 * n ** 3


def test_max_iter_ends_the_solve_without_raising(lib, contrast100):
    bi, bj, bk, f = contrast100
    with Solver(32, box_dim=16, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="fpcg", rtol=1e-8, max_iter=3)
        r = np.abs(s.apply(u) - f).max()
    assert not info.converged and info.vcycles == 3
    assert np.isfinite(u).all()
    assert abs(info.residual - r) <= 1e-12 * r


def test_fpcg_from_a_converged_u0(lib, contrast100):
    bi, bj, bk, f = contrast100
    rtol = 1e-8
    with Solver(32, box_dim=16, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        cold, first = s.solve(f, method="fpcg", rtol=rtol)
        warm, again = s.solve(f, method="fpcg", rtol=rtol, u0=cold.copy())
    assert first.converged and again.converged
    assert again.vcycles <= 1
    assert _rel(warm, cold) <= rtol


def test_refusals_name_the_argument(lib):
    f = np.zeros((16, 16, 16))
    with Solver(16, box_dim=8, lib=lib) as s:
        for bad in (0, 2.5, -1, True, None):
            with pytest.raises(ValueError, match="max_iter"):
                s.solve(f, method="fpcg", max_iter=bad)
        with pytest.raises(ValueError, match="method"):
            s.solve(f, method="cg")
        assert lib.hpgmg_user_solve(s._ptr, 4, 1e-8, None, H.WHERE_HOST, ctypes.byref(H.UserInfo())) == H.USER_BAD_ARGUMENT
