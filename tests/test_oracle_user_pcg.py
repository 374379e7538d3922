"""method="pcg" of the user-problem API (hpgmg_amd/problem.py) on the CPU oracle: conjugate gradients around the V-cycle.

Solves are checked against SciPy's direct solve of the independent assembly (user_problem_lib / user_neumann_lib), as the "mg" tests are, and on
the contrast problem (user_pcg_lib), where V-cycles alone stall, against an iteration gate: 28 (Chebyshev) and 32 (GSRB) iterations to 1e-8 at N = 32,
contrast 100, plus 25 % -- the summation order of the passes changes the rounding, not the Krylov space.  Measured: 30 / 33, which is also what the
reference-faithful MGPCG loop takes with its limit of 20 raised.
"""
import numpy as np
import pytest
import scipy.sparse.linalg as spl

from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_boundary_lib import lift
from user_neumann_lib import ALL, SIDES, assemble_faces, lift_faces
from user_pcg_lib import contrast_problem
from user_problem_lib import assemble, random_coefficients

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8
MGPCG_ITERATIONS = {"cheby": 28, "gsrb": 32}      # the gate on the contrast problem (N = 32, contrast 100, rtol 1e-8), before its 25 %


@pytest.fixture(scope="module")
def lib():
    return Backend.oracle().lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("bc", ["dirichlet", "periodic"])
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_pcg_solve_matches_direct_solve(lib, n, box_dim, bc, a):
    alpha, bi, bj, bk = random_coefficients(n, bc, a != 0.0, seed=3 * n + (bc == "periodic") + int(10 * a))
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(5).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, bc=bc, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="pcg", rtol=1e-10)
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


@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_pcg_with_boundary_values_solves_the_lifted_system(lib, n, box_dim):
    a, b, h = 1.3, 1.0, 1.0 / n
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", True, seed=n + 1)
    rng = np.random.default_rng(8)
    f, g = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=box_dim, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="pcg", rtol=1e-10, boundary=g)
    assert info.converged
    F = f + lift(n, b, h, bi, bj, bk, g)
    ref = spl.spsolve(assemble(n, "dirichlet", a, b, h, alpha, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8
    assert abs(info.norm_f - np.abs(F).max()) <= 1e-12 * np.abs(F).max()


def test_pcg_on_mixed_walls(lib):
    n, a, b = 16, 0.0, 1.0
    h = 1.0 / n
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=21)
    rng = np.random.default_rng(9)
    f, g = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=8, bc=SIDES, a=a, b=b, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="pcg", rtol=1e-10, boundary=g)
    assert info.converged
    F = f + lift_faces(n, SIDES, b, h, bi, bj, bk, g)
    ref = spl.spsolve(assemble_faces(n, SIDES, a, b, h, None, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8


def test_pcg_on_six_neumann_walls_poisson(lib):
    n, b = 16, 1.0
    h = 1.0 / n
    _, bi, bj, bk = random_coefficients(n, "dirichlet", False, seed=22)
    f = np.random.default_rng(10).random((n, n, n)) * 2.0 - 1.0
    with Solver(n, box_dim=8, bc="neumann", a=0.0, b=b, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="pcg", rtol=1e-10)
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
def test_contrast_problem_mg_stalls_pcg_converges(lib, contrast100, smoother):
    bi, bj, bk, f = contrast100
    with Solver(32, box_dim=16, smoother=smoother, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        _, mg = s.solve(f, method="mg", rtol=1e-8)
        u, pcg = s.solve(f, method="pcg", rtol=1e-8, max_iter=50)
        r = np.abs(s.apply(u) - f).max()
    print(f"contrast 100, {smoother}: mg {mg.vcycles} V-cycles rel {mg.residual / mg.norm_f:.3e}; pcg {pcg.vcycles} iterations rel {pcg.residual / pcg.norm_f:.3e}")
    assert not mg.converged
    assert pcg.converged and pcg.residual < 1e-8 * pcg.norm_f
    assert pcg.vcycles <= 1.25 * MGPCG_ITERATIONS[smoother]
    assert abs(r - pcg.residual) <= 1e-12 * r


@pytest.mark.parametrize("smoother", ["cheby", "gsrb"])
def test_contrast_one_pcg_needs_no_more_than_mg(lib, smoother):
    bi, bj, bk, f = contrast_problem(32, 1.0)
    with Solver(32, box_dim=16, smoother=smoother, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        _, mg = s.solve(f, method="mg", rtol=1e-8)
        _, pcg = s.solve(f, method="pcg", rtol=1e-8)
    assert mg.converged and pcg.converged
    assert pcg.vcycles <= mg.vcycles + 1


def test_max_iter_ends_the_solve_without_raising(lib, contrast100):
    bi, bj, bk, f = contrast100
    with Solver(32, box_dim=16, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        u, info = s.solve(f, method="pcg", rtol=1e-8, max_iter=3)
        r = np.abs(s.apply(u) - f).max()
    assert not info.converged and info.vcycles == 3
    assert np.isfinite(u).all()
    assert abs(info.residual - r) <= 1e-12 * r


def test_pcg_from_a_converged_u0(lib, contrast100):
    bi, bj, bk, f = contrast100
    rtol = 1e-8
    with Solver(32, box_dim=16, lib=lib) as s:
        s.set_coefficients(None, bi, bj, bk)
        cold, first = s.solve(f, method="pcg", rtol=rtol)
        warm, again = s.solve(f, method="pcg", rtol=rtol, u0=cold.copy())
    assert first.converged and again.converged
    assert again.vcycles <= 1
    assert _rel(warm, cold) <= rtol


def test_refusals_name_the_argument(lib):
    f = np.zeros((16, 16, 16))
    with Solver(16, box_dim=8, lib=lib) as s:
        for bad in (0, 2.5, -1, True, None):
            with pytest.raises(ValueError, match="max_iter"):
                s.solve(f, method="pcg", max_iter=bad)
        with pytest.raises(ValueError, match="method"):
            s.solve(f, method="cg")
        s.solve(f, method="mg", max_iter=0)          # read by "pcg" only
        assert lib.hpgmg_user_set_max_iterations(s._ptr, 0) != 0
