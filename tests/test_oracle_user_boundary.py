"""Inhomogeneous Dirichlet values of the user-problem API (Solver(..., boundary=), hpgmg_user_set_rhs_dirichlet / hpgmg_user_apply_dirichlet)
on the CPU oracle.

apply(x, boundary=g) is checked against a SciPy assembly of A0 x - T(g), V-cycle solves against spsolve(A0, f + T), an all-zero g against the
homogeneous API bit for bit, and the boundary F-cycle against a manufactured solution: one F-cycle is as accurate as V-cycles to 1e-12
(the FMG property), which the same F-cycle on f + T without the per-level corrections is far from.
"""
import ctypes

import numpy as np
import pytest
import scipy.sparse.linalg as spl

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_boundary_lib import exact, lift, manufactured
from user_problem_lib import assemble, random_coefficients

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8
# measured on this oracle: one F-cycle's max error / the V-cycle solution's is 0.89, 0.92, 0.95 at N = 16, 32, 64 (0.97 at 256 on the GPU)
FMG_FACTOR = 1.5
# the F-cycle on f + T(g) without the level corrections: 100x at N = 16, 500x at 32, 2200x at 64
UNCORRECTED_FACTOR = 50.0


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _rel(x, ref):
    return np.abs(x - ref).max() / np.abs(ref).max()


def _random_boundary(n, seed):
    return np.random.default_rng(seed).random((6, n, n)) * 4.0 - 2.0


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_apply_matches_scipy_assembly(lib, n, box_dim, a):
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=100 + n + int(10 * a))
    b, h = 0.7, 1.0 / n
    x = np.random.default_rng(12).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 13)
    with Solver(n, box_dim=box_dim, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        y = s.apply(x, boundary=g)
        y0 = s.apply(x)
    A0 = assemble(n, "dirichlet", a, b, h, alpha, bi, bj, bk)
    ref = (A0 @ x.ravel()).reshape(n, n, n) - lift(n, b, h, bi, bj, bk, g)
    assert _rel(y, ref) <= 1e-13
    assert not np.array_equal(y, y0)


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
def test_mg_solve_matches_direct_solve(lib, n, box_dim, a):
    alpha, bi, bj, bk = random_coefficients(n, "dirichlet", a != 0.0, seed=200 + n + int(10 * a))
    b, h = 1.0, 1.0 / n
    f = np.random.default_rng(7).random((n, n, n)) * 2.0 - 1.0
    g = _random_boundary(n, 8)
    with Solver(n, box_dim=box_dim, a=a, b=b, lib=lib) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
        r = s.apply(u, boundary=g) - f                       # the true residual of the boundary-value problem
    assert info.converged
    F = f + lift(n, b, h, bi, bj, bk, g)
    assert info.norm_f == pytest.approx(np.abs(F).max(), rel=1e-14)
    ref = spl.spsolve(assemble(n, "dirichlet", a, b, h, alpha, bi, bj, bk).tocsc(), F.ravel()).reshape(n, n, n)
    assert _rel(u, ref) <= 1e-8
    assert np.abs(r).max() <= 1e-10 * np.abs(F).max()


@pytest.mark.parametrize("smoother", ["cheby", "gsrb", "jacobi"])
@pytest.mark.parametrize("a", [0.0, 1.0])
def test_zero_boundary_values_are_the_homogeneous_problem(lib, smoother, a):
    n = 16
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=300 + len(smoother))
    f = np.random.default_rng(9).random((n, n, n)) - 0.4
    zero = np.zeros((6, n, n))
    with Solver(n, box_dim=8, smoother=smoother, a=a, lib=lib) as s:
        s.set_coefficients(*coef)
        for method in ("fmg", "mg"):
            u0, i0 = s.solve(f, method=method)
            u1, i1 = s.solve(f, method=method, boundary=zero)
            assert np.array_equal(u0, u1), method
            assert (i0.residual, i0.vcycles, i0.norm_f) == (i1.residual, i1.vcycles, i1.norm_f)
        assert np.array_equal(s.apply(f), s.apply(f, boundary=zero))


@pytest.mark.parametrize("a", [0.0, 1.0])
def test_manufactured_solution(lib, a):
    """Second order under V-cycles; one F-cycle within FMG_FACTOR of that at every N; without the level corrections far outside it."""
    errs_mg = []
    for n in (16, 32, 64):
        alpha, bi, bj, bk, f, u_star = manufactured(n, a, 1.0)
        with Solver(n, box_dim=min(n // 2, 32), a=a, b=1.0, lib=lib) as s:
            s.set_coefficients(alpha, bi, bj, bk)
            g = s.boundary_from(exact)
            assert np.all(np.abs(g) > 0.05)                   # non-zero on every face
            u_mg, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
            u_fmg, info_f = s.solve(f, method="fmg", boundary=g)
            F = f - s.apply(np.zeros_like(f), boundary=g)     # f + T(g), handed to the homogeneous API: the F-cycle with no corrections
            u_plain, _ = s.solve(F, method="fmg")
        assert info.converged and info_f.vcycles == 1
        e_mg, e_fmg, e_plain = (np.abs(u - u_star).max() for u in (u_mg, u_fmg, u_plain))
        assert e_fmg <= FMG_FACTOR * e_mg, (n, e_fmg, e_mg)
        assert e_plain >= UNCORRECTED_FACTOR * e_mg, (n, e_plain, e_mg)
        errs_mg.append(e_mg)
    assert errs_mg[0] / errs_mg[1] >= 3.5 and errs_mg[1] / errs_mg[2] >= 3.5, errs_mg


def test_boundary_from_layout(lib):
    n = 8
    with Solver(n, box_dim=4, h=0.5, lib=lib) as s:
        g = s.boundary_from(lambda x, y, z: x + 10.0 * y + 100.0 * z)
    c = (np.arange(n) + 0.5) * 0.5
    w = n * 0.5
    assert np.array_equal(g[0], 10.0 * c[None, :] + 100.0 * c[:, None])          # i-low, [k][j]
    assert np.array_equal(g[1], w + 10.0 * c[None, :] + 100.0 * c[:, None])
    assert np.array_equal(g[3], c[None, :] + 10.0 * w + 100.0 * c[:, None])      # j-high, [k][i]
    assert np.array_equal(g[4], c[None, :] + 10.0 * c[:, None])                  # k-low, [j][i]


def test_refusals(lib):
    n = 16
    coef = random_coefficients(n, "dirichlet", False, seed=400)
    f = np.ones((n, n, n))
    g = _random_boundary(n, 14)
    with Solver(n, box_dim=8, bc="periodic", lib=lib) as s:
        with pytest.raises(ValueError, match="^boundary:.*Dirichlet"):
            s.solve(f, boundary=g)
        with pytest.raises(ValueError, match="^boundary:.*Dirichlet"):
            s.apply(f, boundary=g)
        shift = ctypes.c_double()
        assert lib.hpgmg_user_set_rhs_dirichlet(s._ptr, f.ctypes.data, g.ctypes.data, H.WHERE_HOST, ctypes.byref(shift)) == H.USER_UNSUPPORTED
    with Solver(n, box_dim=8, lib=lib) as s:
        s.set_coefficients(None, *coef[1:])
        bad = g.copy(); bad[5, 15, 15] = np.nan                # the last entry of the k-high face
        with pytest.raises(ValueError, match="^boundary:.*not finite"):
            s.solve(f, boundary=bad)
        with pytest.raises(ValueError, match="^boundary:.*not finite"):
            s.apply(f, boundary=bad)
        with pytest.raises(ValueError, match="^boundary: shape"):
            s.solve(f, boundary=np.zeros((6, n, n + 1)))
        with pytest.raises(ValueError, match="^boundary: dtype"):
            s.apply(f, boundary=np.zeros((6, n, n), dtype=np.float32))
        bad_f = f.copy(); bad_f[0, 0, 0] = np.inf
        with pytest.raises(ValueError, match="^f:"):
            s.solve(bad_f, boundary=g)
        u, _ = s.solve(f, boundary=g)                            # still usable
        assert np.isfinite(u).all()
        # new coefficients after a boundary rhs: the lift was made with the old beta, the next solve is refused until a new rhs
        S, info = s._ptr, H.UserInfo()
        shift = ctypes.c_double()
        assert lib.hpgmg_user_set_rhs_dirichlet(S, f.ctypes.data, g.ctypes.data, H.WHERE_HOST, ctypes.byref(shift)) == H.USER_OK
        s.set_coefficients(None, *coef[1:])
        assert lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_NOT_READY
        assert lib.hpgmg_user_set_rhs_dirichlet(S, f.ctypes.data, g.ctypes.data, H.WHERE_HOST, ctypes.byref(shift)) == H.USER_OK
        assert lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_OK
        s.set_coefficients(None, *coef[1:])
        assert lib.hpgmg_user_set_rhs(S, f.ctypes.data, H.WHERE_HOST, ctypes.byref(shift)) == H.USER_OK   # a plain rhs clears the values
        assert lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_OK
