"""Face fluxes of a solution (Solver.flux, Solver.wall_flux, hpgmg_user_flux, hpgmg_dense_unpack_flux) on the CPU oracle.  DESIGN.md §11.6.

flux() is checked against an independent NumPy evaluation from ghost-padded u (user_flux_lib.reference) within the rounding bound derived
there; a alpha u + div_h(flux) against apply(u, boundary=g), the identity that defines the fluxes; the wall fluxes of a solution against the
volume integral of f - a alpha u; a linear u against its exact flux on every kind of wall; and pairs of calls that must give the same bytes.
"""
import ctypes
import math

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_boundary_lib import _beta, exact, manufactured
from user_flux_lib import EPS, SOLVERS, boundary_for, divergence, faces_of, identity_bound, kappa_for, reference
from user_neumann_lib import grad_exact
from user_problem_lib import face_shape, random_coefficients
from user_robin_lib import ALL, CORNERS, SIDES, kappa_of, neumann_of

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8: boxes on zero to three walls, box-to-box and periodic-wrap faces
NAMES = ["dirichlet", "periodic", "corners", "robin", "neumann"]
# Accuracy gates (test_fluxes_converge_to_the_exact_flux): 0.8 times the smallest error ratio per doubling of N measured on the oracle, over
# the Dirichlet, `sides` and all-Robin solvers and N = 16 -> 32 -> 64.  Measured: the table of DESIGN.md §11.6 and the test's docstring.
INTERIOR_RATIO_GATE = 0.8 * 2.01
WALL_RATIO_GATE = 0.8 * 2.00


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _bc_name(name):
    return "periodic" if name == "periodic" else "dirichlet"


def _problem(name, n, a, seed):
    bc = _bc_name(name)
    coef = random_coefficients(n, bc, a != 0.0, seed=seed)
    u = np.random.default_rng(seed + 1).random((n, n, n)) * 2.0 - 1.0
    return bc, coef, u, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _solver(lib, name, n, box_dim, a, b, coef, kappa):
    s = Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=b, lib=lib)
    s.set_coefficients(*coef, robin=kappa)
    return s


# ---------------------------------------------------------------- 1. against the NumPy evaluation, 2. the identity
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_flux_matches_the_numpy_evaluation(lib, name, n, box_dim):
    b, h = 0.7, 1.0 / n
    bc, coef, u, g, kappa = _problem(name, n, 0.0, 600 + n)
    with _solver(lib, name, n, box_dim, 0.0, b, coef, kappa) as s:
        got = s.flux(u, boundary=g)
    ref = reference(n, bc, faces_of(name), b, h, coef[1:], u, g, kappa)
    for axis, (q, (q_ref, bound)) in enumerate(zip(got, ref)):
        assert q.shape == face_shape(n, bc, axis) and q.dtype == np.float64
        excess = np.abs(q - q_ref) - bound
        print(f"{name} N={n} axis {axis}: max |q - ref| / bound = {(np.abs(q - q_ref) / bound).max():.3f}")
        assert (excess <= 0.0).all(), (axis, np.unravel_index(excess.argmax(), excess.shape), excess.max())


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
@pytest.mark.parametrize("name", NAMES)
def test_divergence_of_the_flux_is_the_operator(lib, name, n, box_dim, a):
    """a alpha u + div_h(flux(u, g)) = apply(u, boundary=g), Poisson and Helmholtz."""
    b, h = 0.7, 1.0 / n
    bc, coef, u, g, kappa = _problem(name, n, a, 700 + n + int(10 * a))
    with _solver(lib, name, n, box_dim, a, b, coef, kappa) as s:
        q = s.flux(u, boundary=g)
        y = s.apply(u, boundary=g)
    lhs = divergence(n, bc, h, q)
    if a != 0.0:
        lhs = lhs + a * coef[0] * u
    bound = identity_bound(n, bc, a, h, coef[0], u, [bnd for _, bnd in reference(n, bc, faces_of(name), b, h, coef[1:], u, g, kappa)])
    print(f"{name} N={n} a={a}: max |a alpha u + div q - A u| / bound = {(np.abs(lhs - y) / bound).max():.3f}")
    assert (np.abs(lhs - y) <= bound).all()


# ---------------------------------------------------------------- 3. global balance
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, 1.3])
@pytest.mark.parametrize("name", ["dirichlet", "corners", "robin", "neumann"])
def test_what_leaves_through_the_walls_is_what_the_sources_supply(lib, name, n, box_dim, a):
    """h^2 sum(wall_flux) = h^3 sum(f - a alpha u) for a solution, to within the residual over the volume plus the identity's rounding bound."""
    b, h = 1.0, 1.0 / n
    bc, coef, _, g, kappa = _problem(name, n, a, 800 + n + int(10 * a))
    f = np.random.default_rng(81).random((n, n, n)) * 2.0 - 1.0
    with _solver(lib, name, n, box_dim, a, b, coef, kappa) as s:
        u, info = s.solve(f, method="mg", rtol=1e-10, boundary=g)
        q = s.flux(u, boundary=g)
        out = s.wall_flux(q)
    assert info.converged and info.mean_shift == 0.0 and out.shape == (6, n, n)
    terms = [f.ravel()] + ([-(a * coef[0] * u).ravel()] if a != 0.0 else [])
    supplied = h ** 3 * math.fsum(np.concatenate(terms))
    leaving = h ** 2 * math.fsum(out.ravel())
    rounding = identity_bound(n, bc, a, h, coef[0], u, [bnd for _, bnd in reference(n, bc, faces_of(name), b, h, coef[1:], u, g, kappa)])
    bound = info.residual * (n * h) ** 3 + h ** 3 * math.fsum(rounding.ravel())
    print(f"{name} N={n} a={a}: leaving {leaving:.15e}, supplied {supplied:.15e}, difference {abs(leaving - supplied):.3e}, bound {bound:.3e}")
    assert abs(leaving - supplied) <= bound


# ---------------------------------------------------------------- 4. exactness for linear u
SLOPE = (1.1, -0.7, 0.5)


def _linear(x, y, z):
    return 0.3 + SLOPE[0] * x + SLOPE[1] * y + SLOPE[2] * z


def _linear_grad(x, y, z):
    return SLOPE[0] + 0.0 * x, SLOPE[1] + 0.0 * x, SLOPE[2] + 0.0 * x


@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("name", ["dirichlet", "corners", "robin", "neumann"])
def test_linear_u_has_its_exact_flux_on_every_wall(lib, name, n, box_dim):
    b, beta, h = 0.7, 1.9, 1.0 / n
    c = (np.arange(n) + 0.5) * h
    Z, Y, X = np.meshgrid(c, c, c, indexing="ij")
    u = np.ascontiguousarray(_linear(X, Y, Z))
    coef = [None] + [np.full(face_shape(n, "dirichlet", axis), beta) for axis in range(3)]
    kappa = kappa_for(name, n)
    with _solver(lib, name, n, box_dim, 0.0, b, coef, kappa) as s:
        g = s.boundary_from(_linear, grad=_linear_grad if faces_of(name) else None, robin=kappa)
        q = s.flux(u, boundary=g)
    for axis in range(3):
        err = np.abs(q[axis] - (-b * beta * SLOPE[axis])).max()
        print(f"{name} N={n} axis {axis}: max error {err:.3e}")
        assert err <= 1e-12 * abs(SLOPE[axis]) * b * beta


# ---------------------------------------------------------------- 5. bytes
def _bytes(q):
    return [x.tobytes() for x in q]


def test_six_dirichlet_faces_are_the_dirichlet_solver(lib):
    n = 16
    bc, coef, u, g, _ = _problem("dirichlet", n, 1.3, 910)
    with Solver(n, box_dim=8, bc="dirichlet", a=1.3, lib=lib) as s, Solver(n, box_dim=8, bc=("dirichlet",) * 6, a=1.3, lib=lib) as t:
        s.set_coefficients(*coef)
        t.set_coefficients(*coef)
        assert _bytes(s.flux(u, boundary=g)) == _bytes(t.flux(u, boundary=g))


@pytest.mark.parametrize("name", ["dirichlet", "corners", "robin", "neumann"])
def test_no_boundary_is_zero_data(lib, name):
    n = 16
    _, coef, u, g, kappa = _problem(name, n, 0.0, 920)
    with _solver(lib, name, n, 8, 0.0, 1.0, coef, kappa) as s:
        none = s.flux(u)
        assert _bytes(none) == _bytes(s.flux(u, boundary=np.zeros((6, n, n))))
        assert _bytes(none) != _bytes(s.flux(u, boundary=g))


@pytest.mark.parametrize("walls", [CORNERS, ALL, SIDES])
def test_kappa_zero_is_the_neumann_wall(lib, walls):
    n = 16
    coef = random_coefficients(n, "dirichlet", False, seed=930)
    rng = np.random.default_rng(93)
    u, g = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 4.0 - 2.0
    with Solver(n, box_dim=8, bc=neumann_of(walls), lib=lib) as s, Solver(n, box_dim=8, bc=walls, lib=lib) as t:
        s.set_coefficients(*coef)
        t.set_coefficients(*coef, robin=np.zeros((6, n, n)))
        assert _bytes(s.flux(u, boundary=g)) == _bytes(t.flux(u, boundary=g))
        assert _bytes(s.flux(u)) == _bytes(t.flux(u))


# ---------------------------------------------------------------- 6. no side effects
@pytest.mark.parametrize("name", ["dirichlet", "periodic", "corners"])
def test_flux_leaves_the_solver_as_it_was(lib, name):
    n = 16
    bc, coef, x, g, kappa = _problem(name, n, 1.3, 940)
    f = np.random.default_rng(94).random((n, n, n)) - 0.5
    with _solver(lib, name, n, 8, 1.3, 1.0, coef, kappa) as s:
        u, _ = s.solve(f, boundary=g)
        again, _ = s.solve(f, method="mg", boundary=g)          # what a second solve gives without a flux call in between
        u, _ = s.solve(f, boundary=g)
        s.flux(x, boundary=None if g is None else -g)           # another operand, other data
        assert s.get_solution().tobytes() == u.tobytes()
        info = H.UserInfo()                                     # the right-hand side of the last set_rhs is still in place
        assert lib.hpgmg_user_solve(s._ptr, H.USER_MG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_OK
        assert s.get_solution().tobytes() == again.tobytes()


# ---------------------------------------------------------------- 7. refusals
def test_refusals(lib):
    n = 16
    _, coef, u, g, _ = _problem("dirichlet", n, 0.0, 950)
    with Solver(n, box_dim=8, lib=lib) as s:
        s.set_coefficients(*coef)
        bad = u.copy()
        bad[3, 4, 5] = np.nan
        with pytest.raises(ValueError, match="^u:.*not finite"):
            s.flux(bad, boundary=g)
        with pytest.raises(ValueError, match="^u:.*not finite"):
            s.flux(bad)
        for face in range(6):
            bad_g = g.copy()
            bad_g[face, n - 1, 0] = np.inf
            with pytest.raises(ValueError, match="^boundary:.*not finite"):
                s.flux(u, boundary=bad_g)
        with pytest.raises(ValueError, match="^u: shape"):
            s.flux(u[:-1])
        with pytest.raises(ValueError, match="^boundary: shape"):
            s.flux(u, boundary=g[:5])
        good = s.flux(u, boundary=g)
        with pytest.raises(ValueError, match="^out"):
            s.flux(u, out=good[:2])
        with pytest.raises(ValueError, match="^out"):
            s.flux(u, out=good[0])
        with pytest.raises(ValueError, match=r"^out\[1\]: shape"):
            s.flux(u, out=(good[0], good[2], good[2]))
        with pytest.raises(ValueError, match=r"^out\[2\]: dtype"):
            s.flux(u, out=(good[0], good[1], good[2].astype(np.float32)))
        with pytest.raises(ValueError, match=r"^out\[0\]: expected"):
            s.flux(u, out=(good[0].tolist(), good[1], good[2]))
        with pytest.raises(ValueError, match=r"^out\[0\]:.*not C-contiguous"):
            s.flux(u, out=(np.empty((n + 1, n, n)).T, good[1], good[2]))
        into = tuple(np.full_like(q, 7.0) for q in good)
        assert s.flux(u, boundary=g, out=into) is not None and _bytes(into) == _bytes(good)
        with pytest.raises(ValueError, match="^fluxes"):
            s.wall_flux(good[:2])
        with pytest.raises(ValueError, match=r"^fluxes\[0\]: shape"):
            s.wall_flux((good[2], good[1], good[0]))
        low = coef[1].copy()
        low[2, 2, 2] = -1.0
        with pytest.raises(ValueError, match="^beta_i"):
            s.set_coefficients(None, low, coef[2], coef[3])
        with pytest.raises(ValueError, match="^u.*earlier call was refused"):
            s.flux(u, boundary=g)
        assert lib.hpgmg_user_flux(s._ptr, u.ctypes.data, None, *[q.ctypes.data for q in into], H.WHERE_HOST) == H.USER_NOT_READY
        s.set_coefficients(*coef)
        assert _bytes(s.flux(u, boundary=g)) == _bytes(good)
        p = [q.ctypes.data for q in into]
        assert lib.hpgmg_user_flux(s._ptr, None, None, *p, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_flux(s._ptr, u.ctypes.data, None, p[0], None, p[2], H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_flux(s._ptr, u.ctypes.data, None, *p, 2) == H.USER_BAD_ARGUMENT
    _, coef, u, _, _ = _problem("periodic", n, 0.0, 951)
    with Solver(n, box_dim=8, bc="periodic", lib=lib) as s:
        s.set_coefficients(*coef)
        q = s.flux(u)
        with pytest.raises(ValueError, match="^boundary:.*Dirichlet"):
            s.flux(u, boundary=g)
        with pytest.raises(ValueError, match="^fluxes:.*periodic"):
            s.wall_flux(q)
        assert lib.hpgmg_user_flux(s._ptr, u.ctypes.data, g.ctypes.data, *[x.ctypes.data for x in q], H.WHERE_HOST) == H.USER_UNSUPPORTED


def test_wall_flux_is_slicing_with_a_sign(lib):
    n = 16
    _, coef, u, g, _ = _problem("dirichlet", n, 0.0, 960)
    with Solver(n, box_dim=8, lib=lib) as s:
        s.set_coefficients(*coef)
        qi, qj, qk = s.flux(u, boundary=g)
        w = s.wall_flux((qi, qj, qk))
    assert w.flags.c_contiguous and w.shape == (6, n, n)
    for got, ref in zip(w, (-qi[:, :, 0], qi[:, :, n], -qj[:, 0, :], qj[:, n, :], -qk[0], qk[n])):
        assert np.array_equal(got, ref)


# ---------------------------------------------------------------- 8. accuracy
_ACCURACY = {}


def _flux_errors(lib, walls, n):
    """(max error of the interior fluxes, of the wall fluxes) against -b beta du*/dx_d at the face centres, V-cycles to 1e-12."""
    key = (walls, n)
    if key not in _ACCURACY:
        faces = {"dirichlet": "dirichlet", "sides": SIDES, "robin": ALL}[walls]
        a, b, h = 1.0, 1.0, 1.0 / n
        alpha, bi, bj, bk, f, _ = manufactured(n, a, b)
        kappa = kappa_of(n, faces) if walls != "dirichlet" else None
        with Solver(n, box_dim=min(n // 2, 32), bc=faces, a=a, b=b, lib=lib) as s:
            s.set_coefficients(alpha, bi, bj, bk, robin=kappa)
            g = s.boundary_from(exact, grad=grad_exact if walls != "dirichlet" else None, robin=kappa)
            u, info = s.solve(f, method="mg", rtol=1e-12, boundary=g)
            assert info.converged
            q = s.flux(u, boundary=g)
        c, fc = (np.arange(n) + 0.5) * h, np.arange(n + 1) * h
        interior = wall = 0.0
        for axis in range(3):
            zs, ys, xs = [fc if 2 - axis == ax else c for ax in range(3)]
            Z, Y, X = np.meshgrid(zs, ys, xs, indexing="ij")
            err = np.moveaxis(np.abs(q[axis] - (-b * _beta(X, Y, Z) * grad_exact(X, Y, Z)[axis])), 2 - axis, 0)
            interior = max(interior, err[1:-1].max())
            wall = max(wall, err[0].max(), err[-1].max())
        _ACCURACY[key] = (interior, wall)
    return _ACCURACY[key]


@pytest.mark.parametrize("walls", ["dirichlet", "sides", "robin"])
def test_fluxes_converge_to_the_exact_flux(lib, walls):
    """Measured on the oracle (manufactured u*, beta, alpha of §11.1, a = b = 1, V-cycles to rtol 1e-12), max error and its ratio per doubling:

        walls      N    interior   ratio   wall       ratio
        dirichlet  16   7.424e-03          2.777e-02
        dirichlet  32   3.697e-03  2.01    1.386e-02  2.00
        dirichlet  64   1.829e-03  2.02    6.919e-03  2.00
        sides      16   2.370e-03          3.882e-03
        sides      32   8.359e-04  2.84    1.226e-03  3.17
        sides      64   2.734e-04  3.06    3.725e-04  3.29
        robin      16   1.113e-03          1.701e-03
        robin      32   3.434e-04  3.24    4.436e-04  3.83
        robin      64   9.714e-05  3.54    1.133e-04  3.92

    Between Dirichlet walls the fluxes are first order, in the wall faces and in the inner faces next to them: the p1 ghost 2 g - u leaves u second
    order but with an error that is not smooth across the cells on the wall, and a difference over h or h / 2 loses one order there.  Neumann and
    Robin walls prescribe the flux itself and approach second order.  The gates are 0.8 times the smallest ratio of each column (2.01, 2.00)."""
    errs = [_flux_errors(lib, walls, n) for n in (16, 32, 64)]
    for kind, gate in ((0, INTERIOR_RATIO_GATE), (1, WALL_RATIO_GATE)):
        ratios = [errs[i][kind] / errs[i + 1][kind] for i in range(2)]
        print(f"{walls} {'wall' if kind else 'interior'}: errors {[e[kind] for e in errs]}, ratios {ratios}")
        assert min(ratios) >= gate, (errs, ratios)
