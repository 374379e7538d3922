"""Coefficient sensitivities (Solver.sensitivity, hpgmg_user_sensitivity, hpgmg_dense_unpack_sensitivity) on the CPU oracle.  DESIGN.md §11.9.

sensitivity(u, lam, boundary=g) is G_p = d/dp sum_c lam_c apply(u; g)_c.  It is checked against what defines it -- apply is affine in every
coefficient, so sum G d is lam . (apply under coefficients + d - apply under coefficients) to rounding --, entry by entry against the NumPy
restatement of the table (user_sensitivity_lib.restatement), end to end against central differences of a misfit functional through two solves,
and in pairs of calls that must give the same bytes.  Then the refusals, by name.
"""
import math

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from user_flux_lib import EPS, SOLVERS, boundary_for, faces_of, identity_bound, kappa_for, reference
from user_problem_lib import face_shape, random_coefficients
from user_robin_lib import ALL, CORNERS, SIDES, neumann_of
from user_sensitivity_lib import dot, random_direction, restatement, shifted

GRIDS = [(16, 8), (24, 8)]              # 2^3 and 3^3 boxes of 8: boxes on zero to three walls, box-to-box and periodic-wrap faces
NAMES = ["dirichlet", "periodic", "corners", "robin", "neumann"]
A, B = 1.3, 0.7


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
    rng = np.random.default_rng(seed + 1)
    u, lam = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 2.0 - 1.0
    return bc, coef, u, lam, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _solver(lib, name, n, box_dim, a, b, coef, kappa):
    s = Solver(n, box_dim=box_dim, bc=SOLVERS[name], a=a, b=b, lib=lib)
    s.set_coefficients(*coef, robin=kappa)
    return s


def _bytes(q):
    return [None if x is None else x.tobytes() for x in q]


# ---------------------------------------------------------------- 1. the linearity identity
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, A])
@pytest.mark.parametrize("name", NAMES)
def test_sum_of_G_times_d_is_the_change_of_apply(lib, name, n, box_dim, a):
    """apply is affine in every coefficient entry, so for ANY increment d (here random and positive, of every array)
    sum_p G_p d_p = lam . (apply(u; g) under coefficients + d  -  apply(u; g) under coefficients), from two solvers.  The gate is the rounding of
    the two apply results -- sum_c |lam_c| times user_flux_lib.identity_bound's per-cell bound of each -- plus 8 eps sum |G d| for G itself."""
    h = 1.0 / n
    bc, coef, u, lam, g, kappa = _problem(name, n, a, 1400 + n + int(10 * a))
    d = random_direction(coef, 1450 + n, positive=True)
    more = shifted(coef, d, 1.0)
    with _solver(lib, name, n, box_dim, a, B, coef, kappa) as s, _solver(lib, name, n, box_dim, a, B, more, kappa) as t:
        G = s.sensitivity(u, lam, boundary=g)
        assert _bytes(G) == _bytes(t.sensitivity(u, lam, boundary=g))                  # no beta, no alpha is read
        y0, y1 = s.apply(u, boundary=g), t.apply(u, boundary=g)
    assert (G[0] is None) == (a == 0.0)
    for axis in range(3):
        assert G[1 + axis].shape == face_shape(n, bc, axis) and G[1 + axis].dtype == np.float64
    lhs, magnitude = dot(G, d)
    rhs = math.fsum((lam * (y1 - y0)).ravel())
    gate = 8.0 * EPS * magnitude
    for c in (coef, more):
        per_cell = identity_bound(n, bc, a, h, c[0], u, [bnd for _, bnd in reference(n, bc, faces_of(name), B, h, c[1:], u, g, kappa)])
        gate += math.fsum((np.abs(lam) * per_cell).ravel())
    scale = EPS * math.fsum((np.abs(lam) * (np.abs(y1) + np.abs(y0))).ravel())
    print(f"{name} N={n} a={a}: sum G d = {lhs:.15e}, lam . dy = {rhs:.15e}, |difference| = {abs(lhs - rhs):.3e} = {abs(lhs - rhs) / gate:.2e} of the gate"
          f" = {abs(lhs - rhs) / scale:.3f} eps sum |lam| (|y1| + |y0|)")
    assert abs(lhs - rhs) <= gate


# ---------------------------------------------------------------- 2. entry by entry against the restatement
@pytest.mark.parametrize("n,box_dim", GRIDS)
@pytest.mark.parametrize("a", [0.0, A])
@pytest.mark.parametrize("name", NAMES)
def test_every_entry_matches_the_numpy_restatement(lib, name, n, box_dim, a):
    """Within 16 eps w (|u_lo| + |u_hi| + 2 |g|) (|lam_lo| + |lam_hi|) per face and 4 eps a |u lam| per cell.  Largest fraction of the bound reached:
    0.000 in every case -- the restatement follows the library's operation order, and then has its bits."""
    h = 1.0 / n
    bc, coef, u, lam, g, kappa = _problem(name, n, a, 1500 + n + int(10 * a))
    with _solver(lib, name, n, box_dim, a, B, coef, kappa) as s:
        got = s.sensitivity(u, lam, boundary=g)
    ref = restatement(n, bc, faces_of(name), a, B, h, u, lam, g, kappa)
    for slot, (q, (q_ref, bound)) in enumerate(zip(got, ref)):
        if q_ref is None:
            assert q is None
            continue
        assert q.shape == q_ref.shape
        excess = np.abs(q - q_ref) - bound
        used = np.abs(q - q_ref)[bound > 0.0] / bound[bound > 0.0]
        print(f"{name} N={n} a={a} array {slot}: max |G - ref| / bound = {used.max():.3f}")
        assert (excess <= 0.0).all(), (slot, np.unravel_index(excess.argmax(), excess.shape), excess.max())


# ---------------------------------------------------------------- 3. end to end: the gradient of a misfit through two solves
def _misfit(s, f, g, u_obs):
    u, info = s.solve(f, method="mg", rtol=1e-13, boundary=g)
    return 0.5 * s.h ** 3 * math.fsum(((u - u_obs) ** 2).ravel()), u


@pytest.mark.parametrize("name,a", [("dirichlet", A), ("corners", A), ("periodic", A), ("periodic", 0.0)])
def test_adjoint_gradient_against_central_differences(lib, name, a):
    """J = 1/2 h^3 sum (u - u_obs)^2 with A u = f + T(g); A lam = dJ/du = h^3 (u - u_obs) without data; dJ/dp = -G_p.  The central difference of J
    along a random direction d (entries in (-1/2, 1/2)) at eps = 0.2, 0.1, 0.05 misses -sum G d by O(eps^2): successive errors have ratios in
    [3.5, 4.5] (4.00 measured) and the last is below 1e-4 of the value (about 5e-5 measured; twice that since the seeds may differ)."""
    n = 16
    bc, coef, u_obs, _, g, kappa = _problem(name, n, a, 1600 + int(10 * a))
    f = np.random.default_rng(1601).random((n, n, n)) * 2.0 - 1.0
    d = random_direction(coef, 1602)
    with Solver(n, box_dim=8, bc=SOLVERS[name], a=a, b=B, lib=lib) as s:
        s.set_coefficients(*coef, robin=kappa)
        _, u = _misfit(s, f, g, u_obs)
        lam, _ = s.solve(s.h ** 3 * (u - u_obs), method="mg", rtol=1e-13)
        G = s.sensitivity(u, lam, boundary=g)
        value = -dot(G, d)[0]
        errors = []
        for eps in (0.2, 0.1, 0.05):
            J = []
            for sign in (1.0, -1.0):
                s.set_coefficients(*shifted(coef, d, sign * eps), robin=kappa)
                J.append(_misfit(s, f, g, u_obs)[0])
            errors.append(abs((J[0] - J[1]) / (2.0 * eps) - value))
    ratios = [errors[0] / errors[1], errors[1] / errors[2]]
    print(f"{name} a={a}: dJ/dd = {value:.12e}, errors / |value| = {[e / abs(value) for e in errors]}, ratios = {ratios}")
    assert all(3.5 <= r <= 4.5 for r in ratios), (errors, ratios)
    assert errors[2] < 1e-4 * abs(value), (errors, value)


# ---------------------------------------------------------------- 4. bytes
def test_six_dirichlet_faces_are_the_dirichlet_solver(lib):
    n = 16
    _, coef, u, lam, g, _ = _problem("dirichlet", n, A, 1710)
    with Solver(n, box_dim=8, bc="dirichlet", a=A, lib=lib) as s, Solver(n, box_dim=8, bc=("dirichlet",) * 6, a=A, lib=lib) as t:
        s.set_coefficients(*coef)
        t.set_coefficients(*coef)
        assert _bytes(s.sensitivity(u, lam, boundary=g)) == _bytes(t.sensitivity(u, lam, boundary=g))


@pytest.mark.parametrize("name", ["dirichlet", "corners", "robin", "neumann"])
def test_no_boundary_is_zero_data(lib, name):
    n = 16
    _, coef, u, lam, g, kappa = _problem(name, n, 0.0, 1720)
    with _solver(lib, name, n, 8, 0.0, 1.0, coef, kappa) as s:
        none = s.sensitivity(u, lam)
        assert _bytes(none) == _bytes(s.sensitivity(u, lam, boundary=np.zeros((6, n, n))))
        assert _bytes(none) != _bytes(s.sensitivity(u, lam, boundary=g))


@pytest.mark.parametrize("walls", [CORNERS, ALL, SIDES])
def test_kappa_zero_is_the_neumann_wall(lib, walls):
    n = 16
    coef = random_coefficients(n, "dirichlet", False, seed=1730)
    rng = np.random.default_rng(173)
    u, lam, g = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 4.0 - 2.0
    with Solver(n, box_dim=8, bc=neumann_of(walls), lib=lib) as s, Solver(n, box_dim=8, bc=walls, lib=lib) as t:
        s.set_coefficients(*coef)
        t.set_coefficients(*coef, robin=np.zeros((6, n, n)))
        assert _bytes(s.sensitivity(u, lam, boundary=g)) == _bytes(t.sensitivity(u, lam, boundary=g))
        assert _bytes(s.sensitivity(u, lam)) == _bytes(t.sensitivity(u, lam))


@pytest.mark.parametrize("name", NAMES)
def test_u_and_lam_swap_on_inner_faces_and_in_d_alpha(lib, name):
    """The written order forms the product of the two states (of their differences) first, so d_alpha and every face between two cells are
    symmetric in u and lam bit for bit.  A wall face is not symmetric at all: only u meets the data."""
    n = 16
    bc, coef, u, lam, g, kappa = _problem(name, n, A, 1740)
    with _solver(lib, name, n, 8, A, B, coef, kappa) as s:
        one, two = s.sensitivity(u, lam, boundary=g), s.sensitivity(lam, u, boundary=g)
    assert one[0].tobytes() == two[0].tobytes()
    for axis in range(3):
        x, y = np.moveaxis(one[1 + axis], 2 - axis, 0), np.moveaxis(two[1 + axis], 2 - axis, 0)
        inner = slice(None) if bc == "periodic" else slice(1, n)
        assert np.ascontiguousarray(x[inner]).tobytes() == np.ascontiguousarray(y[inner]).tobytes()
        if bc != "periodic":
            assert not np.array_equal(x[0], y[0]) and not np.array_equal(x[n], y[n])


@pytest.mark.parametrize("name", ["dirichlet", "periodic", "corners"])
def test_sensitivity_leaves_the_solver_as_it_was(lib, name):
    import ctypes
    n = 16
    bc, coef, x, lam, g, kappa = _problem(name, n, A, 1750)
    f = np.random.default_rng(175).random((n, n, n)) - 0.5
    with _solver(lib, name, n, 8, A, 1.0, coef, kappa) as s:
        u, _ = s.solve(f, boundary=g)
        again, _ = s.solve(f, method="mg", boundary=g)          # what a second solve gives without a call in between
        u, _ = s.solve(f, boundary=g)
        s.sensitivity(x, lam, boundary=None if g is None else -g)      # other operands, other data
        assert s.get_solution().tobytes() == u.tobytes()
        info = H.UserInfo()                                     # the right-hand side of the last set_rhs is still in place
        assert lib.hpgmg_user_solve(s._ptr, H.USER_MG, 1e-10, None, H.WHERE_HOST, ctypes.byref(info)) == H.USER_OK
        assert s.get_solution().tobytes() == again.tobytes()


@pytest.mark.parametrize("name", ["dirichlet", "corners"])
def test_a_march_survives_a_call(lib, name):
    """The bytes of the next step are those of an undisturbed march."""
    n = 16
    _, coef, x, lam, g, kappa = _problem(name, n, A, 1760)
    rng = np.random.default_rng(176)
    u0, f = rng.random((n, n, n)) - 0.5, rng.random((n, n, n)) - 0.5
    seen = []
    for disturb in (False, True):
        with _solver(lib, name, n, 8, A, 1.0, coef, kappa) as s:
            s.start(u0, f, boundary=g, dt=1e-3, theta=0.5)
            s.step(f, boundary=g)
            if disturb:
                s.sensitivity(x, lam, boundary=-g)
            info = s.step(f, boundary=g)
            seen.append((s.get_solution().tobytes(), s.rate().tobytes(), info.rate, info.residual))
    assert seen[0] == seen[1]


# ---------------------------------------------------------------- 5. refusals
def test_refusals(lib):
    n = 16
    _, coef, u, lam, g, _ = _problem("dirichlet", n, 0.0, 1800)
    with Solver(n, box_dim=8, lib=lib) as s:
        p4 = [np.empty(face_shape(n, "dirichlet", axis)) for axis in range(3)]
        ptr = [q.ctypes.data for q in p4]
        s.set_coefficients(*coef)
        for name, bad_u, bad_lam in (("u", True, False), ("lam", False, True)):
            bad = u.copy()
            bad[3, 4, 5] = np.nan
            with pytest.raises(ValueError, match=f"^{name}:.*not finite"):
                s.sensitivity(bad if bad_u else u, bad if bad_lam else lam, boundary=g)
            with pytest.raises(ValueError, match=f"^{name}:.*not finite"):
                s.sensitivity(bad if bad_u else u, bad if bad_lam else lam)
        for face in range(6):
            bad_g = g.copy()
            bad_g[face, n - 1, 0] = np.inf
            with pytest.raises(ValueError, match="^boundary:.*not finite"):
                s.sensitivity(u, lam, boundary=bad_g)
        with pytest.raises(ValueError, match="^u: shape"):
            s.sensitivity(u[:-1], lam)
        with pytest.raises(ValueError, match="^lam: shape"):
            s.sensitivity(u, lam[:, :-1])
        with pytest.raises(ValueError, match="^lam: dtype"):
            s.sensitivity(u, lam.astype(np.float32))
        with pytest.raises(ValueError, match="^lam: expected"):
            s.sensitivity(u, lam.tolist())
        with pytest.raises(ValueError, match="^boundary: shape"):
            s.sensitivity(u, lam, boundary=g[:5])
        good = s.sensitivity(u, lam, boundary=g)
        assert good[0] is None
        with pytest.raises(ValueError, match="^out"):
            s.sensitivity(u, lam, out=good[1:])                          # three: the wrong length
        with pytest.raises(ValueError, match="^out"):
            s.sensitivity(u, lam, out=good[1])
        with pytest.raises(ValueError, match=r"^out\[0\]"):
            s.sensitivity(u, lam, out=(np.empty((n, n, n)),) + good[1:])   # a d_alpha on a Poisson solver
        with pytest.raises(ValueError, match=r"^out\[2\]: shape"):
            s.sensitivity(u, lam, out=(None, good[1], good[3], good[3]))
        with pytest.raises(ValueError, match=r"^out\[3\]: dtype"):
            s.sensitivity(u, lam, out=(None, good[1], good[2], good[3].astype(np.float32)))
        with pytest.raises(ValueError, match=r"^out\[1\]:.*not C-contiguous"):
            s.sensitivity(u, lam, out=(None, np.empty((n + 1, n, n)).T, good[2], good[3]))
        into = (None,) + tuple(np.full_like(q, 7.0) for q in good[1:])
        assert s.sensitivity(u, lam, boundary=g, out=into)[1] is into[1] and _bytes(into) == _bytes(good)
        call = lib.hpgmg_user_sensitivity
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, *ptr, H.WHERE_HOST) == H.USER_OK
        assert call(s._ptr, None, lam.ctypes.data, None, None, *ptr, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, u.ctypes.data, None, None, None, *ptr, H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, ptr[0], None, ptr[2], H.WHERE_HOST) == H.USER_BAD_ARGUMENT
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, u.ctypes.data, *ptr, H.WHERE_HOST) == H.USER_BAD_ARGUMENT      # d_alpha with a == 0
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, *ptr, 2) == H.USER_BAD_ARGUMENT
        low = coef[1].copy()
        low[2, 2, 2] = -1.0
        with pytest.raises(ValueError, match="^beta_i"):
            s.set_coefficients(None, low, coef[2], coef[3])
        with pytest.raises(ValueError, match="^u, lam.*earlier call was refused"):
            s.sensitivity(u, lam, boundary=g)
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, *ptr, H.WHERE_HOST) == H.USER_NOT_READY
        s.set_coefficients(*coef)
        assert _bytes(s.sensitivity(u, lam, boundary=g)) == _bytes(good)
    _, coef, u, lam, _, _ = _problem("periodic", n, A, 1801)
    with Solver(n, box_dim=8, bc="periodic", a=A, lib=lib) as s:
        s.set_coefficients(*coef)
        G = s.sensitivity(u, lam)
        assert G[0] is not None and all(q.shape == (n, n, n) for q in G)
        with pytest.raises(ValueError, match="^boundary:.*Dirichlet"):
            s.sensitivity(u, lam, boundary=g)
        with pytest.raises(ValueError, match=r"^out\[0\]"):
            s.sensitivity(u, lam, out=(None,) + G[1:])                   # no d_alpha on a Helmholtz solver
        ptr = [q.ctypes.data for q in G]
        call = lib.hpgmg_user_sensitivity
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, g.ctypes.data, *ptr, H.WHERE_HOST) == H.USER_UNSUPPORTED
        assert call(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, *ptr[1:], H.WHERE_HOST) == H.USER_BAD_ARGUMENT


def test_a_call_before_set_coefficients_is_refused(lib):
    """A fresh solver runs on create's unit coefficients (flux and apply work on it), but it has no coefficient arrays to differentiate."""
    n = 16
    _, coef, u, lam, g, _ = _problem("dirichlet", n, 0.0, 1810)
    with Solver(n, box_dim=8, b=B, lib=lib) as s:
        assert s.flux(u, boundary=g) is not None
        with pytest.raises(ValueError, match="^u, lam, boundary: no valid coefficients"):
            s.sensitivity(u, lam, boundary=g)
        out = [np.empty(face_shape(n, "dirichlet", axis)) for axis in range(3)]
        assert lib.hpgmg_user_sensitivity(s._ptr, u.ctypes.data, lam.ctypes.data, None, None, *[q.ctypes.data for q in out],
                                          H.WHERE_HOST) == H.USER_NOT_READY
        s.set_coefficients(*coef)
        got = s.sensitivity(u, lam, boundary=g)
    ref = restatement(n, "dirichlet", None, 0.0, B, 1.0 / n, u, lam, g)
    assert got[0] is None and _bytes(got[1:]) == _bytes([q for q, _ in ref[1:]])


def test_the_coefficient_version_counts_set_coefficients_and_set_shift(lib):
    n = 16
    _, coef, _, _, _, _ = _problem("dirichlet", n, A, 1820)
    with Solver(n, box_dim=8, a=A, lib=lib) as s:
        v0 = s.coefficient_version
        s.set_coefficients(*coef)
        v1 = s.coefficient_version
        s.set_shift(2.0)
        assert v0 < v1 < s.coefficient_version
