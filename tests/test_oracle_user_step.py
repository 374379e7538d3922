"""Implicit time stepping of the dense-array solver (Solver.start / step / rate / set_shift) on the CPU oracle:
the exact amplification of an eigenvector, the scheme's identity with data that changes in time, the rate's independence of the solver's
tolerance, set_shift against a fresh solver bit for bit, a dt change mid-march, and the lifecycle and refusals.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver, StepInfo
from hpgmg_testlib import Backend
from user_problem_lib import face_shape
from user_step_lib import (B, ROUNDING_FACTOR, ROUNDING_MEASURED, ROUNDING_MEASURED_IDENTITY, data, initial, march, problem, rounding_gate, rounding_scale, spatial)

WALLS = ["dirichlet", "corners", "robin"]


@pytest.fixture(scope="module")
def lib():
    lib = Backend.oracle().lib
    lib.hpgmg_set_verbose(0)
    return lib


def _solver(lib, name, n, box_dim, seed, a=1.0):
    bc, coef, kappa = problem(name, n, seed)
    s = Solver(n, box_dim=box_dim, bc=bc, a=a, b=B, lib=lib)
    s.set_coefficients(*coef, robin=kappa)
    return s, coef


# ---- 1. exact amplification
@pytest.mark.parametrize("theta", [1.0, 0.75, 0.5])
@pytest.mark.parametrize("bc,box_dim,d,kappa", [("periodic", 16, 1, 2.0 * np.pi), ("dirichlet", 8, 3, np.pi)])
def test_an_eigenvector_is_amplified_exactly(lib, bc, box_dim, d, kappa, theta):
    """u0 is an eigenvector of the discrete operator (the p1 ghost -u is the mode's own continuation), so after k steps u = G^k u0 and the rate
    is -mu G^k u0.  A is an M-matrix with row sums >= a min(alpha), so |A^-1|_inf <= 1/a and a step stopped at rtol |F| is off by at most
    rtol |F| / a; the gate is 10 times the sum of that over the steps (the factor covers the inf-norm growth of a Crank-Nicolson step), times a
    for the rate."""
    n, b, dt, steps, rtol = 16, 1.0, 0.01, 4, 1e-10
    h = 1.0 / n
    c = (np.arange(n) + 0.5) * h
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    u0 = np.ascontiguousarray(np.cos(2.0 * np.pi * x) if bc == "periodic" else np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z))
    mu = d * b * (2.0 - 2.0 * np.cos(kappa * h)) / (h * h)
    G = (1.0 - (1.0 - theta) * dt * mu) / (1.0 + theta * dt * mu)
    f = np.zeros((n, n, n))
    with Solver(n, box_dim=box_dim, bc=bc, a=1.0, b=b, lib=lib) as s:
        s.set_coefficients(np.ones((n, n, n)), *[np.ones(face_shape(n, bc, axis)) for axis in range(3)])
        s.start(u0, f, dt=dt, theta=theta)
        assert s.a == 1.0 / (theta * dt)
        gate = 0.0
        for k in range(steps):
            info = s.step(f, rtol=rtol)
            assert isinstance(info, StepInfo) and info.converged and info.t == pytest.approx((k + 1) * dt)
            gate += 10.0 * rtol * info.norm_f / s.a
        u, w = s.get_solution(), s.rate()
    err_u, err_w = np.abs(u - G ** steps * u0).max(), np.abs(w + mu * G ** steps * u0).max()
    print(f"{bc} theta={theta}: |u - G^k u0| = {err_u:.3e} (gate {gate:.3e}), |w + mu G^k u0| = {err_w:.3e} (gate {gate * s.a:.3e})")
    assert err_u <= gate
    assert err_w <= gate * s.a
    assert info.rate == np.abs(w).max()


# ---- 2. the scheme's identity, 3. the rate does not inherit the tolerance
def _identity_march(lib, name, theta, rtol):
    """Two steps with data that changes in time; per step (defect, info, s.a, gate, rate array, f - L(u1; g1))."""
    n, seed, dt = 24, 300, 2e-3
    s, coef = _solver(lib, name, n, 8, seed)
    alpha = coef[0]
    out = []
    with s:
        u0 = initial(n, seed)
        f0, g0 = data(name, n, seed, 0)
        s.start(u0, f0, boundary=g0, dt=dt, theta=theta)
        for k in (1, 2):
            f1, g1 = data(name, n, seed, k)
            info = s.step(f1, boundary=g1, rtol=rtol)
            u1 = s.get_solution()
            L0, L1 = spatial(s, alpha, u0, g0), spatial(s, alpha, u1, g1)
            defect = alpha * (u1 - u0) / dt + theta * (L1 - f1) + (1.0 - theta) * (L0 - f0)
            out.append((defect, info, s.a, rounding_scale(s, coef, u0, u1), s.rate(), f1 - L1))
            u0, f0, g0 = u1, f1, g1
    return out


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", WALLS)
def test_a_step_satisfies_the_theta_scheme(lib, name, theta):
    """alpha (u1 - u0) / dt + theta (L(u1; g1) - f1) + (1 - theta) (L(u0; g0) - f0) is -theta r, r the residual the step's solve stopped at: its
    inf-norm is theta info.residual up to the rounding of L (user_step_lib.ROUNDING_MEASURED_IDENTITY, this check's own measured constant,
    gated at ROUNDING_FACTOR times it)."""
    for defect, info, _, scale, _, _ in _identity_march(lib, name, theta, 1e-8):
        off = abs(np.abs(defect).max() - theta * info.residual)
        print(f"{name} theta={theta}: |defect| = {np.abs(defect).max():.3e}, theta r = {theta * info.residual:.3e}, off by {off / scale:.3f} rounding scales")
        assert info.converged
        assert off <= ROUNDING_FACTOR * ROUNDING_MEASURED_IDENTITY * scale


@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", WALLS)
def test_the_rate_does_not_inherit_the_tolerance(lib, name, theta):
    """With the loose rtol = 1e-3 the rate still equals f1 - L(u1; g1) to rounding: formula (2) carries the solve's residual."""
    for _, info, _, scale, w, expected in _identity_march(lib, name, theta, 1e-3):
        off = np.abs(w - expected).max()
        print(f"{name} theta={theta}: |w - (f - L u)| = {off:.3e} = {off / scale:.3f} rounding scales; the step's residual was {info.residual:.3e}")
        assert info.residual > 1e3 * off                       # the solve did stop far above rounding
        assert off <= ROUNDING_FACTOR * ROUNDING_MEASURED * scale
        assert info.rate == np.abs(w).max()


# ---- 4. set_shift is a fresh solver's operator
@pytest.mark.parametrize("name", ["dirichlet", "periodic", "robin"])
def test_set_shift_gives_a_fresh_solvers_bytes(lib, name):
    n, seed = 24, 400
    f, _ = data(name, n, seed, 0)
    x = initial(n, seed)
    fresh, _ = _solver(lib, name, n, 8, seed, a=37.5)
    shifted, _ = _solver(lib, name, n, 8, seed, a=1.0)
    with fresh, shifted:
        shifted.set_shift(37.5)
        assert shifted.a == 37.5
        for method in ("fmg", "mg"):
            (u_f, i_f), (u_s, i_s) = fresh.solve(f, method=method, rtol=1e-9), shifted.solve(f, method=method, rtol=1e-9)
            assert u_f.tobytes() == u_s.tobytes() and i_f == i_s, method
        assert fresh.apply(x).tobytes() == shifted.apply(x).tobytes()
        shifted.set_shift(2.0)                                    # and back down, with a right-hand side in place: it stays valid
        shifted.set_shift(37.5)
        assert fresh.apply(x).tobytes() == shifted.apply(x).tobytes()


# ---- 5. a dt change mid-march
@pytest.mark.parametrize("theta", [1.0, 0.5])
@pytest.mark.parametrize("name", WALLS)
def test_a_dt_change_mid_march(lib, name, theta):
    """Steps at dt, dt, dt/4 against a march started afresh from the state after step 2.  start's w and the marched w agree to rounding, not to
    the last bit, so the two marches are compared to the rounding gate (user_step_lib.rounding_gate): the rate arrays to the gate itself, the
    states to the gate divided by a (|A^-1|_inf <= 1/a).  The operator after the change is, byte for byte, that of a solver built with the new
    a.  Printed for information only: the rigorous worst case that also allows each solve to stop anywhere within rtol |F| of its solution,
    (2 c gate + 2 rtol |F|) / a for u and 2 gate + 12 b max(beta) / h^2 times that for w."""
    n, seed, dt, rtol = 24, 500, 2e-3, 1e-10
    s, coef = _solver(lib, name, n, 8, seed)
    alpha = coef[0]
    x = initial(n, seed + 1)
    with s:
        f, g = data(name, n, seed, 0)
        s.start(initial(n, seed), f, boundary=g, dt=dt, theta=theta)
        for k in (1, 2):
            f2, g2 = data(name, n, seed, k)
            s.step(f2, boundary=g2, rtol=rtol)
        u2 = s.get_solution()
        f3, g3 = data(name, n, seed, 3)
        info = s.step(f3, boundary=g3, dt=dt / 4.0, rtol=rtol)
        u3, w3, Ax = s.get_solution(), s.rate(), s.apply(x)
        assert s.a == 1.0 / (theta * dt / 4.0) and info.t == pytest.approx(2.25 * dt)
        gate = rounding_gate(s, coef, u2, u3)
    fresh, _ = _solver(lib, name, n, 8, seed, a=1.0 / (theta * dt / 4.0))
    with fresh:
        assert fresh.apply(x).tobytes() == Ax.tobytes()
        fresh.start(u2, f2, boundary=g2, dt=dt / 4.0, theta=theta)
        info_f = fresh.step(f3, boundary=g3, rtol=rtol)
        v3, z3 = fresh.get_solution(), fresh.rate()
        c, a = (1.0 - theta) / theta, fresh.a
        du = (2.0 * c * gate + 2.0 * rtol * max(info.norm_f, info_f.norm_f)) / a
        dw = 2.0 * gate + 12.0 * fresh.b * max(q.max() for q in coef[1:]) / (fresh.h * fresh.h) * du
    print(f"{name} theta={theta}: |du| = {np.abs(u3 - v3).max():.3e} (gate {gate / a:.3e}), |dw| = {np.abs(w3 - z3).max():.3e} (gate {gate:.3e}); "
          f"worst case with the solves' tolerance {du:.3e} / {dw:.3e}")
    assert np.abs(u3 - v3).max() <= gate / a
    assert np.abs(w3 - z3).max() <= gate


# ---- 6. lifecycle and refusals
def _refused(call, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        call(*args, **kwargs)
    return str(e.value)


def _num_vectors(lib, s):
    info = (ctypes.c_int * H.INFO_COUNT)()
    lib.hpgmg_level_info(lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0), info)
    return info[H.INFO_NUM_VECTORS]


def test_step_needs_a_march_and_solve_set_rhs_set_coefficients_end_it(lib):
    name, n, seed, dt = "corners", 16, 600, 1e-2
    s, coef = _solver(lib, name, n, 8, seed)
    bc, _, kappa = problem(name, n, seed)
    f, g = data(name, n, seed, 0)
    u0 = initial(n, seed)
    with s:
        assert _refused(s.step, f, boundary=g).startswith("step: no march is live")
        assert _refused(s.rate).startswith("rate: no march is live")
        assert lib.hpgmg_user_step(s._ptr, f.ctypes.data, g.ctypes.data, H.WHERE_HOST, dt, 1.0, 1e-8, None, None) == H.USER_NOT_READY
        assert _num_vectors(lib, s) == lib.hpgmg_vectors_reserved() + 1      # a solver that never starts: its vectors on the parent commit
        for end in ("solve", "set_rhs", "set_coefficients"):
            s.start(u0, f, boundary=g, dt=dt)
            s.step(f, boundary=g)
            if end == "solve":
                s.solve(f, boundary=g)
            elif end == "set_rhs":
                s.set_rhs(f, boundary=g)
            else:
                s.set_coefficients(*coef, robin=kappa)
            assert _refused(s.step, f, boundary=g).startswith("step: no march is live"), end
            assert _refused(s.rate).startswith("rate: no march is live"), end
        assert _num_vectors(lib, s) == lib.hpgmg_vectors_reserved() + 3      # the first start added two, the later ones none
        u, info = s.solve(f, boundary=g)                                     # and the solver still solves as one that never marched
        assert s.a == 1.0 / dt                                               # (the march left its a)
    fresh, _ = _solver(lib, name, n, 8, seed, a=1.0 / dt)
    with fresh:
        u_f, info_f = fresh.solve(f, boundary=g)
        assert _num_vectors(lib, fresh) == lib.hpgmg_vectors_reserved() + 1
    assert u.tobytes() == u_f.tobytes() and info == info_f


def test_apply_flux_and_get_solution_do_not_end_a_march(lib):
    name, n, seed = "robin", 16, 700
    plain = march(lib, n, 8, name, seed, 0.5, [1e-2, 1e-2, 1e-2], 1e-8)
    s, coef = _solver(lib, name, n, 8, seed)
    x = initial(n, seed + 1)
    with s:
        f, g = data(name, n, seed, 0)
        s.start(initial(n, seed), f, boundary=g, dt=1e-2, theta=0.5)
        for k in (1, 2, 3):
            f, g = data(name, n, seed, k)
            info = s.step(f, boundary=g)
            st, u, w, fields, rate = plain[k - 1]
            assert st == H.USER_OK and s.get_solution().tobytes() == u.tobytes() and s.rate().tobytes() == w.tobytes(), k
            assert (info.residual, info.norm_f, info.mean_shift, info.vcycles, int(info.converged), info.rate) == fields + (rate,), k
            s.apply(x)
            s.apply(x, boundary=g)
            s.flux(x, boundary=g)
            assert s.get_solution().tobytes() == u.tobytes() and s.rate().tobytes() == w.tobytes(), k


@pytest.mark.parametrize("what", ["f", "g"])
def test_a_refused_step_leaves_the_march_intact(lib, what):
    name, n, seed, dts = "corners", 16, 800, [1e-2, 1e-2, 5e-3]
    plain = march(lib, n, 8, name, seed, 0.5, dts, 1e-8)
    spoiled = march(lib, n, 8, name, seed, 0.5, dts, 1e-8, spoil=(2, what))
    assert spoiled[1] == ("refused", H.USER_NOT_FINITE)
    del spoiled[1]
    for k, (ref, got) in enumerate(zip(plain, spoiled), start=1):
        assert got[0] == ref[0] == H.USER_OK
        assert got[1].tobytes() == ref[1].tobytes() and got[2].tobytes() == ref[2].tobytes() and got[3:] == ref[3:], k


def test_bad_arguments_are_refused_by_name(lib):
    name, n, seed = "dirichlet", 16, 900
    s, coef = _solver(lib, name, n, 8, seed)
    f, g = data(name, n, seed, 0)
    u0 = initial(n, seed)
    with s:
        assert _refused(s.start, u0, f).startswith("dt: required")
        for dt in (0.0, -1.0, np.inf):
            assert _refused(s.start, u0, f, dt=dt).startswith("dt:"), dt
        for theta in (0.49, 1.01, 0.0, np.nan):
            assert _refused(s.start, u0, f, dt=0.1, theta=theta).startswith("theta:"), theta
        assert lib.hpgmg_user_start(s._ptr, u0.ctypes.data, f.ctypes.data, None, H.WHERE_HOST, 0.1, 0.25) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_start(s._ptr, u0.ctypes.data, f.ctypes.data, None, H.WHERE_HOST, 0.0, 1.0) == H.USER_BAD_ARGUMENT
        for a in (0.0, -2.0, np.inf, np.nan):
            assert _refused(s.set_shift, a).startswith("a:"), a
            assert lib.hpgmg_user_set_shift(s._ptr, float(a)) == H.USER_BAD_ARGUMENT
        bad = u0.copy()
        bad[1, 2, 3] = np.inf
        assert _refused(s.start, bad, f, dt=0.1).startswith("u: holds a value that is not finite")
        assert _refused(s.step, f).startswith("step: no march is live")           # the refused start began none
        s.start(u0, f, boundary=g, dt=0.1)
        assert _refused(s.step, f, theta=0.3).startswith("theta:")
        assert _refused(s.step, f, dt=-0.1).startswith("dt:")
        assert _refused(s.step, f, rtol=0.0).startswith("rtol:")
        assert _refused(s.step, f[:8]).startswith("f: shape")
        nan_g = g.copy()
        nan_g[5, 0, 0] = np.nan
        assert _refused(s.step, f, boundary=nan_g).startswith("boundary: holds a value that is not finite")
        s.step(f, boundary=g)                                                    # the march is still live
    with Solver(n, box_dim=8, a=0.0, lib=lib) as poisson:
        assert _refused(poisson.start, u0, f, dt=0.1).startswith("a: time stepping needs a Helmholtz solver")
        assert _refused(poisson.set_shift, 2.0).startswith("a: this solver is Poisson")
        assert lib.hpgmg_user_start(poisson._ptr, u0.ctypes.data, f.ctypes.data, None, H.WHERE_HOST, 0.1, 1.0) == H.USER_BAD_ARGUMENT
        assert lib.hpgmg_user_set_shift(poisson._ptr, 2.0) == H.USER_BAD_ARGUMENT
    with Solver(n, box_dim=8, bc="periodic", a=1.0, lib=lib) as p:
        p.set_coefficients(np.zeros((n, n, n)), *[np.ones((n, n, n))] * 3)
        assert _refused(p.start, u0, f, dt=0.1).startswith("alpha: zero everywhere")
        assert _refused(p.start, u0, f, boundary=g, dt=0.1).startswith("boundary: boundary values need a Dirichlet domain")
