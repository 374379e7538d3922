"""The Newmark march of the dense-array solver (Solver.wave_start / wave_step / velocity / acceleration) on the CPU oracle: the exact
propagation of an eigenvector against the scalar recurrence (and the closed form of the average-acceleration rule), the defect identity with data that
changes in time and a dt change, the discrete energy balance and the potential-energy formula, and the lifecycle and refusals.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import user_wave_lib as W
from hpgmg_amd.problem import Solver, WaveInfo
from hpgmg_testlib import Backend
from user_problem_lib import face_shape
from user_step_lib import B, data, initial, problem, rounding_scale, spatial

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


# ---- (b) exact propagation of an eigenvector
@pytest.mark.parametrize("rule", W.RULES, ids=lambda r: "beta%g-gamma%g-sigma%g" % r)
@pytest.mark.parametrize("bc,box_dim,d,kappa", [("periodic", 16, 1, 2.0 * np.pi), ("dirichlet", 8, 3, np.pi)])
def test_an_eigenvector_is_propagated_exactly(lib, bc, box_dim, d, kappa, rule):
    """u0 = phi is an eigenvector of the discrete K (eigenvalue mu; alpha = 1) and v0 = 0, so u, v, q stay multiples of phi whose factors follow the
    scheme on the oscillator s'' + sigma s' + mu s = 0; for (1/4, 1/2, 0) that is s_n = cos(2 n atan(omega dt / 2)).  A0 is an M-matrix with row sums
    >= a min(alpha), so |A0^-1|_inf <= 1/a and a step stopped at rtol |F| is off by at most rtol |F| / a in u; the gate is 10 times the sum of that over
    the steps, times gamma / (beta dt) for v and 1 / (beta dt^2) for q (the corrector's factors)."""
    n, b, dt, steps, rtol = 16, 1.0, 0.01, 4, 1e-10
    beta, gamma, sigma = rule
    h = 1.0 / n
    c = (np.arange(n) + 0.5) * h
    z, y, x = np.meshgrid(c, c, c, indexing="ij")
    phi = np.ascontiguousarray(np.cos(2.0 * np.pi * x) if bc == "periodic" else np.sin(np.pi * x) * np.sin(np.pi * y) * np.sin(np.pi * z))
    mu = d * b * (2.0 - 2.0 * np.cos(kappa * h)) / (h * h)
    zero = np.zeros((n, n, n))
    with Solver(n, box_dim=box_dim, bc=bc, a=1.0, b=b, lib=lib) as s:
        s.set_coefficients(np.ones((n, n, n)), *[np.ones(face_shape(n, bc, axis)) for axis in range(3)])
        info = s.wave_start(phi, zero, zero, dt=dt, beta=beta, gamma=gamma, damping=sigma)
        assert isinstance(info, WaveInfo) and info.t == 0.0 and info.vcycles == 0 and s.a == W.shift(dt, beta, gamma, sigma)
        assert info.kinetic == 0.0 and info.potential == pytest.approx(0.5 * h ** 3 * mu * (phi * phi).sum(), rel=1e-10)
        gate = 0.0
        for k in range(steps):
            info = s.wave_step(zero, rtol=rtol)
            assert info.converged and info.t == pytest.approx((k + 1) * dt)
            gate += 10.0 * rtol * info.norm_f / s.a
        u, v, q = s.get_solution(), s.velocity(), s.acceleration()
    sn, vn, qn = W.oscillator(mu, dt, beta, gamma, sigma, steps)[-1]
    errs = np.abs(u - sn * phi).max(), np.abs(v - vn * phi).max(), np.abs(q - qn * phi).max()
    gates = gate, gate * gamma / (beta * dt), gate / (beta * dt * dt)
    print(f"{bc} {rule}: |u - s phi| = {errs[0]:.3e} (gate {gates[0]:.3e}), |v - s' phi| = {errs[1]:.3e} (gate {gates[1]:.3e}), "
          f"|q - s'' phi| = {errs[2]:.3e} (gate {gates[2]:.3e})")
    for err, g in zip(errs, gates):
        assert err <= g
    if rule == (0.25, 0.5, 0.0):
        closed = np.cos(2.0 * steps * np.arctan(np.sqrt(mu) * dt / 2.0))
        assert abs(sn - closed) <= 64 * W.EPS and np.abs(u - closed * phi).max() <= gate


# ---- (c) the defect identity
@pytest.mark.parametrize("sigma", [0.0, 0.7])
@pytest.mark.parametrize("name", WALLS)
def test_the_equation_at_the_new_time_holds_with_defect_minus_r(lib, name, sigma):
    """alpha q + sigma alpha v + apply(u, boundary=g) - a alpha u - f, formed from the arrays the API returns, is -r, r the residual the step's solve
    stopped at: its inf-norm is info.residual up to the rounding of apply - a alpha u (user_step_lib.rounding_scale; the constant measured on the oracle
    is user_wave_lib.DEFECT_MEASURED, gated at ROUNDING_FACTOR times it).  Random coefficients, f and g that change every step, a dt change at the third
    step.  At the start the defect is rounding alone: q0 is defined by the equation."""
    n, seed, dt, rtol = 24, 300, 2e-3, 1e-6
    s, coef = _solver(lib, name, n, 8, seed)
    alpha = coef[0]
    worst = 0.0
    with s:
        f, g = data(name, n, seed, 0)
        info = s.wave_start(initial(n, seed), W.velocity0(n, seed), f, boundary=g, dt=dt, damping=sigma)
        for k in range(4):
            if k:
                f, g = data(name, n, seed, k)
                info = s.wave_step(f, boundary=g, dt=dt / 4.0 if k == 3 else None, rtol=rtol)
                assert info.converged and info.residual > 0.0
            u, v, q = s.get_solution(), s.velocity(), s.acceleration()
            defect = alpha * q + sigma * alpha * v + spatial(s, alpha, u, g) - f
            scale = rounding_scale(s, coef, u)
            off = abs(np.abs(defect).max() - (info.residual if k else 0.0))
            worst = max(worst, off / scale)
            print(f"{name} sigma={sigma} step {k}: |defect| = {np.abs(defect).max():.3e}, |r| = {info.residual if k else 0.0:.3e}, off by {off / scale:.3f} rounding scales")
            assert off <= W.ROUNDING_FACTOR * W.DEFECT_MEASURED * scale
        assert s.a == W.shift(dt / 4.0, 0.25, 0.5, sigma) and info.t == pytest.approx(2.25 * dt)
    print(f"{name} sigma={sigma}: worst {worst:.3f} rounding scales")


# ---- (d) energy
def _energy_rounding(s, coef, u):
    """The scale of the rounding of h^3/2 sum u ((F - r) - (a alpha) u): per cell |u| times user_step_lib.rounding_scale, over the volume, halved."""
    return 0.5 * (s.n * s.h) ** 3 * np.abs(u).max() * rounding_scale(s, coef, u)


@pytest.mark.parametrize("sigma", [0.0, 0.7])
@pytest.mark.parametrize("name", WALLS)
def test_the_energy_balance_of_the_average_acceleration_rule(lib, name, sigma):
    """With f = 0 and g = 0 the rule (1/4, 1/2) satisfies  E1 - E0 = -sigma dt h^3 sum alpha ((v0 + v1)/2)^2 - h^3 (u1 - u0).(r0 + r1)/2  with E = kinetic +
    potential as WaveInfo reports them.  The first term comes from velocity(); the second is bounded by Vol |u1 - u0|_inf rtol |F|_inf; the rest is the
    rounding of the two potential energies (ENERGY_MEASURED of _energy_rounding each, gated at ROUNDING_FACTOR times it).  And the potential energy, which
    the step takes from its closing residual, equals h^3/2 sum u (apply(u) - a alpha u) to that rounding."""
    n, seed, dt, rtol, steps = 24, 900, 2e-3, 1e-10, 5
    s, coef = _solver(lib, name, n, 8, seed)
    alpha = coef[0]
    zero = np.zeros((n, n, n))
    vol, worst = 1.0, [0.0, 0.0]
    with s:
        info0 = s.wave_start(initial(n, seed), W.velocity0(n, seed), zero, dt=dt, damping=sigma)
        u0, v0 = s.get_solution(), s.velocity()
        for k in range(steps + 1):
            if k:
                info1 = s.wave_step(zero, rtol=rtol)
                u1, v1 = s.get_solution(), s.velocity()
                vbar = 0.5 * (v0 + v1)
                damped = -sigma * dt * s.h ** 3 * (alpha * vbar * vbar).sum()
                slack = vol * np.abs(u1 - u0).max() * rtol * info1.norm_f
                rounding = _energy_rounding(s, coef, u0) + _energy_rounding(s, coef, u1)
                off = abs((info1.energy - info0.energy) - damped)
                worst[0] = max(worst[0], max(0.0, off - slack) / rounding)
                print(f"{name} sigma={sigma} step {k}: E = {info1.energy:.12e}, E1 - E0 = {info1.energy - info0.energy:.3e}, damping {damped:.3e}, "
                      f"off by {off:.3e} (tolerance slack {slack:.3e}, rounding scale {rounding:.3e})")
                assert info1.converged and off <= slack + W.ROUNDING_FACTOR * W.ENERGY_MEASURED * rounding
                assert info1.kinetic == pytest.approx(0.5 * s.h ** 3 * (alpha * v1 * v1).sum(), rel=1e-12)
                if sigma == 0.0:
                    assert abs(info1.energy - info0.energy) <= 1e-9 * info0.energy      # conserved: far below any physical change
                info0, u0, v0 = info1, u1, v1
            direct = 0.5 * s.h ** 3 * (u0 * (s.apply(u0) - s.a * alpha * u0)).sum()
            off = abs(info0.potential - direct)
            worst[1] = max(worst[1], off / _energy_rounding(s, coef, u0))
            assert off <= W.ROUNDING_FACTOR * W.ENERGY_MEASURED * _energy_rounding(s, coef, u0), (k, info0.potential, direct)
    print(f"{name} sigma={sigma}: worst balance {worst[0]:.4f}, worst potential {worst[1]:.4f} energy rounding scales")


# ---- (e) lifecycle and refusals
def _refused(call, *args, **kwargs):
    with pytest.raises(ValueError) as e:
        call(*args, **kwargs)
    return str(e.value)


def _num_vectors(lib, s):
    info = (ctypes.c_int * H.INFO_COUNT)()
    lib.hpgmg_level_info(lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0), info)
    return info[H.INFO_NUM_VECTORS]


def test_bad_arguments_are_refused_by_name(lib):
    name, n, seed = "dirichlet", 16, 900
    s, coef = _solver(lib, name, n, 8, seed)
    f, g = data(name, n, seed, 0)
    u0, v0 = initial(n, seed), W.velocity0(n, seed)
    P = lambda a: a.ctypes.data  # noqa: E731
    with s:
        assert _refused(s.wave_start, u0, v0, f).startswith("dt: required")
        for dt in (0.0, -1.0, np.inf, np.nan):
            assert _refused(s.wave_start, u0, v0, f, dt=dt).startswith("dt:"), dt
            assert lib.hpgmg_user_wave_start(s._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, dt, 0.25, 0.5, 0.0, None) == H.USER_BAD_ARGUMENT
        for sigma in (-0.1, np.inf, np.nan):
            assert _refused(s.wave_start, u0, v0, f, dt=0.1, damping=sigma).startswith("damping:"), sigma
            assert lib.hpgmg_user_wave_start(s._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, 0.1, 0.25, 0.5, sigma, None) == H.USER_BAD_ARGUMENT
        # the conditionally stable rules: gamma < 1/2, beta < gamma / 2, central differences (beta = 0) included
        for beta, gamma, who in ((0.25, 0.49, "gamma:"), (0.0, 0.5, "beta:"), (0.24, 0.5, "beta:"), (0.29, 0.6, "beta:"), (np.nan, 0.5, "beta:"), (0.25, np.inf, "gamma:")):
            assert _refused(s.wave_start, u0, v0, f, dt=0.1, beta=beta, gamma=gamma).startswith(who), (beta, gamma)
            assert lib.hpgmg_user_wave_start(s._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, 0.1, beta, gamma, 0.0, None) == H.USER_BAD_ARGUMENT
        assert _refused(s.wave_start, u0, v0, f, dt=1e-200).startswith("dt:")                     # a is not finite
        assert lib.hpgmg_user_wave_start(s._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, 1e-200, 0.25, 0.5, 0.0, None) == H.USER_BAD_ARGUMENT
        for slot, who in ((0, "u"), (1, "v"), (2, "f")):
            arrays = [u0.copy(), v0.copy(), f.copy()]
            arrays[slot][1, 2, 3] = np.inf
            assert _refused(s.wave_start, *arrays, dt=0.1).startswith(f"{who}: holds a value that is not finite")
        assert _refused(s.wave_step, f).startswith("wave_step: no wave march is live")              # the refused starts began none
        assert _refused(s.velocity).startswith("velocity: no wave march is live")
        assert _refused(s.acceleration).startswith("acceleration: no wave march is live")
        assert lib.hpgmg_user_wave_step(s._ptr, P(f), None, H.WHERE_HOST, 0.1, 1e-8, None) == H.USER_NOT_READY
        s.wave_start(u0, v0, f, boundary=g, dt=0.1)
        assert _refused(s.wave_step, f, dt=-0.1).startswith("dt:")
        assert _refused(s.wave_step, f, rtol=0.0).startswith("rtol:")
        assert _refused(s.wave_step, f[:8]).startswith("f: shape")
        nan_g = g.copy()
        nan_g[5, 0, 0] = np.nan
        assert _refused(s.wave_step, f, boundary=nan_g).startswith("boundary: holds a value that is not finite")
        assert s.wave_step(f, boundary=g).t == pytest.approx(0.1)                                   # the march is still live
    with Solver(n, box_dim=8, a=0.0, lib=lib) as poisson:
        assert _refused(poisson.wave_start, u0, v0, f, dt=0.1).startswith("a: the wave march needs a Helmholtz solver")
        assert lib.hpgmg_user_wave_start(poisson._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, 0.1, 0.25, 0.5, 0.0, None) == H.USER_BAD_ARGUMENT
    with Solver(n, box_dim=8, bc="periodic", a=1.0, lib=lib) as p:
        assert _refused(p.wave_start, u0, v0, f, boundary=g, dt=0.1).startswith("boundary: boundary values need a Dirichlet domain")
        assert lib.hpgmg_user_wave_start(p._ptr, P(u0), P(v0), P(f), P(g), H.WHERE_HOST, 0.1, 0.25, 0.5, 0.0, None) == H.USER_UNSUPPORTED
        alpha = np.ones((n, n, n))
        alpha[3, 2, 1] = 0.0
        p.set_coefficients(alpha, *[np.ones((n, n, n))] * 3)
        assert _refused(p.wave_start, u0, v0, f, dt=0.1).startswith("alpha: zero in some cell")
        assert lib.hpgmg_user_wave_start(p._ptr, P(u0), P(v0), P(f), None, H.WHERE_HOST, 0.1, 0.25, 0.5, 0.0, None) == H.USER_OUT_OF_RANGE


def test_only_one_march_is_live(lib):
    """step / rate on a wave march and wave_step / velocity / acceleration on a theta march answer NOT_READY; each start ends the other march."""
    name, n, seed, dt = "corners", 16, 600, 1e-2
    s, coef = _solver(lib, name, n, 8, seed)
    f, g = data(name, n, seed, 0)
    u0, v0 = initial(n, seed), W.velocity0(n, seed)
    P = lambda a: a.ctypes.data  # noqa: E731
    with s:
        s.wave_start(u0, v0, f, boundary=g, dt=dt)
        assert _refused(s.step, f, boundary=g).startswith("step: no march is live")
        assert _refused(s.rate).startswith("rate: no march is live")
        assert lib.hpgmg_user_step(s._ptr, P(f), P(g), H.WHERE_HOST, dt, 1.0, 1e-8, None, None) == H.USER_NOT_READY
        assert lib.hpgmg_user_get_rate(s._ptr, P(np.empty((n, n, n))), H.WHERE_HOST) == H.USER_NOT_READY
        s.wave_step(f, boundary=g)                                                                 # the refusals left the wave march alone
        s.start(u0, f, boundary=g, dt=dt)
        assert _refused(s.wave_step, f, boundary=g).startswith("wave_step: no wave march is live")
        assert _refused(s.velocity).startswith("velocity: no wave march is live")
        assert lib.hpgmg_user_wave_step(s._ptr, P(f), P(g), H.WHERE_HOST, dt, 1e-8, None) == H.USER_NOT_READY
        assert lib.hpgmg_user_get_acceleration(s._ptr, P(np.empty((n, n, n))), H.WHERE_HOST) == H.USER_NOT_READY
        s.step(f, boundary=g)                                                                      # and the theta march


def test_what_ends_a_wave_march_and_what_does_not(lib):
    name, n, seed, dt = "corners", 16, 600, 1e-2
    s, coef = _solver(lib, name, n, 8, seed)
    bc, _, kappa = problem(name, n, seed)
    f, g = data(name, n, seed, 0)
    u0, v0, x = initial(n, seed), W.velocity0(n, seed), initial(n, seed + 1)
    with s:
        assert _num_vectors(lib, s) == lib.hpgmg_vectors_reserved() + 1      # a solver that never marches keeps its vectors
        for end in ("solve", "set_rhs", "set_coefficients", "eigs", "start"):
            s.wave_start(u0, v0, f, boundary=g, dt=dt)
            s.wave_step(f, boundary=g)
            if end == "solve":
                s.solve(f, boundary=g)
            elif end == "set_rhs":
                s.set_rhs(f, boundary=g)
            elif end == "set_coefficients":
                s.set_coefficients(*coef, robin=kappa)
            elif end == "eigs":
                s.eigs(1, max_iter=1)
            else:
                s.start(u0, f, boundary=g, dt=dt)
            assert _refused(s.wave_step, f, boundary=g).startswith("wave_step: no wave march is live"), end
            assert _refused(s.velocity).startswith("velocity: no wave march is live"), end
            assert _refused(s.acceleration).startswith("acceleration: no wave march is live"), end
        s.wave_start(u0, v0, f, boundary=g, dt=dt)
        info = s.wave_step(f, boundary=g)
        u, v, q = s.get_solution(), s.velocity(), s.acceleration()
        s.apply(x); s.apply(x, boundary=g); s.flux(x, boundary=g); s.sensitivity(x, x, boundary=g)
        assert s.get_solution().tobytes() == u.tobytes() and s.velocity().tobytes() == v.tobytes() and s.acceleration().tobytes() == q.tobytes()
        assert s.wave_step(f, boundary=g).t == pytest.approx(2 * dt)


def test_wave_start_after_a_theta_march_and_after_pcg(lib):
    """The wave march shares the theta march's two vectors and adds one; a first pcg after them uses those ids as its own.  A wave march started after
    either computes the bits of one on a fresh solver."""
    name, n, seed, dts = "robin", 16, 700, [1e-2, 1e-2, 5e-3]
    rule = (0.3025, 0.6, 0.2)
    fresh = W.march(lib, n, 8, name, seed, rule, dts, 1e-8)
    s, coef = _solver(lib, name, n, 8, seed)
    with s:
        f0, g0 = data(name, n, seed, 0)
        s.start(initial(n, seed), f0, boundary=g0, dt=0.05, theta=0.5)
        s.step(f0, boundary=g0)
        assert _num_vectors(lib, s) == lib.hpgmg_vectors_reserved() + 3
        for before in ("theta", "pcg"):
            if before == "pcg":
                s.solve(f0, method="pcg", rtol=1e-6, boundary=g0)          # pcg's vectors are ids the march's three hold already
            info = s.wave_start(initial(n, seed), W.velocity0(n, seed), f0, boundary=g0, dt=dts[0], beta=rule[0], gamma=rule[1], damping=rule[2])
            assert _num_vectors(lib, s) == lib.hpgmg_vectors_reserved() + 4, before
            got = [(s.get_solution(), s.velocity(), s.acceleration(), info)]
            for k, dt in enumerate(dts, start=1):
                f, g = data(name, n, seed, k)
                info = s.wave_step(f, boundary=g, dt=dt, rtol=1e-8)
                got.append((s.get_solution(), s.velocity(), s.acceleration(), info))
            for k, ((u, v, q, info), ref) in enumerate(zip(got, fresh)):
                assert u.tobytes() == ref[1].tobytes() and v.tobytes() == ref[2].tobytes() and q.tobytes() == ref[3].tobytes(), (before, k)
                assert (info.residual, info.norm_f, info.mean_shift, info.vcycles, int(info.converged), info.t, info.kinetic, info.potential) == ref[4], (before, k)


@pytest.mark.parametrize("what", ["f", "g"])
def test_a_refused_step_leaves_the_march_intact(lib, what):
    name, n, seed, dts = "corners", 16, 800, [1e-2, 1e-2, 5e-3]
    rule = (0.25, 0.5, 0.7)
    plain = W.march(lib, n, 8, name, seed, rule, dts, 1e-8)
    again = W.march(lib, n, 8, name, seed, rule, dts, 1e-8)
    W.same_march(again, plain)                                               # the same call sequence twice gives the same bits
    spoiled = W.march(lib, n, 8, name, seed, rule, dts, 1e-8, spoil=(2, what))
    assert spoiled[2] == ("refused", H.USER_NOT_FINITE)
    del spoiled[2]
    W.same_march(spoiled, plain)
