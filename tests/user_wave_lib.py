"""What the tests of the Newmark march share (Solver.wave_start / wave_step / velocity / acceleration and the hooks hpgmg_wave_predict / _correct /
_init): NumPy restatements of the three passes over whole padded boxes and of their two sums in the CG passes' order
(pcg_lib.header_order_dot), the hook calls, the scalar recurrence of one oscillator, the rounding gates, and a march through the C entry points that
takes its arrays from the host or from device memory (user_step_lib.march's sibling).

A level of the hook tests is a plain one of VECTORS vectors under the 7pt-cheby-helm configuration; IDS names the vectors a pass touches.  Every ghost
and padding double of every vector is NaN: a result that read one is not finite, and an output whose ghost or padding changed shows as other bits.
"""
import ctypes

import numpy as np

import hpgmg_amd as H
import pcg_lib as P
from hpgmg_amd.problem import Solver
from reduction_lib import bits, cell_offsets, random_field
from user_step_lib import B, data, initial, problem

EPS = np.finfo(np.float64).eps
VECTORS = 16
IDS = {"u": H.VECTOR_U, "F": H.VECTOR_F, "r": H.VECTOR_TEMP, "uold": 12, "v": 13, "q": 14, "spare": 15}
ALPHA = H.VECTOR_ALPHA
RULES = [(0.25, 0.5, 0.0), (0.25, 0.5, 0.7), (0.3025, 0.6, 0.2)]       # (beta, gamma, sigma) of the propagation test
# dt, cu, cv, a, sigma, cq, cg of the hook tests: the coefficients of one step with dt = 0.03, beta = 0.3025, gamma = 0.6, sigma = 0.2
HOOK_DT, HOOK_BETA, HOOK_GAMMA, HOOK_SIGMA = 0.03, 0.3025, 0.6, 0.2
# The potential formula u ((F - r) - (a alpha) u) and the defect alpha q + sigma alpha v + apply(u, g) - a alpha u - f both cancel the a alpha u term: what
# is left carries a rounding that scales with user_step_lib.rounding_scale.  The constants are the largest |error| / scale seen on the CPU oracle over
# every configuration and step of tests/test_oracle_user_wave.py (the tests print theirs); the tests gate at ROUNDING_FACTOR times them.
ROUNDING_FACTOR = 10.0
DEFECT_MEASURED = 0.76           # | |defect|_inf - |r|_inf | / rounding_scale: the defect identity (0.522 ... 0.754 per configuration)
ENERGY_MEASURED = 0.0017         # |potential - h^3/2 u.(apply(u) - a alpha u)| / (vol |u|_inf rounding_scale / 2): the potential formula (0.0006 ... 0.0017;
                                 # the scale assumes every cell at |u|_inf with errors of one sign, hence the small constant)


def shift(dt, beta, gamma, sigma):
    return 1.0 / (beta * (dt * dt)) + (sigma * gamma) / (beta * dt)


def coefficients_of(dt, beta, gamma, sigma):
    """(cu, cv, a, cq, cg) in the library's written order (host/user_wave.inc)."""
    return (dt * dt) * (0.5 - beta), dt * (1.0 - gamma), shift(dt, beta, gamma, sigma), 1.0 / (beta * (dt * dt)), gamma * dt


def oscillator(mu, dt, beta, gamma, sigma, steps):
    """The scheme on s'' + sigma s' + mu s = 0 from s = 1, s' = 0: [(s_n, s'_n, s''_n)] for n = 0 .. steps."""
    cu, cv, a, cq, cg = coefficients_of(dt, beta, gamma, sigma)
    s, v = 1.0, 0.0
    q = -mu * s - sigma * v
    out = [(s, v, q)]
    for _ in range(steps):
        st, vt = s + dt * v + cu * q, v + cv * q
        s = (a * st - sigma * vt) / (a + mu)
        q = (s - st) * cq
        v = vt + cg * q
        out.append((s, v, q))
    return out


# ---------------------------------------------------------------------------------------------------------------------------- the hooks
def new_level(be, geom, periodic=False):
    lv = be.level(geom[0], geom[1], num_vectors=VECTORS, bc=H.BC_PERIODIC if periodic else H.BC_DIRICHLET)
    assert (lv.num_vectors, lv.num_boxes, lv.box_dim, lv.ghosts) == (VECTORS, geom[0] ** 3, geom[1], 1)
    return lv


def nan_outside(level, field):
    out = np.full_like(field, np.nan)
    q = cell_offsets(level)
    out[:, q] = field[:, q]
    return out


def fields_of(level, seed):
    """name -> field for IDS and "alpha": random interiors in [-1, 1), alpha in [0.5, 1.5), NaN in every ghost and padding double."""
    F = {name: nan_outside(level, random_field(level, seed + n)) for n, name in enumerate(sorted(IDS))}
    F["alpha"] = nan_outside(level, np.abs(random_field(level, seed + 99)) + 0.5)
    return F


def write_fields(lv, F, names=None):
    for name in (F if names is None else names):
        lv.write_all(ALPHA if name == "alpha" else IDS[name], F[name])


def _fn(lv, name, host):
    return getattr(lv.b.lib, name + ("_host" if host else ""))


def _sums():
    return (ctypes.c_double * 2)(np.nan, np.nan)


def call_predict(lv, dt, cu, cv, a, sigma, host=False, ids=None):
    i = dict(IDS, **(ids or {}))
    return _fn(lv, "hpgmg_wave_predict", host)(lv.ptr, i["u"], i["uold"], i["v"], i["F"], i["q"], dt, cu, cv, a, sigma)


def call_correct(lv, a, cq, cg, host=False, ids=None):
    i, s = dict(IDS, **(ids or {})), _sums()
    return _fn(lv, "hpgmg_wave_correct", host)(lv.ptr, i["q"], i["v"], i["u"], i["uold"], i["F"], i["r"], a, cq, cg, s), (s[0], s[1])


def call_init(lv, a, sigma, host=False, ids=None):
    i, s = dict(IDS, **(ids or {})), _sums()
    return _fn(lv, "hpgmg_wave_init", host)(lv.ptr, i["q"], i["r"], i["u"], i["v"], i["F"], a, sigma, s), (s[0], s[1])


def tree(level, terms, **wrong):
    """One tree of the CG passes' order over per-cell leaf terms (a box array): header_order_dot with the terms as products."""
    return P.header_order_dot(terms, np.ones_like(terms), level.box_dim, **wrong)       # t * 1.0 is t, bit for bit


def predict_restated(level, F, dt, cu, cv, a, sigma):
    """{name: field} of the four vectors wave_predict writes; one NumPy operation per operation of include/hpgmg_wave_math.h, in its association."""
    c = cell_offsets(level)
    u, v, q, Fv, al = (F[k][:, c] for k in ("u", "v", "q", "F", "alpha"))
    ut = (u + dt * v) + cu * q
    vt = v + cv * q
    out = {k: F[k].copy() for k in ("u", "uold", "v", "F")}
    out["F"][:, c] = Fv + al * (a * ut - sigma * vt)
    out["u"][:, c] = ut; out["uold"][:, c] = ut; out["v"][:, c] = vt
    return out


def energy_terms(u, v, Fv, r, al, a):
    return (al * v) * v, u * ((Fv - r) - (a * al) * u)


def correct_restated(level, F, a, cq, cg, **wrong):
    c = cell_offsets(level)
    u, uold, v, Fv, r, al = (F[k][:, c] for k in ("u", "uold", "v", "F", "r", "alpha"))
    q = (u - uold) * cq
    vn = v + cg * q
    out = {"q": F["q"].copy(), "v": F["v"].copy()}
    out["q"][:, c] = q; out["v"][:, c] = vn
    kin, pot = energy_terms(u, vn, Fv, r, al, a)
    return out, (tree(level, kin, **wrong), tree(level, pot, **wrong))


def init_restated(level, F, a, sigma, **wrong):
    c = cell_offsets(level)
    u, v, Fv, r, al = (F[k][:, c] for k in ("u", "v", "F", "r", "alpha"))
    out = {"q": F["q"].copy()}
    out["q"][:, c] = ((r + (a * al) * u) / al) - sigma * v
    kin, pot = energy_terms(u, v, Fv, r, al, a)
    return out, (tree(level, kin, **wrong), tree(level, pot, **wrong))


def same_bits(got, want, what):
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: other bits at {bad[:5].tolist()} ..."


def same_sums(got, want, what):
    assert P.same_scalar(got[0], want[0]) and P.same_scalar(got[1], want[1]), (what, got, want)


# ---------------------------------------------------------------------------------------------------------------------------- the march
def host_arrays():
    return (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST


def info_fields(info):
    return (info.norm_of_residual, info.norm_of_f, info.mean_shift, info.vcycles, info.converged, info.t, info.kinetic, info.potential)


def velocity0(n, seed):
    return np.random.default_rng(seed + 6).random((n, n, n)) * 2.0 - 1.0


def march(lib, n, box_dim, name, seed, rule, dts, rtol, device=None, spoil=None):
    """wave_start at time level 0, then one step per entry of `dts` (time level k = 1, 2, ...) through the C entry points; device = DeviceArrays: every
    array lives in device memory.  rule = (beta, gamma, sigma).  spoil = (k, "f" | "g"): before step k a step with a NaN in that array is tried, and its
    status recorded.  Returns [(status, u, v, q, info fields)] for the start and every step, with ("refused", status) entries where a spoiled step was
    tried."""
    bc, coef, kappa = problem(name, n, seed)
    put, w = host_arrays() if device is None else (device.put, H.WHERE_PLUGIN)
    beta, gamma, sigma = rule
    out = []

    def fetch(s, call):
        if device is None:
            a = np.full((n, n, n), 7.0)
            assert call(s._ptr, a.ctypes.data, w) == H.USER_OK
            return a
        p = device.put(np.full((n, n, n), 7.0))
        assert call(s._ptr, p, w) == H.USER_OK
        return device.get(p, (n, n, n))

    def state(s, st, info):
        return (st, fetch(s, lib.hpgmg_user_get_solution), fetch(s, lib.hpgmg_user_get_velocity), fetch(s, lib.hpgmg_user_get_acceleration), info_fields(info))

    with Solver(n, box_dim=box_dim, bc=bc, a=1.0, b=B, lib=lib) as s:
        alpha, bi, bj, bk = coef
        if kappa is None:
            assert lib.hpgmg_user_set_coefficients(s._ptr, put(alpha), put(bi), put(bj), put(bk), w) == H.USER_OK
        else:
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, put(alpha), put(bi), put(bj), put(bk), put(kappa), w) == H.USER_OK
        (f, g), u0, v0 = data(name, n, seed, 0), initial(n, seed), velocity0(n, seed)          # named: a host pointer must outlive the call
        info = H.UserWaveInfo()
        st = lib.hpgmg_user_wave_start(s._ptr, put(u0), put(v0), put(f), put(g), w, dts[0], beta, gamma, sigma, ctypes.byref(info))
        assert st == H.USER_OK
        out.append(state(s, st, info))
        for k, dt in enumerate(dts, start=1):
            f, g = data(name, n, seed, k)
            info = H.UserWaveInfo()
            if spoil is not None and spoil[0] == k:
                bad_f, bad_g = f.copy(), None if g is None else g.copy()
                if spoil[1] == "f":
                    bad_f[n - 1, 0, n // 2] = np.nan
                else:
                    bad_g[3, n - 1, 1] = np.nan
                out.append(("refused", lib.hpgmg_user_wave_step(s._ptr, put(bad_f), put(bad_g), w, dt, rtol, ctypes.byref(info))))
            pf, pg = put(f), put(g)
            st = lib.hpgmg_user_wave_step(s._ptr, pf, pg, w, dt if k == 1 or dt != dts[k - 2] else 0.0, rtol, ctypes.byref(info))
            out.append(state(s, st, info))
            if device is not None:
                device.free()
    return out


def same_march(got, ref):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        if r[0] == "refused":
            assert g == r, k
            continue
        assert g[0] == r[0] == H.USER_OK, k
        for what, x, y in zip("uvq", g[1:4], r[1:4]):
            assert x.tobytes() == y.tobytes(), f"{what} after step {k}"
        assert g[4] == r[4], (k, g[4], r[4])
