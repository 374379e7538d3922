"""Helpers of the lifecycle tests of the dense-array Solver (hpgmg_amd/problem.py): one solver kept alive through new coefficients, right-hand
sides, boundary data, warm starts and methods, against a fresh solver per step.

A spec is (n, box_dim, bc, smoother, a).  A sequence is a list of steps:
    ("coef", (alpha, beta_i, beta_j, beta_k)[, robin])      set_coefficients
    ("solve", f, method, kwargs)                            kwargs: rtol, max_iter, u0, boundary
    ("apply", x, g)                                         g: boundary data or None
    ("flux", u, g)
    ("close_reopen",)                                       close the solver and create one of the same spec (a "coef" step follows)
Every array of a step is a concrete NumPy array, so a step means the same on any library and on a fresh solver.  Only bits are compared, so the
coefficients are plain rng.random fields (beta in [0.5, 3], alpha in [0.5, 1.5]): nothing here needs a solve to converge.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver, _METHOD
from user_problem_lib import face_shape

WALLS = ("convective", "dirichlet", "neumann", "convective", "dirichlet", "convective")
SPECS = [  # n, box_dim, bc, smoother, a
    (32, 16, "dirichlet", "cheby", 1.0),
    (48, 16, "periodic", "gsrb", 0.0),
    (32, 16, WALLS, "cheby", 0.0),
    (48, 16, ("neumann",) * 6, "jacobi", 0.0),      # the singular path: mean_shift is compared
]
PAIR = [(32, 16, "dirichlet", "cheby", 1.0), (48, 16, WALLS, "cheby", 1.0)]      # two live solvers share one smoother and one a != 0
INFO = ("residual", "norm_f", "vcycles", "converged", "mean_shift")


def spec_id(spec):
    n, box_dim, bc, smoother, a = spec
    kind = bc if isinstance(bc, str) else "neumann" if set(bc) == {"neumann"} else "walls"
    return f"{n}-{box_dim}-{kind}-{smoother}-a{a:g}"


def shape_bc(spec):
    """The boundary condition that decides the shapes of the beta arrays."""
    return spec[2] if isinstance(spec[2], str) else "dirichlet"


def has_robin(spec):
    return not isinstance(spec[2], str) and "convective" in spec[2]


def coefficients(spec, seed):
    n, a = spec[0], spec[4]
    rng = np.random.default_rng(seed)
    alpha = 0.5 + rng.random((n, n, n)) if a != 0.0 else None
    return (alpha,) + tuple(0.5 + 2.5 * rng.random(face_shape(n, shape_bc(spec), axis)) for axis in range(3))


def kappa(spec, seed):
    n = spec[0]
    return np.random.default_rng(seed).random((6, n, n)) * 2.0


def doubled(coef):
    """The same coefficients with every beta doubled (exactly: a power of two)."""
    return (coef[0],) + tuple(2.0 * c for c in coef[1:])


def new_solver(lib, spec):
    n, box_dim, bc, smoother, a = spec
    return Solver(n, box_dim=box_dim, bc=bc, smoother=smoother, a=a, b=1.0, lib=lib)


class _DeviceBuffers:
    """ONE device buffer per argument name, overwritten in place between steps: a library that kept a caller's pointer instead of its content
    would read the next step's data.  D is a DeviceArrays of test_gpu_user_problem.py."""

    def __init__(self, D):
        self.D, self.ptr = D, {}

    def put(self, name, a):
        if a is None:
            return None
        if name not in self.ptr:
            self.ptr[name] = self.D.empty(a.nbytes)
        assert self.D.K.hpgmg_hip_memcpy_h2d(self.ptr[name], a.ctypes.data, a.nbytes) == 0
        return self.ptr[name]

    def out(self, name, nbytes):
        if name not in self.ptr:
            self.ptr[name] = self.D.empty(nbytes)
        return self.ptr[name]

    def get(self, name, shape):
        return self.D.get(self.ptr[name], shape)


class Player:
    """One live Solver that plays steps.  entry "host": NumPy arrays through the Solver's methods; "device": device memory through the C entry
    points (device = a DeviceArrays)."""

    def __init__(self, lib, spec, entry="host", device=None):
        assert entry in ("host", "device") and (entry == "host" or device is not None)
        self.lib, self.spec, self.entry = lib, spec, entry
        self.buf = _DeviceBuffers(device) if entry == "device" else None
        self.s = new_solver(lib, spec)

    def close(self):
        self.s.close()

    def play(self, step):
        kind = step[0]
        if kind == "close_reopen":
            self.s.close()
            self.s = new_solver(self.lib, self.spec)
            return {}
        return getattr(self, "_" + kind + "_" + self.entry)(*step[1:])

    # ---- host: the Python API
    def _coef_host(self, coef, robin=None):
        self.s.set_coefficients(*coef, **({"robin": robin} if robin is not None else {}))
        return {}

    def _solve_host(self, f, method, kwargs):
        u, info = self.s.solve(f, method=method, **kwargs)
        return dict(u=u, **{k: getattr(info, k) for k in INFO})

    def _apply_host(self, x, g):
        return {"y": self.s.apply(x, boundary=g)}

    def _flux_host(self, u, g):
        return dict(zip(("qi", "qj", "qk"), self.s.flux(u, boundary=g)))

    # ---- device: the C entry points on device memory
    def _coef_device(self, coef, robin=None):
        p = [self.buf.put(name, c) for name, c in zip(("alpha", "beta_i", "beta_j", "beta_k"), coef)]
        if robin is None:
            assert self.lib.hpgmg_user_set_coefficients(self.s._ptr, *p, H.WHERE_PLUGIN) == 0
        else:
            assert self.lib.hpgmg_user_set_coefficients_robin(self.s._ptr, *p, self.buf.put("kappa", robin), H.WHERE_PLUGIN) == 0
        return {}

    def _solve_device(self, f, method, kwargs):
        lib, S, w = self.lib, self.s._ptr, H.WHERE_PLUGIN
        info, shift = H.UserInfo(), ctypes.c_double()
        g, u0, rtol = kwargs.get("boundary"), kwargs.get("u0"), kwargs.get("rtol", 1e-10)
        if g is None:
            assert lib.hpgmg_user_set_rhs(S, self.buf.put("f", f), w, ctypes.byref(shift)) == 0
        else:
            assert lib.hpgmg_user_set_rhs_dirichlet(S, self.buf.put("f", f), self.buf.put("g", g), w, ctypes.byref(shift)) == 0
        if method in ("pcg", "fpcg"):
            assert lib.hpgmg_user_set_max_iterations(S, kwargs.get("max_iter", 100)) == 0
        assert lib.hpgmg_user_solve(S, _METHOD[method], rtol, self.buf.put("u0", u0), w, ctypes.byref(info)) == 0
        assert lib.hpgmg_user_get_solution(S, self.buf.out("u", f.nbytes), w) == 0
        return dict(u=self.buf.get("u", f.shape), residual=info.norm_of_residual, norm_f=info.norm_of_f, vcycles=info.vcycles,
                    converged=bool(info.converged), mean_shift=info.mean_shift)

    def _apply_device(self, x, g):
        lib, S, w = self.lib, self.s._ptr, H.WHERE_PLUGIN
        px, py = self.buf.put("x", x), self.buf.out("y", x.nbytes)
        if g is None:
            assert lib.hpgmg_user_apply(S, px, py, w) == 0
        else:
            assert lib.hpgmg_user_apply_dirichlet(S, px, self.buf.put("g", g), py, w) == 0
        return {"y": self.buf.get("y", x.shape)}

    def _flux_device(self, u, g):
        n, bc = self.spec[0], shape_bc(self.spec)
        shapes = [face_shape(n, bc, axis) for axis in range(3)]
        po = [self.buf.out(name, 8 * int(np.prod(shape))) for name, shape in zip(("qi", "qj", "qk"), shapes)]
        assert self.lib.hpgmg_user_flux(self.s._ptr, self.buf.put("x", u), self.buf.put("g", g), *po, H.WHERE_PLUGIN) == 0
        return {name: self.buf.get(name, shape) for name, shape in zip(("qi", "qj", "qk"), shapes)}


def run(lib, spec, steps, entry="host", device=None, before=None, after=None):
    """Plays `steps` on one Solver; returns every step's outputs (a dict of arrays and of the SolveInfo fields; {} for a step without any).
    before(i, step) / after(i, step, out): called around step i (switches, counters)."""
    p = Player(lib, spec, entry, device)
    outs = []
    try:
        for i, step in enumerate(steps):
            if before:
                before(i, step)
            outs.append(p.play(step))
            if after:
                after(i, step, outs[-1])
    finally:
        p.close()
    return outs


def fresh(lib, spec, steps, i, entry="host", device=None):
    """Step i alone on a new solver that has only seen the last "coef" step before it (the same arrays, u0 included)."""
    coef = [s for s in steps[:i] if s[0] == "coef"][-1]
    return run(lib, spec, [coef, steps[i]], entry, device)[1]


def differences(got, ref):
    """Names of the outputs of one step that are not the same bits."""
    assert got.keys() == ref.keys()
    bad = []
    for k, v in ref.items():
        if isinstance(v, np.ndarray):
            if got[k].shape != v.shape or got[k].tobytes() != v.tobytes():
                bad.append(k)
        elif not (got[k] == v or (v != v and got[k] != got[k])):
            bad.append(k)
    return bad


def assert_same(got, ref, what=""):
    """Two runs of the same steps, step by step and bit by bit."""
    assert len(got) == len(ref)
    bad = [(i, differences(g, r)) for i, (g, r) in enumerate(zip(got, ref)) if differences(g, r)]
    assert not bad, f"{what}: (step, outputs) that differ: {bad}"


_SEQ = {}


def sequence(lib, spec):
    """The standard sequence SEQ of the spec.  The warm start of step 8 and the flux of step 4 take a u of an earlier step: `lib` (the CPU
    oracle) plays the steps before them once, so that the sequence holds arrays only.  Cached per spec; the arrays are never written to.

    On a domain with walls the fmg / mg / apply / flux steps pass boundary data, in turn g1, None, g2, ...: the F-cycle's hook, and with it the
    key of its segments, comes and goes between solves.  With a Robin wall step 5 changes kappa only."""
    key = spec_id(spec)
    if key in _SEQ:
        return _SEQ[key]
    n = spec[0]
    rng = np.random.default_rng(1000 + n)
    f1, f2, x, noise = (rng.random((n, n, n)) - 0.3, rng.random((n, n, n)) - 0.6, rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) - 0.5)
    walls = shape_bc(spec) == "dirichlet"
    cycle = [rng.random((6, n, n)) * 4.0 - 2.0, None, rng.random((6, n, n)) * 2.0 - 1.0] if walls else [None]
    turn = [0]

    def g():
        turn[0] += 1
        return cycle[(turn[0] - 1) % len(cycle)]

    c1, c2 = coefficients(spec, 2000 + n), coefficients(spec, 3000 + n)
    if has_robin(spec):
        coef1, coef5 = ("coef", c1, kappa(spec, 4000 + n)), ("coef", c1, kappa(spec, 5000 + n))
    else:
        coef1, coef5 = ("coef", c1), ("coef", c2)
    steps = [coef1, ("solve", f1, "fmg", {"boundary": g()}), ("apply", x, g())]
    u2 = run(lib, spec, steps)[1]["u"]
    steps += [("flux", u2, g()), coef5, ("solve", f1, "fmg", {"boundary": g()}), ("solve", f2, "mg", {"rtol": 1e-8, "boundary": g()})]
    u7 = run(lib, spec, [coef5, steps[6]])[1]["u"]
    steps += [("solve", f2, "mg", {"rtol": 1e-8, "boundary": g(), "u0": u7 + 1e-3 * noise}),
              ("solve", f1, "pcg", {"rtol": 1e-8, "max_iter": 6}),            # grows every level by three vectors
              ("solve", f1, "fpcg", {"rtol": 1e-8, "max_iter": 6}),
              ("solve", f1, "fmg", {"boundary": steps[5][3]["boundary"]})]    # step 6 again
    for step in steps:
        for v in step[1:]:
            for arr in (v if isinstance(v, tuple) else v.values() if isinstance(v, dict) else (v,)):
                if isinstance(arr, np.ndarray):
                    arr.setflags(write=False)
    _SEQ[key] = steps
    return steps


def interleave(lib, specs, sequences, entry="host", devices=None):
    """Two (or more) live solvers whose steps alternate: step 0 of each, then step 1 of each, ...  Returns one list of outputs per solver."""
    players = []
    outs = [[] for _ in specs]
    try:
        for k, spec in enumerate(specs):
            players.append(Player(lib, spec, entry, devices[k] if devices else None))
        for i in range(max(len(s) for s in sequences)):
            for k, steps in enumerate(sequences):
                if i < len(steps):
                    outs[k].append(players[k].play(steps[i]))
    finally:
        for p in players:
            p.close()
    return outs


def refused_then_recovered(lib, spec, entry="host", device=None):
    """set_coefficients with one NaN in beta_k is refused and leaves solve raising; valid coefficients after it give a fresh solver's bits.
    Returns (recovered output, fresh output)."""
    n = spec[0]
    f = np.random.default_rng(77).random((n, n, n)) - 0.3
    c1, c2 = coefficients(spec, 78), coefficients(spec, 79)
    bad = c2[:3] + (c2[3].copy(),)
    bad[3][n // 2, 3, n - 1] = np.nan
    solve = ("solve", f, "fmg", {})
    p = Player(lib, spec, entry, device)
    try:
        p.play(("coef", c1))
        p.play(solve)
        with pytest.raises(ValueError, match="beta_k: holds a value that is not finite"):
            p.s.set_coefficients(*bad)
        with pytest.raises(ValueError, match="no valid coefficients"):
            p.s.solve(f)
        p.play(("coef", c2))
        got = p.play(solve)
    finally:
        p.close()
    return got, fresh(lib, spec, [("coef", c2), solve], 1)
