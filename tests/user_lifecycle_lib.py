"""Helpers of the lifecycle tests of the dense-array Solver (hpgmg_amd/problem.py): one solver kept alive through new coefficients, right-hand
sides, boundary data, warm starts and methods, against a fresh solver per step.

A spec is (n, box_dim, bc, smoother, a).  A sequence is a list of steps:
    ("coef", (alpha, beta_i, beta_j, beta_k)[, robin])      set_coefficients
    ("solve", f, method, kwargs)                            kwargs: rtol, max_iter, u0, boundary
    ("apply", x, g)                                         g: boundary data or None
    ("flux", u, g)
    ("close_reopen",)                                       close the solver and create one of the same spec (a "coef" step follows)
    ("start", u0, f, g, dt, theta)                          begin a time march; g: boundary data or None
    ("step", f, g, dt, theta, rtol)                         one step of it; dt, theta None: as before.  Outputs u, the rate array w, the info, rate
    ("shift", a)                                            set_shift
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


def new_solver(lib, spec, a=None):
    """a: another a than the spec's (a fresh solver for one that marched or had set_shift)"""
    n, box_dim, bc, smoother, a0 = spec
    return Solver(n, box_dim=box_dim, bc=bc, smoother=smoother, a=a0 if a is None else a, b=1.0, lib=lib)


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

    def __init__(self, lib, spec, entry="host", device=None, a=None):
        assert entry in ("host", "device") and (entry == "host" or device is not None)
        self.lib, self.spec, self.entry = lib, spec, entry
        self.buf = _DeviceBuffers(device) if entry == "device" else None
        self.s = new_solver(lib, spec, a)

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

    def _start_host(self, u0, f, g, dt, theta):
        self.s.start(u0, f, boundary=g, dt=dt, theta=theta)
        return {}

    def _step_host(self, f, g, dt, theta, rtol):
        info = self.s.step(f, boundary=g, dt=dt, theta=theta, rtol=rtol)
        return dict(u=self.s.get_solution(), w=self.s.rate(), rate=info.rate, **{k: getattr(info, k) for k in INFO})

    def _shift_host(self, a):
        self.s.set_shift(a)
        return {}

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

    def _start_device(self, u0, f, g, dt, theta):
        p = [self.buf.put(name, v) for name, v in (("u0", u0), ("f", f), ("g", g))]
        assert self.lib.hpgmg_user_start(self.s._ptr, *p, H.WHERE_PLUGIN, dt, theta) == 0
        return {}

    def _step_device(self, f, g, dt, theta, rtol):
        lib, S, w = self.lib, self.s._ptr, H.WHERE_PLUGIN
        info, rate = H.UserInfo(), ctypes.c_double(-1.0)
        assert lib.hpgmg_user_step(S, self.buf.put("f", f), self.buf.put("g", g), w, dt or 0.0, theta or 0.0, rtol, ctypes.byref(info),
                                   ctypes.byref(rate)) == 0                      # 0: as before
        assert lib.hpgmg_user_get_solution(S, self.buf.out("u", f.nbytes), w) == 0
        assert lib.hpgmg_user_get_rate(S, self.buf.out("w", f.nbytes), w) == 0
        return dict(u=self.buf.get("u", f.shape), w=self.buf.get("w", f.shape), rate=rate.value, residual=info.norm_of_residual,
                    norm_f=info.norm_of_f, vcycles=info.vcycles, converged=bool(info.converged), mean_shift=info.mean_shift)

    def _shift_device(self, a):
        assert self.lib.hpgmg_user_set_shift(self.s._ptr, a) == 0
        return {}


def run(lib, spec, steps, entry="host", device=None, before=None, after=None, a=None):
    """Plays `steps` on one Solver; returns every step's outputs (a dict of arrays and of the SolveInfo fields; {} for a step without any).
    before(i, step) / after(i, step, out): called around step i (switches, counters).  a: the solver is created with this a, not the spec's."""
    p = Player(lib, spec, entry, device, a)
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


def shift_before(spec, steps, i):
    """The a of the live solver when step i begins: the spec's, then whatever the last start / step with a dt / shift made it."""
    a, dt, theta = spec[4], None, None
    for step in steps[:i]:
        if step[0] == "close_reopen":
            a = spec[4]
        elif step[0] == "shift":
            a = step[1]
        elif step[0] in ("start", "step"):
            new_dt, new_theta = (step[4], step[5]) if step[0] == "start" else (step[3], step[4])
            dt, theta = new_dt or dt, new_theta or theta
            a = 1.0 / (theta * dt)
    return a


def fresh(lib, spec, steps, i, entry="host", device=None):
    """Step i alone on a new solver that has only seen the last "coef" step before it (the same arrays, u0 included) and the live solver's
    current a.  A "step" of a march: the new solver has also seen the last "start" and the march's steps since, and nothing between them (a
    march restarted from a fetched state agrees to rounding only, DESIGN.md §11.8: so it is replayed from its start)."""
    coef = [s for s in steps[:i] if s[0] == "coef"][-1]
    if steps[i][0] == "step":
        first = max(j for j in range(i) if steps[j][0] == "start")
        assert not any(s[0] in ("coef", "solve", "close_reopen", "shift") for s in steps[first:i]), "the march of step i ended before it"
        replay = [coef, steps[first]] + [s for s in steps[first + 1:i + 1] if s[0] == "step"]
        return run(lib, spec, replay, entry, device)[-1]
    return run(lib, spec, [coef, steps[i]], entry, device, a=shift_before(spec, steps, i))[1]


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


MARCH_DT, MARCH_THETA, MARCH_RTOL = 2e-3, 0.5, 1e-6
_MARCH = {}


def march_sequence(spec):
    """The sequence with time marches, for a spec with a != 0 (1-based, as DESIGN.md §11.7 counts): 3 is the solver's FIRST start, after a solve
    has run -- the finest level gets two more vectors, so new storage (create_vectors); 5 and 6 use the operator and its scratch vectors in the
    middle of a march; 8 changes dt; 9 ends the march and may take its two vectors; 12 and 16 put new coefficients under a solver that
    marched; 19 and 20 are set_shift and a solve on it.  Every array is random and independent of any output, so nothing has to be played to
    build it.  Cached per spec; the arrays are never written to."""
    key = spec_id(spec)
    if key in _MARCH:
        return _MARCH[key]
    assert spec[4] != 0.0
    n = spec[0]
    rng = np.random.default_rng(6000 + n)
    walls = shape_bc(spec) == "dirichlet"

    def cells(lo=-1.0, hi=1.0):
        return lo + (hi - lo) * rng.random((n, n, n))

    def g():
        return rng.random((6, n, n)) * 4.0 - 2.0 if walls else None

    def coef(seed):
        return ("coef", coefficients(spec, seed)) + ((kappa(spec, seed + 1),) if has_robin(spec) else ())

    def start():
        return ("start", cells(), cells(-2.0, 2.0), g(), MARCH_DT, MARCH_THETA)

    def step(dt=None):
        return ("step", cells(-2.0, 2.0), g(), dt, None, MARCH_RTOL)

    f1 = cells(-0.3, 0.7)
    steps = [coef(7000 + n), ("solve", f1, "fmg", {"boundary": g()}),
             start(), step(), ("apply", cells(), g()), ("flux", cells(), g()), step(), step(MARCH_DT / 4.0),
             ("solve", f1, "pcg", {"rtol": 1e-8, "max_iter": 2}),
             start(), step(),
             coef(8000 + n), start(), step(),
             ("close_reopen",), coef(9000 + n), start(), step(),
             ("shift", 2.5), ("solve", f1, "fmg", {"boundary": g()})]
    assert [s[0] for s in steps] == ["coef", "solve", "start", "step", "apply", "flux", "step", "step", "solve", "start", "step", "coef", "start",
                                     "step", "close_reopen", "coef", "start", "step", "shift", "solve"]
    for s in steps:
        for v in s[1:]:
            for arr in (v if isinstance(v, tuple) else v.values() if isinstance(v, dict) else (v,)):
                if isinstance(arr, np.ndarray):
                    arr.setflags(write=False)
    _MARCH[key] = steps
    return steps


def issued_thrice(steps):
    """(steps with every solve issued three times in a row and every march step followed by two more of the same data, for each the index of the
    step it came from).  With graphs on, the three issues of a solve are eager, captured and replayed; the repeated steps of a march are further
    time steps, and only a run of the same expanded sequence is their reference."""
    out, of = [], []
    for i, step in enumerate(steps):
        for _ in range(3 if step[0] in ("solve", "step") else 1):
            out.append(step)
            of.append(i)
    return out, of


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
