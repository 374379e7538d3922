"""Face fluxes of a solution on the MI355X: the HIP build (kernels/dense_flux.hip, one launch for the three arrays) equals
the CPU oracle bit for bit, with arrays entering from the host (through the staging buffer) and from the device (in place); kappa = 0 gives the
Neumann solver's bytes; a non-finite boundary value on the device is reported; the solution is untouched; torch tensors equal the NumPy path.

Shapes: N = 64 in boxes of 32 (2^3 boxes: every box touches three walls) and N = 48 in boxes of 16 (3^3 boxes: boxes on zero, one, two and
three walls; box-to-box faces in the middle of the domain and, periodic, the wrap).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays
from user_flux_lib import SOLVERS, boundary_for, kappa_for
from user_problem_lib import face_shape, random_coefficients
from user_robin_lib import ALL, CORNERS, neumann_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _inputs(name, n, a, seed):
    bc = "periodic" if name == "periodic" else "dirichlet"
    coef = random_coefficients(n, bc, a != 0.0, seed=seed)
    u = np.random.default_rng(seed + 1).random((n, n, n)) * 2.0 - 1.0
    return bc, coef, u, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _flux(lib, n, box_dim, faces, a, coef, kappa, u, g, device=None):
    """The three arrays and the status through hpgmg_user_flux; device = DeviceArrays: every array lives in device memory."""
    bc = "periodic" if faces == "periodic" else "dirichlet"
    shapes = [face_shape(n, bc, axis) for axis in range(3)]
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=0.7, lib=lib) as s:
        if device is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = [np.full(shape, 7.0) for shape in shapes]
            ptr = [q.ctypes.data for q in outs]
        else:
            put, w = device.put, H.WHERE_PLUGIN
            ptr = [device.put(np.full(shape, 7.0)) for shape in shapes]
        alpha, bi, bj, bk = coef
        if kappa is None:
            assert lib.hpgmg_user_set_coefficients(s._ptr, put(alpha), put(bi), put(bj), put(bk), w) == 0
        else:
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, put(alpha), put(bi), put(bj), put(bk), put(kappa), w) == 0
        st = lib.hpgmg_user_flux(s._ptr, put(u), put(g), ptr[0], ptr[1], ptr[2], w)
        if device is not None:
            outs = [device.get(p, shape) for p, shape in zip(ptr, shapes)]
    return st, outs


CASES = [  # n, box_dim, solver, a, entry
    (64, 32, "dirichlet", 1.0, "host"),
    (64, 32, "dirichlet", 0.0, "device"),
    (48, 16, "dirichlet", 0.0, "host"),
    (64, 32, "periodic", 0.0, "host"),
    (48, 16, "periodic", 1.0, "device"),
    (64, 32, "corners", 1.0, "device"),
    (48, 16, "corners", 0.0, "host"),
    (64, 32, "robin", 0.0, "host"),
    (48, 16, "robin", 1.0, "device"),
    (64, 32, "neumann", 0.0, "device"),
    (48, 16, "neumann", 1.0, "host"),
]


@pytest.mark.parametrize("n,box_dim,name,a,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, name, a, entry):
    hip, oracle, K = libs
    _, coef, u, g, kappa = _inputs(name, n, a, 1000 + n + int(a))
    st_ref, ref = _flux(oracle, n, box_dim, SOLVERS[name], a, coef, kappa, u, g)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        st, got = _flux(hip, n, box_dim, SOLVERS[name], a, coef, kappa, u, g, device=D)
        st0, got0 = _flux(hip, n, box_dim, SOLVERS[name], a, coef, kappa, u, None, device=D)      # zero data: no boundary array at all
    finally:
        if D:
            D.free()
    assert st == st_ref == H.USER_OK and st0 == H.USER_OK
    for axis in range(3):
        assert got[axis].tobytes() == ref[axis].tobytes(), axis
        assert np.isfinite(got0[axis]).all() and not (got0[axis] == 7.0).any()                      # every entry was written
    if g is not None:
        st_z, zero = _flux(oracle, n, box_dim, SOLVERS[name], a, coef, kappa, u, np.zeros_like(g))
        assert st_z == H.USER_OK and [q.tobytes() for q in got0] == [q.tobytes() for q in zero]


@pytest.mark.parametrize("walls,a", [(CORNERS, 1.0), (ALL, 0.0)])
def test_kappa_zero_gives_the_neumann_solvers_bytes(libs, walls, a):
    hip, _, K = libs
    n, box_dim = 48, 16
    _, coef, u, g, _ = _inputs("corners", n, a, 1100 + int(a))
    D = DeviceArrays(K)
    try:
        st_ref, ref = _flux(hip, n, box_dim, neumann_of(walls), a, coef, None, u, g, device=D)
        st, got = _flux(hip, n, box_dim, walls, a, coef, np.zeros((6, n, n)), u, g, device=D)
    finally:
        D.free()
    assert st == st_ref == H.USER_OK
    assert [q.tobytes() for q in got] == [q.tobytes() for q in ref]


def test_bad_values_are_reported_from_the_device(libs):
    hip, _, K = libs
    n = 48
    _, coef, u, g, kappa = _inputs("corners", n, 0.0, 1200)
    D = DeviceArrays(K)
    try:
        for face in range(6):
            bad = g.copy()
            bad[face, n - 1, n - 1] = np.nan if face & 1 else np.inf
            assert _flux(hip, n, 16, CORNERS, 0.0, coef, kappa, u, bad, device=D)[0] == H.USER_NOT_FINITE, face
            assert _flux(hip, n, 16, CORNERS, 0.0, coef, kappa, u, bad)[0] == H.USER_NOT_FINITE, face
            D.free()
        bad_u = u.copy()
        bad_u[n - 1, 0, n // 2] = np.nan
        assert _flux(hip, n, 16, CORNERS, 0.0, coef, kappa, bad_u, g, device=D)[0] == H.USER_NOT_FINITE
    finally:
        D.free()


@pytest.mark.parametrize("name", ["dirichlet", "robin"])
def test_the_solution_is_unchanged_after_flux(libs, name):
    hip, oracle, _ = libs
    n = 48
    _, coef, x, g, kappa = _inputs(name, n, 1.0, 1300)
    f = np.random.default_rng(13).random((n, n, n)) - 0.5
    seen = []
    for lib in (hip, oracle):
        with Solver(n, box_dim=16, bc=SOLVERS[name], a=1.0, lib=lib) as s:
            s.set_coefficients(*coef, robin=kappa)
            u, _ = s.solve(f, boundary=g)
            q = s.flux(x, boundary=-g)
            assert s.get_solution().tobytes() == u.tobytes()
            seen.append([u] + list(q) + list(s.flux(u, boundary=g)) + [s.wall_flux(q)])
    for got, ref in zip(*seen):
        assert got.tobytes() == ref.tobytes()


def test_torch_tensors(libs):
    """A child process that imports torch first: flux and wall_flux on tensors equal the NumPy path bitwise, and mixed kinds are refused."""
    worker = os.path.join(ROOT, "tests", "user_flux_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
