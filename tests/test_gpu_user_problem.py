"""The user-problem API on the MI355X: the HIP build equals the CPU oracle bit for bit, the benchmark's 256^3 problem goes through the API
onto the fused kernels and gives the benchmark's u, torch tensors work in place, and the pack / unpack kernels round-trip and validate at 256^3.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend, load_golden
from user_problem_lib import benchmark_arrays, face_shape, random_coefficients

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    return hip, Backend.oracle().lib, K


class DeviceArrays:
    """Device copies of host arrays through the kernel library (no torch in this process)."""

    def __init__(self, K):
        self.K, self.ptrs = K, []

    def put(self, a):
        if a is None:
            return None
        p = self.K.hpgmg_hip_malloc(a.nbytes)
        assert p
        assert self.K.hpgmg_hip_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        self.ptrs.append(p)
        return p

    def empty(self, nbytes):
        p = self.K.hpgmg_hip_malloc(nbytes)
        assert p
        self.ptrs.append(p)
        return p

    def get(self, p, shape):
        out = np.empty(shape)
        assert self.K.hpgmg_hip_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        for p in self.ptrs:
            self.K.hpgmg_hip_free(p)
        self.ptrs = []


def _run_api(lib, n, box_dim, bc, smoother, a, coef, f, x, method, device=None):
    """u, A x and the info through the C entry points; device = DeviceArrays: the arrays live in device memory."""
    alpha, bi, bj, bk = coef
    s = Solver(n, box_dim=box_dim, bc=bc, smoother=smoother, a=a, b=1.0, lib=lib)
    try:
        info = H.UserInfo()
        shift = ctypes.c_double()
        if device is None:
            s.set_coefficients(alpha, bi, bj, bk)
            u, got = s.solve(f, method=method, rtol=1e-10)
            y = s.apply(x)
            return u, y, (got.residual, got.vcycles)
        D = device
        ptrs = [D.put(alpha), D.put(bi), D.put(bj), D.put(bk)]
        assert lib.hpgmg_user_set_coefficients(s._ptr, *ptrs, H.WHERE_PLUGIN) == 0
        assert lib.hpgmg_user_set_rhs(s._ptr, D.put(f), H.WHERE_PLUGIN, ctypes.byref(shift)) == 0
        assert lib.hpgmg_user_solve(s._ptr, H.USER_FMG if method == "fmg" else H.USER_MG, 1e-10, None, H.WHERE_PLUGIN, ctypes.byref(info)) == 0
        du, dy = D.empty(f.nbytes), D.empty(f.nbytes)
        assert lib.hpgmg_user_get_solution(s._ptr, du, H.WHERE_PLUGIN) == 0
        assert lib.hpgmg_user_apply(s._ptr, D.put(x), dy, H.WHERE_PLUGIN) == 0
        return D.get(du, f.shape), D.get(dy, f.shape), (info.norm_of_residual, info.vcycles)
    finally:
        s.close()


CASES = [  # n, box_dim, bc, smoother, a, method, entry
    (64, 32, "dirichlet", "cheby", 0.0, "fmg", "host"),
    (64, 32, "dirichlet", "cheby", 1.0, "mg", "device"),
    (64, 32, "periodic", "cheby", 0.0, "mg", "host"),
    (64, 32, "dirichlet", "gsrb", 1.0, "fmg", "device"),
    (64, 32, "periodic", "jacobi", 0.0, "fmg", "device"),
    (48, 16, "dirichlet", "jacobi", 1.0, "mg", "host"),
    (48, 16, "periodic", "gsrb", 0.0, "mg", "device"),
    (48, 16, "periodic", "cheby", 1.0, "fmg", "host"),
]


@pytest.mark.parametrize("n,box_dim,bc,smoother,a,method,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, bc, smoother, a, method, entry):
    hip, oracle, K = libs
    coef = random_coefficients(n, bc, a != 0.0, seed=n + len(smoother) + int(a))
    rng = np.random.default_rng(n)
    f, x = rng.random((n, n, n)) - 0.3, rng.random((n, n, n)) * 2.0 - 1.0
    ref = _run_api(oracle, n, box_dim, bc, smoother, a, coef, f, x, method)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = _run_api(hip, n, box_dim, bc, smoother, a, coef, f, x, method, device=D)
    finally:
        if D:
            D.free()
    assert np.array_equal(got[1], ref[1]), "apply differs"
    assert np.array_equal(got[0], ref[0]), "u differs"
    assert got[2] == ref[2]


def _counters(hip, K):
    hip.hpgmg_brick_visits.restype = ctypes.c_longlong
    pairs = (ctypes.c_longlong * 2)()
    K.hpgmg_hip_pair_launch_counts(pairs)
    return hip.hpgmg_brick_visits(), pairs[0]


@pytest.mark.parametrize("log2,per_rank,helmholtz", [(7, 8, 1), (7, 1, 0)])
def test_benchmark_problem_at_full_size_on_the_fast_path(libs, log2, per_rank, helmholtz):
    """config 2 (hpgmg-fv --helmholtz 7 8, 256^3) and one 128^3 Poisson problem: initialize_problem's arrays through the API, u bit for bit."""
    hip, _, K = libs
    B = Backend(hip, "hip")
    B.configure(H.OP_7PT, H.SMOOTH_CHEBY, helmholtz, 1)
    bench = B.solver_cli(log2, per_rank)
    try:
        lvl = bench.level(0)
        n, box_dim, bi = lvl.dim, lvl.box_dim, lvl.info[H.INFO_BOXES_IN_I]
        r_bench = bench.fmg(0)
        u_bench = lvl.interior(H.VECTOR_U)
    finally:
        bench.destroy()
    a = 1.0 if helmholtz else 0.0
    arr = benchmark_arrays(hip, bi, box_dim, "dirichlet", a, 1.0)
    with Solver(n, bc="dirichlet", smoother="cheby", a=a, b=1.0, lib=hip) as s:
        s.set_coefficients(arr["alpha"], arr["beta_i"], arr["beta_j"], arr["beta_k"])
        before = _counters(hip, K)
        u, info = s.solve(arr["f"], method="fmg", rtol=1e-10)
        after = _counters(hip, K)
    assert after[0] > before[0], "no brick visits: the user solve left the fused V-cycle kernels"
    assert after[1] > before[1], "no sweep-pair launches: the user solve left the fused Chebyshev kernels"
    assert np.array_equal(u, u_bench)
    assert "%1.15e" % info.residual == "%1.15e" % r_bench
    key = f"7pt-cheby{'-helm' if helmholtz else ''} {log2} {per_rank}"
    gold = load_golden("fcycle_norms.json").get(key)
    if gold:
        assert "%1.15e" % info.residual == gold["norms"][0]


def test_torch_tensors_in_place(libs):
    """A child process that imports torch first: device results equal host results bitwise, and out= is filled in place."""
    worker = os.path.join(ROOT, "tests", "user_problem_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr


def test_pack_unpack_round_trip_and_validation_at_256(libs):
    hip, _, K = libs
    n = 256
    with Solver(n, bc="dirichlet", smoother="cheby", a=1.0, lib=hip) as s:
        L = hip.hpgmg_solver_level(hip.hpgmg_user_solver_of(s._ptr), 0)
        rng = np.random.default_rng(256)
        x = rng.random((n, n, n))
        y = np.empty_like(x)
        assert hip.hpgmg_dense_pack(L, H.VECTOR_TEMP, x.ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0
        assert hip.hpgmg_dense_unpack(L, H.VECTOR_TEMP, y.ctypes.data, H.WHERE_HOST) == 0
        assert np.array_equal(x, y)
        D = DeviceArrays(K)
        try:                                                     # the device entry: in place, same bytes
            px, py = D.put(x), D.empty(x.nbytes)
            assert hip.hpgmg_dense_pack(L, H.VECTOR_E, px, H.WHERE_PLUGIN, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0
            assert hip.hpgmg_dense_unpack(L, H.VECTOR_E, py, H.WHERE_PLUGIN) == 0
            assert np.array_equal(D.get(py, x.shape), x)
        finally:
            D.free()
        x[-1, -1, -1] = np.nan                                   # one bad cell, in the last box
        assert hip.hpgmg_dense_pack(L, H.VECTOR_TEMP, x.ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == H.DENSE_NOT_FINITE
        beta = np.ones(face_shape(n, "dirichlet", 0))
        beta[-1, -1, -1] = -1.0                                  # face N of the last box: read from its ghost layer
        assert hip.hpgmg_dense_pack(L, H.VECTOR_TEMP, beta.ctypes.data, H.WHERE_HOST, H.DENSE_FACE_I, H.DENSE_CHECK_POSITIVE) == H.DENSE_OUT_OF_RANGE
        beta[-1, -1, -1] = 0.5
        assert hip.hpgmg_dense_pack(L, H.VECTOR_TEMP, beta.ctypes.data, H.WHERE_HOST, H.DENSE_FACE_I, H.DENSE_CHECK_POSITIVE) == 0
