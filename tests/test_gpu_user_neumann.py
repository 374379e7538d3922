"""Neumann and mixed walls on the MI355X: the HIP build (kernels/dense_io.hip dense_pack_walls_kernel, kernels/dense_boundary.hip) equals the
CPU oracle bit for bit for the lifted right-hand side, apply(boundary=) and u of both methods; the masked pack with mask 0 writes the plain
pack's bytes; torch tensors equal the NumPy path; at 256^3 the mixed-wall F-cycle meets the accuracy gate measured on the oracle and its
V-cycles stay on the fused brick and sweep-pair kernels.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend
from test_gpu_user_problem import DeviceArrays, _counters
from user_boundary_lib import exact, manufactured
from user_neumann_lib import ALL, SIDES, grad_exact, mask_of
from user_problem_lib import random_coefficients

pytestmark = pytest.mark.gpu

FMG_FACTOR = 1.5            # test_oracle_user_neumann.py: measured 0.90 - 1.26 on the oracle at N = 16 .. 64


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _run(lib, n, box_dim, faces, smoother, a, coef, f, g, x, device=None):
    """F (the lifted right-hand side as packed), A_N x - T(g), u of fmg, u of mg, u of fmg with no data, and the infos, through the C entry points."""
    alpha, bi, bj, bk = coef
    out = {}
    with Solver(n, box_dim=box_dim, bc=faces, smoother=smoother, a=a, b=1.0, lib=lib) as s:
        S, info, shift = s._ptr, H.UserInfo(), ctypes.c_double()
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        D = device
        keys = ("F", "y", "u_fmg", "u_mg", "u_zero")
        if D is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = {k: np.empty((n, n, n)) for k in keys}
            ptr = {k: v.ctypes.data for k, v in outs.items()}
        else:
            put, w = D.put, H.WHERE_PLUGIN
            ptr = {k: D.empty(f.nbytes) for k in keys}
        assert lib.hpgmg_user_set_coefficients(S, put(alpha), put(bi), put(bj), put(bk), w) == 0
        pf, pg = put(f), put(g)
        for method, key in ((H.USER_FMG, "u_fmg"), (H.USER_MG, "u_mg")):
            assert lib.hpgmg_user_set_rhs_dirichlet(S, pf, pg, w, ctypes.byref(shift)) == 0
            if key == "u_fmg":
                assert lib.hpgmg_dense_unpack(L, H.VECTOR_F, ptr["F"], w) == 0
            assert lib.hpgmg_user_solve(S, method, 1e-10, None, w, ctypes.byref(info)) == 0
            out[key + "_info"] = (info.norm_of_residual, info.norm_of_f, info.vcycles, info.mean_shift)
            assert lib.hpgmg_user_get_solution(S, ptr[key], w) == 0
        assert lib.hpgmg_user_set_rhs(S, pf, w, ctypes.byref(shift)) == 0          # zero data: the hook still runs
        assert lib.hpgmg_user_solve(S, H.USER_FMG, 1e-10, None, w, ctypes.byref(info)) == 0
        out["u_zero_info"] = (info.norm_of_residual, info.norm_of_f, info.vcycles, info.mean_shift)
        assert lib.hpgmg_user_get_solution(S, ptr["u_zero"], w) == 0
        assert lib.hpgmg_user_apply_dirichlet(S, put(x), pg, ptr["y"], w) == 0
        for k in keys:
            out[k] = outs[k] if D is None else D.get(ptr[k], f.shape)
    return out


CASES = [  # n, box_dim, walls, smoother, a, entry
    (64, 32, SIDES, "cheby", 1.0, "host"),
    (64, 32, SIDES, "cheby", 0.0, "device"),
    (64, 32, ALL, "cheby", 0.0, "device"),
    (64, 32, ALL, "gsrb", 1.0, "device"),
    (64, 32, SIDES, "jacobi", 0.0, "host"),
    (48, 16, SIDES, "cheby", 0.0, "host"),
    (48, 16, ALL, "cheby", 1.0, "device"),
    (48, 16, SIDES, "gsrb", 0.0, "host"),
    (48, 16, ALL, "jacobi", 0.0, "device"),
]


@pytest.mark.parametrize("n,box_dim,walls,smoother,a,entry", CASES)
def test_hip_equals_oracle(libs, n, box_dim, walls, smoother, a, entry):
    hip, oracle, K = libs
    coef = random_coefficients(n, "dirichlet", a != 0.0, seed=600 + n + len(smoother) + int(a))
    rng = np.random.default_rng(n + 2)
    f, x, g = rng.random((n, n, n)) - 0.3, rng.random((n, n, n)) * 2.0 - 1.0, rng.random((6, n, n)) * 4.0 - 2.0
    ref = _run(oracle, n, box_dim, walls, smoother, a, coef, f, g, x)
    D = DeviceArrays(K) if entry == "device" else None
    try:
        got = _run(hip, n, box_dim, walls, smoother, a, coef, f, g, x, device=D)
    finally:
        if D:
            D.free()
    for key in ("F", "y", "u_fmg", "u_mg", "u_zero"):
        assert np.array_equal(got[key], ref[key]), key
    for key in ("u_fmg_info", "u_mg_info", "u_zero_info"):
        assert got[key] == ref[key], key
    if walls == ALL and a == 0.0:
        assert ref["u_fmg_info"][3] != 0.0                     # the singular case went through the mean shift


@pytest.mark.parametrize("n,box_dim", [(64, 32), (48, 16)])
def test_masked_pack_with_mask_0_is_the_plain_pack(libs, n, box_dim):
    """Whole padded boxes, byte for byte; and with a mask the only difference is 0.0 on the masked walls, whose values land in the wall array."""
    hip, _, K = libs
    coef = random_coefficients(n, "dirichlet", False, seed=700 + n)
    D = DeviceArrays(K)
    try:
        with Solver(n, box_dim=box_dim, lib=hip) as s:
            L = hip.hpgmg_solver_level(hip.hpgmg_user_solver_of(s._ptr), 0)
            info = (ctypes.c_int * H.INFO_COUNT)()
            hip.hpgmg_level_info(L, info)
            vol, boxes, dim, gh = info[H.INFO_VOLUME], info[H.INFO_NUM_MY_BOXES], info[H.INFO_BOX_DIM], info[H.INFO_GHOSTS]
            strides = (1, info[H.INFO_JSTRIDE], info[H.INFO_KSTRIDE])

            def read(vid):
                out = np.empty((boxes, vol))
                for box in range(boxes):
                    hip.hpgmg_level_read_vector(L, box, vid, out[box].ctypes.data)
                return out

            for axis, (vid, beta) in enumerate(zip((H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K), coef[1:])):
                layout = H.DENSE_FACE_I + axis
                wall = D.put(np.full((6, n, n), -7.0))
                for where, src in ((H.WHERE_HOST, beta.ctypes.data), (H.WHERE_PLUGIN, D.put(beta))):
                    assert hip.hpgmg_dense_pack(L, vid, src, where, layout, H.DENSE_CHECK_POSITIVE) == 0
                    plain = read(vid)
                    assert hip.hpgmg_dense_pack_walls(L, vid, src, where, layout, H.DENSE_CHECK_POSITIVE, 0, wall) == 0
                    assert plain.tobytes() == read(vid).tobytes()
                    assert np.all(D.get(wall, (6, n, n)) == -7.0)              # mask 0 leaves the wall array alone
                assert hip.hpgmg_dense_pack_walls(L, vid, beta.ctypes.data, H.WHERE_HOST, layout, H.DENSE_CHECK_POSITIVE, 63, wall) == 0
                masked, expect = read(vid), plain.copy()
                for box in range(boxes):
                    low = (ctypes.c_int * 3)()
                    hip.hpgmg_level_box_low(L, box, low)
                    cells = np.arange(dim)[:, None] * strides[(axis + 1) % 3] + np.arange(dim)[None, :] * strides[(axis + 2) % 3] + gh * sum(strides)
                    if low[axis] == 0:
                        expect[box][cells] = 0.0
                    if low[axis] + dim == n:
                        expect[box][cells + dim * strides[axis]] = 0.0
                assert masked.tobytes() == expect.tobytes()
                got = D.get(wall, (6, n, n))
                lo, hi = (np.take(beta, at, axis=2 - axis) for at in (0, n))
                assert np.array_equal(got[2 * axis], lo) and np.array_equal(got[2 * axis + 1], hi)
                assert np.all(np.delete(got, (2 * axis, 2 * axis + 1), axis=0) == -7.0)      # the other axes' faces are not this array's
                bad = beta.copy()
                bad[(slice(None),) * (2 - axis) + (0,)].flat[5] = -1.0         # a masked wall's value is still checked
                assert hip.hpgmg_dense_pack_walls(L, vid, bad.ctypes.data, H.WHERE_HOST, layout, H.DENSE_CHECK_POSITIVE, 63, wall) == H.DENSE_OUT_OF_RANGE
    finally:
        D.free()


def test_torch_tensors(libs):
    """A child process that imports torch first: mixed walls with tensors equal the NumPy path bitwise."""
    worker = os.path.join(ROOT, "tests", "user_neumann_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr


def test_helmholtz_256_mixed_walls_on_the_fast_path(libs):
    hip, _, K = libs
    n = 256
    alpha, bi, bj, bk, f, u_star = manufactured(n, 1.0, 1.0)
    with Solver(n, bc=SIDES, smoother="cheby", a=1.0, b=1.0, lib=hip) as s:
        s.set_coefficients(alpha, bi, bj, bk)
        g = s.boundary_from(exact, grad=grad_exact)
        before = _counters(hip, K)
        u_fmg, info = s.solve(f, method="fmg", boundary=g)
        after = _counters(hip, K)
        u_mg, info_mg = s.solve(f, method="mg", rtol=1e-12, boundary=g)
    assert after[0] > before[0], "no brick visits: the mixed-wall F-cycle's V-cycles left the fused kernels"
    assert after[1] > before[1], "no sweep-pair launches: the mixed-wall F-cycle's V-cycles left the fused Chebyshev kernels"
    assert info.vcycles == 1 and info_mg.converged
    e_fmg, e_mg = np.abs(u_fmg - u_star).max(), np.abs(u_mg - u_star).max()
    print(f"256^3 manufactured, Neumann side walls: F-cycle error {e_fmg:.3e}, V-cycles {e_mg:.3e} ({info_mg.vcycles}), ratio {e_fmg / e_mg:.3f}")
    assert e_fmg <= FMG_FACTOR * e_mg, (e_fmg, e_mg)
