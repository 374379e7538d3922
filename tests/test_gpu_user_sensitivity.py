"""Coefficient sensitivities on the MI355X: the HIP build (kernels/dense_sensitivity.hip, one launch for the four arrays) equals
the CPU oracle bit for bit and writes every entry, with arrays entering from the host (through the staging buffer, now sized for four) and from the
device (in place); kappa = 0 gives the Neumann solver's bytes; a non-finite boundary value is reported from host and device arrays; torch tensors
and hpgmg_amd.autograd.solve equal the NumPy path and the manual composition (a child process that imports torch first).

Solver shapes: N = 64 in boxes of 32 (2^3 boxes: every box touches three walls), N = 48 in boxes of 16 (3^3 boxes: boxes on zero to three walls,
box-to-box faces in the middle of the domain and, periodic, the wrap), N = 16 in boxes of 4 (rows shorter than a wave).

The hook alone (hpgmg_dense_unpack_sensitivity on test_gpu_operators.make_pair levels), three ways and all bitwise over every output entry: the HIP
plugin, the oracle's host default (host/hooks_host.inc) and the NumPy restatement (user_sensitivity_lib.restatement).  The launch shape, from
hpgmg_hip_dense_unpack_sensitivity (256 cells per workgroup, at most 4096 workgroups; the caps of kernels/dense_step.hip):
    per_box = ceil(side^3 / 256),  gridDim.y = min(boxes, 4096),  cap = 4096 / gridDim.y,  gridDim.x = min(per_box, cap)
    a workgroup makes ceil(per_box / gridDim.x) trips of the cell stride, a grid row takes ceil(boxes / gridDim.y) boxes; the cell index is divided
    when the side is no power of two.

    (boxes per side, side)  boxes  per_box  gridDim.y   cap  gridDim.x  cell trips  boxes per row
    (1, 104)                    1     4394          1  4096       4096           2              1   no power of two; 298 workgroups make a second trip
    (17, 2)                  4913        1       4096     1          1           1              2   817 grid rows take a second box; 8 of 256 lanes live
    (3, 12)                    27        7         27   151          7           1              1   no power of two; 1728 = 6 * 256 + 192: the last workgroup is partly live
    (1, 6)                      1        1          1  4096          1           1              1   216 of 256 lanes live
    (1, 1)                      1        1          1  4096          1           1              1   one cell, on all six walls: it writes seven entries
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
from test_gpu_operators import make_pair
from test_gpu_user_problem import DeviceArrays
from user_flux_lib import SOLVERS, boundary_for, kappa_for
from user_problem_lib import face_shape, random_coefficients
from user_robin_lib import ALL, CORNERS, D, N, R, neumann_of
from user_sensitivity_lib import restatement

pytestmark = pytest.mark.gpu

A, B = 1.3, 0.7


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
    rng = np.random.default_rng(seed + 1)
    u, lam = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 2.0 - 1.0
    return bc, coef, u, lam, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _shapes(n, bc):
    return [(n, n, n)] + [face_shape(n, bc, axis) for axis in range(3)]


def _sens(lib, n, box_dim, faces, a, coef, kappa, u, lam, g, device=None):
    """The status and the four arrays (the first None when a == 0) through hpgmg_user_sensitivity, every output pre-filled with NaN;
    device = DeviceArrays: every array lives in device memory."""
    bc = "periodic" if faces == "periodic" else "dirichlet"
    shapes = _shapes(n, bc)
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=B, lib=lib) as s:
        if device is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = [np.full(shape, np.nan) for shape in shapes]
            ptr = [q.ctypes.data for q in outs]
        else:
            put, w = device.put, H.WHERE_PLUGIN
            ptr = [device.put(np.full(shape, np.nan)) for shape in shapes]
        alpha, bi, bj, bk = coef
        if kappa is None:
            assert lib.hpgmg_user_set_coefficients(s._ptr, put(alpha), put(bi), put(bj), put(bk), w) == 0
        else:
            assert lib.hpgmg_user_set_coefficients_robin(s._ptr, put(alpha), put(bi), put(bj), put(bk), put(kappa), w) == 0
        st = lib.hpgmg_user_sensitivity(s._ptr, put(u), put(lam), put(g), ptr[0] if a != 0.0 else None, ptr[1], ptr[2], ptr[3], w)
        if device is not None:
            outs = [device.get(p, shape) for p, shape in zip(ptr, shapes)]
    if a == 0.0:
        assert np.isnan(outs[0]).all()          # no d_alpha on a Poisson solver: its buffer was not passed
        outs[0] = None
    return st, outs


def _bytes(q):
    return [None if x is None else x.tobytes() for x in q]


def _written(q):
    return all(x is None or np.isfinite(x).all() for x in q)


GRIDS = [(64, 32), (48, 16), (16, 4)]
NAMES = ["dirichlet", "periodic", "corners", "robin", "neumann"]
# every solver on every grid, from host and from device arrays; a alternates so that every solver and every grid sees Poisson and Helmholtz
CASES = [(n, box_dim, name, A if (gi + si) % 2 else 0.0) for gi, (n, box_dim) in enumerate(GRIDS) for si, name in enumerate(NAMES)]


@pytest.mark.parametrize("n,box_dim,name,a", CASES)
def test_hip_equals_oracle(libs, n, box_dim, name, a):
    hip, oracle, K = libs
    _, coef, u, lam, g, kappa = _inputs(name, n, a, 2000 + n + int(a))
    st_ref, ref = _sens(oracle, n, box_dim, SOLVERS[name], a, coef, kappa, u, lam, g)
    assert st_ref == H.USER_OK and _written(ref)
    st, host = _sens(hip, n, box_dim, SOLVERS[name], a, coef, kappa, u, lam, g)                     # through the staging buffer
    dev = DeviceArrays(K)
    try:
        st_d, device = _sens(hip, n, box_dim, SOLVERS[name], a, coef, kappa, u, lam, g, device=dev)      # in place
        st_0, none = _sens(hip, n, box_dim, SOLVERS[name], a, coef, kappa, u, lam, None, device=dev)     # zero data: no boundary array at all
    finally:
        dev.free()
    assert st == st_d == st_0 == H.USER_OK
    assert _bytes(host) == _bytes(ref)
    assert _bytes(device) == _bytes(ref)
    assert _written(none)                                                                            # every entry was written
    if g is not None:
        st_z, zero = _sens(oracle, n, box_dim, SOLVERS[name], a, coef, kappa, u, lam, np.zeros_like(g))
        assert st_z == H.USER_OK and _bytes(none) == _bytes(zero)


@pytest.mark.parametrize("walls,a", [(CORNERS, A), (ALL, 0.0)])
def test_kappa_zero_gives_the_neumann_solvers_bytes(libs, walls, a):
    hip, _, K = libs
    n, box_dim = 48, 16
    _, coef, u, lam, g, _ = _inputs("corners", n, a, 2100 + int(a))
    dev = DeviceArrays(K)
    try:
        st_ref, ref = _sens(hip, n, box_dim, neumann_of(walls), a, coef, None, u, lam, g, device=dev)
        st, got = _sens(hip, n, box_dim, walls, a, coef, np.zeros((6, n, n)), u, lam, g, device=dev)
    finally:
        dev.free()
    assert st == st_ref == H.USER_OK and _written(got)
    assert _bytes(got) == _bytes(ref)


def test_bad_values_are_reported_from_host_and_device(libs):
    hip, _, K = libs
    n = 48
    _, coef, u, lam, g, kappa = _inputs("corners", n, 0.0, 2200)
    dev = DeviceArrays(K)
    try:
        for face in range(6):
            bad = g.copy()
            bad[face, n - 1, n - 1] = np.nan if face & 1 else np.inf
            assert _sens(hip, n, 16, CORNERS, 0.0, coef, kappa, u, lam, bad, device=dev)[0] == H.USER_NOT_FINITE, face
            assert _sens(hip, n, 16, CORNERS, 0.0, coef, kappa, u, lam, bad)[0] == H.USER_NOT_FINITE, face
            dev.free()
        for which in (0, 1):
            bad = [u.copy(), lam.copy()]
            bad[which][n - 1, 0, n // 2] = np.nan
            assert _sens(hip, n, 16, CORNERS, 0.0, coef, kappa, bad[0], bad[1], g, device=dev)[0] == H.USER_NOT_FINITE, which
            dev.free()
    finally:
        dev.free()


# ---------------------------------------------------------------- the hook alone, at the edges of its launch shape
VARIANT = "7pt-cheby-helm"
U_ID, LAM_ID = H.VECTOR_U, H.VECTOR_F
GEOMS = [(1, 104), (17, 2), (3, 12), (1, 6), (1, 1)]
MIXED = 0b011010                                      # i-high, j-high and k-low are masked walls; the other three Dirichlet
WALLS = [("dirichlet", 0, False), ("neumann", 63, False), ("mixed-kappa", MIXED, True)]      # (name, mask, with a kappa array)
_pairs = {}


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom): the two levels of one geometry with the box-to-box ghost zones of u and lam filled (the caller's part of the hook's
    contract) and the two as dense arrays; made once and kept for the module (4913 boxes take seconds to fill box by box)."""
    def get(geom):
        if geom not in _pairs:
            lh, lo = make_pair(hip, oracle, VARIANT, *geom, seed=41 + geom[1])
            for lv in (lh, lo):
                for vid in (U_ID, LAM_ID):
                    lv.b.lib.exchange_boundary(lv.ptr, vid, lv.b.lib.stencil_get_shape())
            assert lh.ghosts >= 1 and lh.num_boxes == geom[0] ** 3 and lh.box_dim == geom[1]
            _pairs[geom] = (lh, lo, lo.interior(U_ID), lo.interior(LAM_ID))
        return _pairs[geom]
    return get


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    while _pairs:
        lh, lo, _, _ = _pairs.popitem()[1]
        lh.destroy(); lo.destroy()


def _id(v):
    return f"{v[0]}x{v[1]}" if isinstance(v[0], int) else v[0]          # a geometry, or the name of a WALLS entry


class _Plugin:
    """Boundary arrays in a backend's plugin memory (hpgmg_vector_alloc)."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, a):
        if a is None:
            return None
        p = self.lib.hpgmg_vector_alloc(a.size)
        self.lib.hpgmg_vector_upload(p, a.ctypes.data, a.size)
        self.ptrs.append(p)
        return p

    def free(self):
        for p in self.ptrs:
            self.lib.hpgmg_vector_free(p)
        self.ptrs = []


@pytest.mark.parametrize("walls", WALLS, ids=_id)
@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_the_hook_three_ways(libs, pair_of, geom, walls):
    """HIP from host arrays (staged), HIP into device arrays (in place), the oracle's host default and the NumPy restatement: the same bits in
    every entry of the four arrays (three with mask 0, which runs without alpha: d_alpha NULL), and no entry left at its NaN pre-fill."""
    _, mask, with_kappa = walls
    _, _, K = libs
    lh, lo, u, lam = pair_of(geom)
    n, h = lh.dim, lh.h
    helm = mask != 0
    rng = np.random.default_rng(4200 + n + mask)
    g = rng.random((6, n, n)) * 4.0 - 2.0
    wall = rng.random((6, n, n)) + 0.5 if mask else None
    kappa = rng.random((6, n, n)) * 3.0 if with_kappa else None
    faces = tuple((R if with_kappa else N) if (mask >> f) & 1 else D for f in range(6))
    ref = [q for q, _ in restatement(n, "dirichlet", faces, A if helm else 0.0, B, h, u, lam, g, kappa)]
    shapes = _shapes(n, "dirichlet")
    seen = {}
    for key, lv, where in (("hip-host", lh, H.WHERE_HOST), ("oracle", lo, H.WHERE_HOST), ("hip-device", lh, H.WHERE_PLUGIN)):
        mem, dev = _Plugin(lv.b.lib), DeviceArrays(K)
        try:
            if where == H.WHERE_HOST:
                outs = [np.full(shape, np.nan) for shape in shapes]
                ptr = [q.ctypes.data for q in outs]
            else:
                ptr = [dev.put(np.full(shape, np.nan)) for shape in shapes]
            st = lv.b.lib.hpgmg_dense_unpack_sensitivity(lv.ptr, U_ID, LAM_ID, mem.put(g), A, B, mask, mem.put(wall), mem.put(kappa),
                                                         ptr[0] if helm else None, ptr[1], ptr[2], ptr[3], where)
            if where == H.WHERE_PLUGIN:
                outs = [dev.get(p, shape) for p, shape in zip(ptr, shapes)]
        finally:
            mem.free(); dev.free()
        assert st == 0, key
        if not helm:
            assert np.isnan(outs[0]).all(), key
            outs[0] = None
        seen[key] = outs
    for key, outs in seen.items():
        for slot, (q, q_ref) in enumerate(zip(outs, ref)):
            assert (q is None) == (q_ref is None), (key, slot)
            if q is None:
                continue
            bad = np.argwhere(q.view(np.uint64) != q_ref.view(np.uint64))
            assert bad.size == 0, f"{key} array {slot}: differs from the restatement at {bad[:5].tolist()} ... ({len(bad)} entries)"


def test_the_hook_reports_a_bad_value_and_refuses_what_flux_refuses(libs, pair_of):
    lh, lo, u, lam = pair_of((3, 12))
    n = lh.dim
    shapes = _shapes(n, "dirichlet")
    for lv in (lh, lo):
        lib, mem = lv.b.lib, _Plugin(lv.b.lib)
        outs = [np.full(shape, np.nan) for shape in shapes]
        ptr = [q.ctypes.data for q in outs]
        try:
            g = np.zeros((6, n, n))
            g[3, 5, 7] = np.inf
            pg = mem.put(g)
            call = lib.hpgmg_dense_unpack_sensitivity
            assert call(lv.ptr, U_ID, LAM_ID, pg, A, B, 0, None, None, *ptr, H.WHERE_HOST) == H.DENSE_NOT_FINITE
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 0, None, None, *ptr, H.WHERE_HOST) == 0
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 0, None, None, None, *ptr[1:], H.WHERE_HOST) == 0          # d_alpha may be NULL
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 0, None, None, ptr[0], None, ptr[2], ptr[3], H.WHERE_HOST) == -1
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 5, None, None, *ptr, H.WHERE_HOST) == -1                  # a mask without the wall betas
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 64, pg, None, *ptr, H.WHERE_HOST) == -1
            assert call(lv.ptr, -1, LAM_ID, None, A, B, 0, None, None, *ptr, H.WHERE_HOST) == -1
            assert call(lv.ptr, U_ID, lv.num_vectors, None, A, B, 0, None, None, *ptr, H.WHERE_HOST) == -1
            assert call(lv.ptr, U_ID, LAM_ID, None, A, B, 0, None, None, *ptr, 2) == -1
        finally:
            mem.free()


def test_torch_tensors_and_autograd(libs):
    """A child process that imports torch first: sensitivity on tensors equals the NumPy path bitwise, out= is written in place, and the gradients
    of hpgmg_amd.autograd.solve are lam and -sensitivity(u, lam, boundary=g) of the manual composition, bitwise; its three errors raise."""
    worker = os.path.join(ROOT, "tests", "user_sensitivity_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
