"""Cell-centred conductivities on the MI355X: the HIP build (kernels/dense_cells.hip: one launch packs the three beta vectors from
the cell field, one launch writes d_alpha and d_k) equals the CPU oracle bit for bit, with arrays entering from the host (through the staging buffer)
and from the device (in place): apply and flux after set_cell_coefficients, the two arrays of cell_sensitivity with every entry written over a NaN
pre-fill, the statuses of a bad k; torch tensors and hpgmg_amd.autograd.solve_cells equal the NumPy path and the manual composition (a child
process that imports torch first).

Solver shapes: N = 64 in boxes of 32 (2^3 boxes: every box touches three walls), N = 48 in boxes of 16 (3^3 boxes: boxes on zero to three walls,
box-to-box faces in the middle of the domain and, periodic, the wrap), N = 16 in boxes of 4 (rows shorter than a wave).

The hooks alone (hpgmg_dense_pack_cell_mean, hpgmg_dense_unpack_cell_sensitivity on test_gpu_operators.make_pair levels), three ways and all
bitwise: the HIP plugin (staged and in place), the oracle's host default (host/hooks_host.inc) and the NumPy restatement (user_cells_lib.face_mean
through dense_hooks_lib.pack / pack_walls; user_sensitivity_lib.restatement through user_cells_lib.cell_gather).

The pack's launch shape, from hpgmg_hip_dense_pack_cell_mean (256 lanes per workgroup over the padded volume of a box, at most 16384 workgroups
along x and 65535 grid rows: dense_grid's caps of kernels/dense_io.hip):
    blocks = ceil(volume / 256),  gridDim.x = min(blocks, 16384),  gridDim.y = min(boxes, 65535);  a workgroup makes ceil(blocks / gridDim.x) trips

    (boxes per side, side)  boxes  padded volume  blocks  gridDim.x  trips
    (1, 162)                    1      4,410,944   17230      16384      2   the smallest side whose padded volume exceeds one trip of 16384 x 256 lanes
    (3, 12)                    27          3,136      13         13      1   a middle box on no wall, boxes on one to three walls; the last workgroup partly live
    (17, 2)                  4913             64       1          1      1   4913 grid rows, most boxes on no wall; 64 of 256 lanes live
    (1, 6)                      1            512       2          2      1   a side that is no power of two
    (1, 1)                      1             36       1          1      1   one cell on six walls: its lane and three ghost lanes write the six wall betas
and a periodic (3, 12), where the low faces of the first boxes take the wrap.

The cell sensitivity's launch shape, from hpgmg_hip_dense_unpack_cell_sensitivity (256 cells per workgroup, at most 4096 workgroups: the caps of
kernels/dense_sensitivity.hip, so its table holds):
    per_box = ceil(side^3 / 256),  gridDim.y = min(boxes, 4096),  cap = 4096 / gridDim.y,  gridDim.x = min(per_box, cap)

    (boxes per side, side)  boxes  per_box  gridDim.y   cap  gridDim.x  cell trips  boxes per row
    (1, 104)                    1     4394          1  4096       4096           2              1   no power of two; 298 workgroups make a second trip
    (17, 2)                  4913        1       4096     1          1           1              2   817 grid rows take a second box; 8 of 256 lanes live
    (3, 12)                    27        7         27   151          7           1              1   no power of two; the last workgroup is partly live
    (1, 6)                      1        1          1  4096          1           1              1   216 of 256 lanes live
    (1, 1)                      1        1          1  4096          1           1              1   one cell on all six walls: no neighbour of k is read
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_hooks_lib as DH
import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import ROOT, Backend
from test_gpu_dense_hooks import Pair, _Mem
from test_gpu_user_problem import DeviceArrays
from user_cells_lib import MEANS, STATUS_CASES, block_field, cell_gather, face_mean, planted
from user_flux_lib import SOLVERS, boundary_for, kappa_for
from user_problem_lib import face_shape
from user_robin_lib import D, N, R
from user_sensitivity_lib import restatement

pytestmark = pytest.mark.gpu

A, B = 1.3, 0.7
MEAN_ID = {"harmonic": H.MEAN_HARMONIC, "arithmetic": H.MEAN_ARITHMETIC}
BETAS = (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
U_ID, LAM_ID = H.VECTOR_U, H.VECTOR_F
SENTINEL = -7.0


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


def _bytes(q):
    return [None if x is None else x.tobytes() for x in q]


# ---------------------------------------------------------------- through the API
def _inputs(name, n, a, seed):
    rng = np.random.default_rng(seed + 1)
    alpha = rng.random((n, n, n)) + 0.5 if a != 0.0 else None
    x, lam = rng.random((n, n, n)) * 2.0 - 1.0, rng.random((n, n, n)) * 2.0 - 1.0
    return alpha, block_field(n, seed), x, lam, boundary_for(name, n, seed + 2), kappa_for(name, n)


def _run(lib, n, box_dim, faces, a, alpha, k, mean, kappa, x, lam, g, device=None):
    """(status of set_cell_coefficients, [A x - T(g), the three fluxes], status of cell_sensitivity, [d_alpha, d_k]) through the C entry points, every
    output pre-filled with NaN; device = DeviceArrays: every array lives in device memory.  A refused set ends the run there."""
    bc = "periodic" if faces == "periodic" else "dirichlet"
    shapes = [(n, n, n)] + [face_shape(n, bc, axis) for axis in range(3)] + [(n, n, n), (n, n, n)]
    with Solver(n, box_dim=box_dim, bc=faces, a=a, b=B, lib=lib) as s:
        if device is None:
            put, w = (lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST
            outs = [np.full(shape, np.nan) for shape in shapes]
            ptr = [q.ctypes.data for q in outs]
        else:
            put, w = device.put, H.WHERE_PLUGIN
            ptr = [device.put(np.full(shape, np.nan)) for shape in shapes]
        st = lib.hpgmg_user_set_cell_coefficients(s._ptr, put(alpha), put(k), MEAN_ID[mean], put(kappa), w)
        if st != H.USER_OK:
            return st, None, None, None
        pg = put(g)
        assert (lib.hpgmg_user_apply(s._ptr, put(x), ptr[0], w) if g is None else lib.hpgmg_user_apply_dirichlet(s._ptr, put(x), pg, ptr[0], w)) == 0
        assert lib.hpgmg_user_flux(s._ptr, put(x), pg, ptr[1], ptr[2], ptr[3], w) == 0
        st_s = lib.hpgmg_user_cell_sensitivity(s._ptr, put(x), put(lam), put(k), MEAN_ID[mean], pg, ptr[4] if a != 0.0 else None, ptr[5], w)
        if device is not None:
            outs = [device.get(p, shape) for p, shape in zip(ptr, shapes)]
    if a == 0.0:
        assert np.isnan(outs[4]).all()          # no d_alpha on a Poisson solver: its buffer was not passed
        outs[4] = None
    return st, outs[:4], st_s, outs[4:]


GRIDS = [(64, 32), (48, 16), (16, 4)]
NAMES = ["dirichlet", "periodic", "corners", "robin", "neumann"]


@pytest.mark.parametrize("a", [0.0, A])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("n,box_dim", GRIDS)
def test_hip_equals_oracle(libs, n, box_dim, name, a):
    hip, oracle, K = libs
    alpha, k, x, lam, g, kappa = _inputs(name, n, a, 5000 + n + int(a))
    for mean in MEANS:
        st, ref, st_s, ref_s = _run(oracle, n, box_dim, SOLVERS[name], a, alpha, k, mean, kappa, x, lam, g)
        assert st == st_s == H.USER_OK and all(np.isfinite(q).all() for q in ref + [q for q in ref_s if q is not None])
        host = _run(hip, n, box_dim, SOLVERS[name], a, alpha, k, mean, kappa, x, lam, g)                  # through the staging buffer
        dev = DeviceArrays(K)
        try:
            device = _run(hip, n, box_dim, SOLVERS[name], a, alpha, k, mean, kappa, x, lam, g, device=dev)   # in place
        finally:
            dev.free()
        for key, (st_h, got, st_hs, got_s) in (("host", host), ("device", device)):
            assert st_h == st_hs == H.USER_OK, (key, mean)
            assert _bytes(got) == _bytes(ref), (key, mean)
            assert _bytes(got_s) == _bytes(ref_s), (key, mean)                                            # every entry written: the oracle's are finite


@pytest.mark.parametrize("case", STATUS_CASES, ids=lambda c: c[0])
def test_statuses_from_host_and_device(libs, case):
    """A bad k is reported by set_cell_coefficients and by cell_sensitivity alike, from host arrays and from device arrays."""
    hip, _, K = libs
    _, plants, mean, status, _ = case
    n, box_dim = 24, 8
    alpha, good, x, lam, g, kappa = _inputs("corners", n, 0.0, 5100)
    k = planted(n, plants)
    out = np.full((n, n, n), np.nan)
    dev = DeviceArrays(K)
    try:
        for device in (None, dev):
            assert _run(hip, n, box_dim, SOLVERS["corners"], 0.0, None, k, mean, kappa, x, lam, g, device=device)[0] == status
            put, w = ((lambda v: None if v is None else v.ctypes.data), H.WHERE_HOST) if device is None else (device.put, H.WHERE_PLUGIN)
            with Solver(n, box_dim=box_dim, bc=SOLVERS["corners"], b=B, lib=hip) as s:
                assert hip.hpgmg_user_set_cell_coefficients(s._ptr, None, put(good), MEAN_ID[mean], put(kappa), w) == H.USER_OK
                assert hip.hpgmg_user_cell_sensitivity(s._ptr, put(x), put(lam), put(k), MEAN_ID[mean], None, None, put(out), w) == status
            dev.free()
    finally:
        dev.free()


# ---------------------------------------------------------------- the hooks alone, at the edges of their launch shapes
PERIODIC = (3, 12, "periodic")
SENS_GEOMS = [(1, 104), (17, 2), (3, 12), (1, 6), (1, 1)]
_pairs = {}


def _id(g):
    return DH.geom_id(g[:2]) + ("-periodic" if len(g) > 2 else "") if isinstance(g[0], int) else g[0]


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom): the two levels of one geometry (test_gpu_dense_hooks.Pair) with lam's box-to-box ghost zones filled as well as u's (the
    caller's part of the sensitivity hook's contract); made once and kept for the module (4913 boxes take seconds to fill box by box)."""
    def get(geom):
        if geom not in _pairs:
            P = _pairs[geom] = Pair(hip, oracle, geom)
            for lv in (P.lh, P.lo):
                lv.b.lib.exchange_boundary(lv.ptr, LAM_ID, lv.b.lib.stencil_get_shape())
            P.lam = DH.unpack(P.geo, P.lo.read_all(LAM_ID))
        return _pairs[geom]
    return get


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    while _pairs:
        _pairs.popitem()[1].destroy()


def _packed(P, K, k, mean, mask, expect=0):
    """The three beta vectors (whole padded boxes, over a NaN pre-fill) and the wall array (over a sentinel) after the hook on each of the three sides."""
    n = P.n
    before = np.full((6, n, n), SENTINEL)
    seen = {}
    for key, lv, where, mem in P.sides(K):
        walls = _Mem(lv.b.lib)
        try:
            for vid in BETAS:
                lv.write_all(vid, P.nan)
            pw = walls.put(before)
            st = lv.b.lib.hpgmg_dense_pack_cell_mean(lv.ptr, mem.put(k), where, MEAN_ID[mean], mask, pw if mask else None)
            assert st == expect, (key, mean, mask, st)
            seen[key] = [lv.read_all(vid) for vid in BETAS] + [walls.get(pw, before.shape)]
        finally:
            mem.free(); walls.free()
    return seen, before


def _face_route(P, k, mean, mask, before):
    """What the existing packs leave for the three face arrays of means: the restatement of the contract."""
    F = face_mean(P.n, "periodic" if P.periodic else "dirichlet", k, mean)
    wall, vectors = before, []
    for axis in range(3):
        if mask:
            boxes, wall = DH.pack_walls(P.geo, F[axis], H.DENSE_FACE_I + axis, mask, wall)
        else:
            boxes = DH.pack(P.geo, F[axis], H.DENSE_FACE_I + axis)
        vectors.append(boxes)
    return vectors + [wall]


def _agree(seen, want, computed_nan=False):
    for key, arrays in seen.items():
        assert len(arrays) == len(want)
        for slot, (a, b) in enumerate(zip(arrays, want)):
            assert DH.same_bits(a, b, computed_nan), f"{key} array {slot} against the restatement: {DH.first_differences(a, b, computed_nan=computed_nan)}"


PACK_CASES = [(geom, walls) for geom in DH.GEOMS for walls in DH.WALLS] + [(PERIODIC, DH.WALLS[0])]      # a periodic level has no walls to mask


@pytest.mark.parametrize("geom,walls", PACK_CASES, ids=lambda v: _id(v))
def test_the_pack_hook_three_ways(libs, pair_of, geom, walls):
    """HIP from a host array (staged), HIP from a device array (in place), the oracle's host default and the face route restated in NumPy: the same bits
    in every padded double of every box of the three vectors and in every entry of `wall` (which keeps its pre-fill on the faces that are not masked
    and, with mask 0, everywhere)."""
    _, mask, _ = walls
    _, _, K = libs
    P = pair_of(geom)
    k = block_field(P.n, 5200 + P.n + mask)
    for mean in MEANS:
        seen, before = _packed(P, K, k, mean, mask)
        _agree(seen, _face_route(P, k, mean, mask, before))


def _status_cells(geom, n):
    if geom[:2] == (1, 162):
        return [("second-trip", (157, 3, 5))]             # padded offset >= 4,194,304: only the second trip of the x stride reaches it
    out = [("first", (0, 0, 0)), ("last", (n - 1, n - 1, n - 1))]
    if geom[:2] == (3, 12):
        out.append(("middle-box", (17, 12, 23)))
    return out


@pytest.mark.parametrize("geom", [(1, 162), (3, 12), PERIODIC], ids=_id)
def test_the_pack_hook_status_word(libs, pair_of, geom):
    """One bad entry per call at each position only one lane or one trip reaches, and the two mean cases across a box face; a bad status still
    leaves the bytes the face route leaves (any NaN where the arithmetic met the planted value)."""
    _, _, K = libs
    P = pair_of(geom)
    n = P.n
    mask = 0 if P.periodic else DH.MIXED
    for _, at in _status_cells(geom, n):
        for value, expect in ((np.nan, H.DENSE_NOT_FINITE), (-1.0, H.DENSE_OUT_OF_RANGE)):
            k = np.ones((n, n, n))
            k[at] = value
            seen, before = _packed(P, K, k, "harmonic", mask, expect)
            _agree(seen, _face_route(P, k, "harmonic", mask, before), computed_nan=True)
    if P.geo.boxes > 1:
        d = P.geo.dim                                       # the two cells on either side of a box face (the wrap on the periodic level: cells n - 1 and 0)
        lo, hi = ((5, 6, n - 1), (5, 6, 0)) if P.periodic else ((5, 6, d - 1), (5, 6, d))
        for value, expect in ((1e200, H.DENSE_NOT_FINITE), (1e-200, H.DENSE_OUT_OF_RANGE)):
            k = np.ones((n, n, n))
            k[lo] = k[hi] = value
            _packed(P, K, k, "harmonic", mask, expect)
            _packed(P, K, k, "arithmetic", mask, 0)
        k = np.ones((n, n, n))
        k[lo], k[hi] = -1.0, np.inf
        _packed(P, K, k, "harmonic", mask, H.DENSE_NOT_FINITE | H.DENSE_OUT_OF_RANGE)


@pytest.mark.parametrize("walls", DH.WALLS, ids=_id)
@pytest.mark.parametrize("geom", SENS_GEOMS, ids=_id)
def test_the_cell_sensitivity_hook_three_ways(libs, pair_of, geom, walls):
    """HIP from host arrays (staged), HIP on device arrays (in place), the oracle's host default and the restatement (the face pass of
    user_sensitivity_lib gathered by user_cells_lib.cell_gather): the same bits in every entry of d_alpha and d_k (d_k alone with mask 0, which runs
    without alpha: d_alpha NULL), and no entry left at its NaN pre-fill."""
    _, mask, with_kappa = walls
    _, _, K = libs
    P = pair_of(geom)
    n, h, helm = P.n, P.h, mask != 0
    rng = np.random.default_rng(5300 + n + mask)
    g = rng.random((6, n, n)) * 4.0 - 2.0
    wall = rng.random((6, n, n)) + 0.5 if mask else None
    kappa = rng.random((6, n, n)) * 3.0 if with_kappa else None
    faces = tuple((R if with_kappa else N) if (mask >> f) & 1 else D for f in range(6))
    k = block_field(n, 5301 + n)
    G = [q for q, _ in restatement(n, "dirichlet", faces, A if helm else 0.0, B, h, P.u, P.lam, g, kappa)]
    for mean in MEANS:
        ref = [G[0], cell_gather(n, "dirichlet", k, mean, *G[1:])]
        for key, lv, where, mem in P.sides(K):
            bnd = _Mem(lv.b.lib)
            try:
                ptr = [mem.put(np.full((n, n, n), np.nan)) for _ in range(2)]
                st = lv.b.lib.hpgmg_dense_unpack_cell_sensitivity(lv.ptr, U_ID, LAM_ID, mem.put(k), MEAN_ID[mean], bnd.put(g), A, B, mask, bnd.put(wall),
                                                                  bnd.put(kappa), ptr[0] if helm else None, ptr[1], where)
                outs = [mem.get(p, (n, n, n)) for p in ptr]
            finally:
                mem.free(); bnd.free()
            assert st == 0, (key, mean)
            if not helm:
                assert np.isnan(outs[0]).all(), key
                outs[0] = None
            for slot, (q, q_ref) in enumerate(zip(outs, ref)):
                assert (q is None) == (q_ref is None), (key, mean, slot)
                if q is not None:
                    assert DH.same_bits(q, q_ref), f"{key} {mean} array {slot}: {DH.first_differences(q, q_ref)}"


def test_the_cell_sensitivity_hook_on_a_periodic_level(libs, pair_of):
    _, _, K = libs
    P = pair_of(PERIODIC)
    n = P.n
    k = block_field(n, 5400)
    G = [q for q, _ in restatement(n, "periodic", None, A, B, P.h, P.u, P.lam)]
    for mean in MEANS:
        ref = [G[0], cell_gather(n, "periodic", k, mean, *G[1:])]
        for key, lv, where, mem in P.sides(K):
            try:
                ptr = [mem.put(np.full((n, n, n), np.nan)) for _ in range(2)]
                assert lv.b.lib.hpgmg_dense_unpack_cell_sensitivity(lv.ptr, U_ID, LAM_ID, mem.put(k), MEAN_ID[mean], None, A, B, 0, None, None, ptr[0],
                                                                    ptr[1], where) == 0, key
                outs = [mem.get(p, (n, n, n)) for p in ptr]
            finally:
                mem.free()
            assert DH.same_bits(outs[0], ref[0]) and DH.same_bits(outs[1], ref[1]), (key, mean)


def test_the_hooks_refuse(libs, pair_of):
    """-1 from both backends alike, with nothing written."""
    P, Pp = pair_of((3, 12)), pair_of(PERIODIC)
    n = P.n
    k = block_field(n, 5500)
    for lv, lvp in ((P.lh, Pp.lh), (P.lo, Pp.lo)):
        lib, mem = lv.b.lib, _Mem(lv.b.lib)
        try:
            for vid in BETAS:
                lv.write_all(vid, P.nan)
            wall = mem.put(np.full((6, n, n), SENTINEL))
            pack, p = lib.hpgmg_dense_pack_cell_mean, k.ctypes.data
            assert pack(lv.ptr, None, H.WHERE_HOST, H.MEAN_HARMONIC, 0, None) == -1
            assert pack(lv.ptr, p, 2, H.MEAN_HARMONIC, 0, None) == -1
            assert pack(lv.ptr, p, H.WHERE_HOST, 2, 0, None) == -1
            assert pack(lv.ptr, p, H.WHERE_HOST, -1, 0, None) == -1
            assert pack(lv.ptr, p, H.WHERE_HOST, H.MEAN_HARMONIC, 64, wall) == -1
            assert pack(lv.ptr, p, H.WHERE_HOST, H.MEAN_HARMONIC, -1, wall) == -1
            assert pack(lv.ptr, p, H.WHERE_HOST, H.MEAN_HARMONIC, 5, None) == -1
            assert pack(lvp.ptr, p, H.WHERE_HOST, H.MEAN_HARMONIC, 5, wall) == -1
            assert all(np.isnan(lv.read_all(vid)).all() for vid in BETAS)
            assert (mem.get(wall, (6, n, n)) == SENTINEL).all()
            out = np.full((n, n, n), np.nan)
            sens, o = lib.hpgmg_dense_unpack_cell_sensitivity, out.ctypes.data
            assert sens(lv.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, o, H.WHERE_HOST) == 0
            assert np.isfinite(out).all()
            out[:] = np.nan
            assert sens(lv.ptr, U_ID, LAM_ID, None, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, None, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, LAM_ID, p, 2, None, A, B, 0, None, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, -1, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, lv.num_vectors, p, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 5, None, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 64, wall, None, None, o, H.WHERE_HOST) == -1
            assert sens(lv.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, None, A, B, 0, None, None, None, o, 2) == -1
            assert sens(lvp.ptr, U_ID, LAM_ID, p, H.MEAN_HARMONIC, wall, A, B, 0, None, None, None, o, H.WHERE_HOST) == -1      # data on a periodic level
            assert np.isnan(out).all()
        finally:
            mem.free()


def test_torch_tensors_and_autograd(libs):
    """A child process that imports torch first: set_cell_coefficients and cell_sensitivity on tensors equal the NumPy path bitwise, out= is written in
    place, the gradients of hpgmg_amd.autograd.solve_cells are lam, -d_alpha and -d_k of the manual composition, bitwise, its three errors raise, and
    k.grad agrees with the face mean written in torch and fed to autograd.solve."""
    worker = os.path.join(ROOT, "tests", "user_cells_torch_worker.py")
    out = subprocess.run([sys.executable, worker], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "torch worker ok" in out.stdout, out.stdout + out.stderr
