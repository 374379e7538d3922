"""The boundary-value hooks one by one on the MI355X (include/hpgmg_operators.h hpgmg_boundary_flux / _flux_faces / _flux_robin / _restrict / _lift /
_interp / _interp_faces / _interp_robin): on every level and adjacent level pair of three solvers the HIP kernels (kernels/dense_boundary.hip) leave
the bytes of the host defaults (host/hooks_host.inc, in the CPU oracle): the whole 6 n^2 array, every padded box of the vector.  The whole-solve
tests compare them only through a solve.  The level chains (CHAINS):
    16 in boxes of 8    2 x 2 x 2 boxes of 8^3 -- box faces that are no domain faces, every edge and corner -- and a chain of levels down to one cell
                        (the n < 2 rule; six Neumann walls stop at 2^3)
    48 in boxes of 16   48/16, 24/8, 12/4, 6/2 in 27 boxes each (3 per side: a middle box on no wall), then 3/3 in one box: interp and lift across the
                        change from 27 boxes to one box of an odd side
    104                 104/8, 52/4, 26/2 in 2197 boxes each, then 13/13 in one box: 1014 face positions (the last of 4 workgroups partly live), an odd side
The Robin forms run on every level with a kappa array that is >= 0 with some entries exactly 0.0, and are held to what the header promises: an all-zero
kappa array gives the _faces bytes, mask 0 the plain hook's.  The search branch of bnd_coarse_cell (coarse boxes not in i-fastest order, which no solver
builds) runs on hand-built levels in test_interp_robin_finds_the_owner_of_a_coarse_cell.

Both sides compile their arithmetic from include/hpgmg_boundary_math.h, so this is no independent check of the formulas (test_oracle_user_*.py
hold those to SciPy assemblies and manufactured solutions): it checks what each side keeps of its own -- the reads of the level's vectors, the
indexing, which lane or loop owns a cell, the launch mapping.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_amd.problem import Solver
from hpgmg_testlib import Backend
from test_gpu_user_problem import DeviceArrays
from user_neumann_lib import ALL, CORNERS, ONE, SIDES, mask_of

pytestmark = pytest.mark.gpu

# (N, box_dim of Solver): the level sizes, the boxes per level, the last level's size under six Neumann walls (else the last of the sizes)
CHAINS = {
    (16, 8): ([16, 8, 4, 2, 1], None, 2),
    (48, 16): ([48, 24, 12, 6, 3], [27, 27, 27, 27, 1], 3),
    (104, None): ([104, 52, 26, 13], [2197, 2197, 2197, 1], 13),
}
B_COEF = 1.5                 # the operator's b of the flux weights
ID = H.VECTOR_U              # the work vector: present on every level


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    return hip, Backend.oracle().lib, K


class HostArrays:
    """DeviceArrays for the oracle, whose plugin memory is host memory."""

    def __init__(self):
        self.held = {}

    def put(self, a):
        a = a.copy()
        self.held[a.ctypes.data] = a
        return a.ctypes.data

    def get(self, p, shape):
        return self.held[p].reshape(shape).copy()

    def free(self):
        self.held = {}


class _Level:
    def __init__(self, lib, L, arrays, rng):
        """g, the wall betas and the work vector (whole padded boxes) from the generator; phi, phi_faces hold the two fluxes once they have run."""
        info = (ctypes.c_int * H.INFO_COUNT)()
        lib.hpgmg_level_info(L, info)
        self.lib, self.L, self.arrays = lib, L, arrays
        n = self.n = info[H.INFO_DIM]
        self.vol, self.boxes = info[H.INFO_VOLUME], info[H.INFO_NUM_MY_BOXES]
        self.g, self.wall = self.put(rng.random((6, n, n)) * 4.0 - 2.0), self.put(0.5 + rng.random((6, n, n)))
        self.v = rng.random((self.boxes, self.vol)) * 2.0 - 1.0
        self.phi, self.phi_faces, self.phi_robin = self.zeros(), self.zeros(), self.zeros()
        krng = np.random.default_rng(4321 + n)                      # a generator of its own: the arrays above stay what they were
        kappa = krng.random((6, n, n)) * 3.0
        kappa[krng.random((6, n, n)) < 0.25] = 0.0
        self.kappa, self.kappa_zero = self.put(kappa), self.zeros()

    def put(self, a):
        return self.arrays.put(a)

    def zeros(self):
        return self.put(np.zeros((6, self.n, self.n)))

    def get(self, p):
        return self.arrays.get(p, (6, self.n, self.n))

    def reset(self):
        for box in range(self.boxes):
            self.lib.hpgmg_level_write_vector(self.L, box, ID, self.v[box].ctypes.data)

    def read(self):
        out = np.empty((self.boxes, self.vol))
        for box in range(self.boxes):
            self.lib.hpgmg_level_read_vector(self.L, box, ID, out[box].ctypes.data)
        return out


def _hooks(lib, chain, faces, arrays):
    """Every hook on every level and level pair: [(what, array after the call)]."""
    mask = mask_of(faces)
    rng = np.random.default_rng(1234 + mask)
    out = []
    (N, BOX), (sizes, boxes, bottom_neumann) = chain, CHAINS[chain]
    with Solver(N, **({} if BOX is None else {"box_dim": BOX}), bc=faces, lib=lib) as s:
        hs = lib.hpgmg_user_solver_of(s._ptr)
        levels = [_Level(lib, lib.hpgmg_solver_level(hs, l), arrays, rng) for l in range(lib.hpgmg_solver_num_levels(hs))]
        if chain == (16, 8):
            assert [X.n for X in levels] == [N >> l for l in range(len(levels))] and levels[0].boxes == 8
            assert levels[-1].n == (2 if mask == 63 else 1)
        assert [X.n for X in levels] == sizes[:len(levels)] and levels[-1].n == (bottom_neumann if mask == 63 else sizes[-1])
        assert boxes is None or [X.boxes for X in levels] == boxes[:len(levels)]
        for l, X in enumerate(levels):
            assert lib.hpgmg_boundary_flux(X.L, X.phi, X.g, B_COEF) == 0
            plain = X.get(X.phi)
            out.append((f"flux level {l}", plain))
            assert lib.hpgmg_boundary_flux_faces(X.L, X.phi_faces, X.g, B_COEF, mask, X.wall) == 0
            out.append((f"flux_faces level {l}", X.get(X.phi_faces)))
            if mask == 0:
                assert np.array_equal(out[-1][1], plain), f"flux_faces with mask 0 is not flux on level {l}"
            X.reset()
            lib.hpgmg_boundary_lift(X.L, ID, X.phi_faces, None, -1.0)      # the per-face flux: the plain one is 0 on a Neumann wall, whose own beta is 0
            out.append((f"lift level {l}", X.read()))
            assert not np.array_equal(out[-1][1], X.v)
            assert lib.hpgmg_boundary_flux_robin(X.L, X.phi_robin, X.g, B_COEF, mask, X.wall, X.kappa) == 0
            out.append((f"flux_robin level {l}", X.get(X.phi_robin)))
            if mask == 0:
                assert out[-1][1].tobytes() == plain.tobytes(), f"flux_robin with mask 0 is not flux on level {l}"
            X.reset()
            lib.hpgmg_boundary_lift(X.L, ID, X.phi_robin, None, -1.0)
            out.append((f"lift from the Robin flux level {l}", X.read()))
            assert not np.array_equal(out[-1][1], X.v)
            scratch = X.zeros()
            assert lib.hpgmg_boundary_flux_robin(X.L, scratch, X.g, B_COEF, mask, X.wall, X.kappa_zero) == 0
            assert X.get(scratch).tobytes() == X.get(X.phi_faces).tobytes(), f"flux_robin with kappa = 0 is not flux_faces on level {l}"
        for l, (F, C) in enumerate(zip(levels, levels[1:])):
            g_c = C.zeros()
            lib.hpgmg_boundary_restrict(C.L, g_c, F.L, F.g)
            out.append((f"restrict level {l} -> {l + 1}", C.get(g_c)))
            C.reset()
            lib.hpgmg_boundary_lift(C.L, ID, C.phi_faces, F.phi_faces, 1.0)
            out.append((f"lift with phi_fine level {l + 1}", C.read()))
            C.reset()                                            # the coarse iterate that interp_faces reads
            F.reset()
            lib.hpgmg_boundary_interp(F.L, ID, C.L, C.g)
            plain = F.read()
            out.append((f"interp level {l + 1} -> {l}", plain))
            assert not np.array_equal(plain, F.v)
            F.reset()
            lib.hpgmg_boundary_interp_faces(F.L, ID, C.L, C.g, mask)
            out.append((f"interp_faces level {l + 1} -> {l}", F.read()))
            if mask == 0:
                assert np.array_equal(out[-1][1], plain), f"interp_faces with mask 0 is not interp onto level {l}"
            faces_bytes = out[-1][1].tobytes()
            F.reset()
            lib.hpgmg_boundary_interp_robin(F.L, ID, C.L, C.g, mask, C.kappa)
            out.append((f"interp_robin level {l + 1} -> {l}", F.read()))
            if mask == 0:
                assert out[-1][1].tobytes() == plain.tobytes(), f"interp_robin with mask 0 is not interp onto level {l}"
            F.reset()
            lib.hpgmg_boundary_interp_robin(F.L, ID, C.L, C.g, mask, C.kappa_zero)
            assert F.read().tobytes() == faces_bytes, f"interp_robin with kappa = 0 is not interp_faces onto level {l}"
    return out


WALL_SETS = list(zip(["mask0", "one", "sides", "corners", "all"], [("dirichlet",) * 6, ONE, SIDES, CORNERS, ALL]))
# (the 16 / 8 cases keep the ids they had before the other chains came)
CASES = [pytest.param(chain, faces, id=name if chain == (16, 8) else f"{chain[0]}-{name}") for chain in CHAINS for name, faces in WALL_SETS]


@pytest.mark.parametrize("chain,faces", CASES)
def test_each_hook_equals_the_host_default(libs, chain, faces):
    hip, oracle, K = libs
    ref = _hooks(oracle, chain, faces, HostArrays())
    D = DeviceArrays(K)
    try:
        got = _hooks(hip, chain, faces, D)
    finally:
        D.free()
    assert [what for what, _ in got] == [what for what, _ in ref]
    for (what, a), (_, b) in zip(got, ref):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), what          # the bytes too: the sign of a zero is part of the contract


# ---------------------------------------------------------------- the search branch of bnd_coarse_cell
def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class _HandLevel:
    """A hpgmg_hip_level built by hand in device memory the test allocates, with the geometry and content of an oracle level: `order` lists the
    oracle's boxes in the order this level keeps them (base pointers and lows permuted together)."""

    def __init__(self, K, D, lv, order):
        self.K, self.lv, self.order = K, lv, order
        self.bytes_per_box = lv.num_vectors * lv.volume * 8
        self.dev = D.empty(lv.num_boxes * self.bytes_per_box)
        base = np.array([self.dev + b * self.bytes_per_box for b in order], dtype=np.uint64)
        low = np.array([lv.box_low(b) for b in order], dtype=np.int32)
        self.level = H.HipLevel(D.put(base), D.put(low), lv.num_boxes, lv.box_dim, lv.ghosts, lv.jStride, lv.kStride, lv.volume, lv.dim, lv.dim, lv.dim, 0)

    def write(self, content):
        """content[vector][box]: the oracle's padded boxes, in the oracle's box order."""
        host = np.ascontiguousarray(np.stack(content, axis=1))      # (box, vector, volume): box b of the oracle lives at dev + b * bytes_per_box
        assert host.nbytes == self.lv.num_boxes * self.bytes_per_box
        assert self.K.hpgmg_hip_memcpy_h2d(self.dev, host.ctypes.data, host.nbytes) == 0

    def read(self, vid):
        host = np.empty((self.lv.num_boxes, self.lv.num_vectors, self.lv.volume))
        assert self.K.hpgmg_hip_memcpy_d2h(host.ctypes.data, self.dev, host.nbytes) == 0
        return host[:, vid].copy()


def test_interp_robin_finds_the_owner_of_a_coarse_cell(libs):
    """hpgmg_hip_boundary_interp_robin called directly on a fine 8^3 cube in 8 boxes of 4 and its coarse 4^3 cube in 8 boxes of 2: the coarse boxes in
    i-fastest order with boxes_per_side = 2 (the box formula), the same with boxes_per_side = 0 (the search), and the coarse boxes listed in a permuted
    order with boxes_per_side = 0 -- the owner of the last in-range cell (3, 3, 3) is then the second box listed, not the last.  All three leave the
    bytes of the oracle's hpgmg_boundary_interp_robin on levels of the same shape and content; boxes_per_side = 3 is refused, the fine vector untouched."""
    _, _, K = libs
    ob = Backend.oracle()
    ob.configure(op=H.OP_7PT, smoother=H.SMOOTH_CHEBY, helmholtz=1, variable_coeff=1)
    lf, lc = ob.level(2, 4, num_vectors=2, h=1.0 / 8), ob.level(2, 2, num_vectors=2, h=1.0 / 4)
    vid, mask, nc = 1, 0b011010, 4
    call = K.hpgmg_hip_boundary_interp_robin
    call.restype = ctypes.c_int
    call.argtypes = [ctypes.POINTER(H.HipLevel), ctypes.c_int, ctypes.POINTER(H.HipLevel), ctypes.c_int, ctypes.c_void_p, ctypes.c_double, ctypes.c_int,
                     ctypes.c_void_p]
    rng = np.random.default_rng(88)
    fine = [rng.random((8, lf.volume)) * 2.0 - 1.0 for _ in range(2)]
    coarse = [rng.random((8, lc.volume)) * 2.0 - 1.0 for _ in range(2)]
    g_c, kappa_c = rng.random((6, nc, nc)) * 4.0 - 2.0, rng.random((6, nc, nc)) * 3.0
    kappa_c[1, 0, :] = 0.0
    D, mem = DeviceArrays(K), HostArrays()
    try:
        for v in range(2):
            lf.write_all(v, fine[v]); lc.write_all(v, coarse[v])
        ob.lib.hpgmg_boundary_interp_robin(lf.ptr, vid, lc.ptr, mem.put(g_c), mask, mem.put(kappa_c))
        want = lf.read_all(vid)
        assert not _same_bytes(want, fine[vid])
        assert [lc.box_low(b) for b in range(8)] == [(2 * (b % 2), 2 * ((b // 2) % 2), 2 * (b // 4)) for b in range(8)]      # i-fastest
        Lf = _HandLevel(K, D, lf, list(range(8)))
        pg, pk = D.put(g_c), D.put(kappa_c)
        permuted = [3, 7, 0, 5, 1, 6, 2, 4]
        assert lc.box_low(permuted[1]) == (2, 2, 2) and permuted[-1] != 7
        for order, boxes_per_side in ((list(range(8)), 2), (list(range(8)), 0), (permuted, 0)):
            Lc = _HandLevel(K, D, lc, order)
            Lc.write(coarse)
            Lf.write(fine)
            assert call(ctypes.byref(Lf.level), vid, ctypes.byref(Lc.level), boxes_per_side, pg, lc.h, mask, pk) == 0, (order, boxes_per_side)
            got = Lf.read(vid)
            assert _same_bytes(got, want), (order, boxes_per_side, np.argwhere(got != want)[:5].tolist())
            assert _same_bytes(Lf.read(0), fine[0])                          # the other vector of the level is not touched
        Lf.write(fine)
        assert call(ctypes.byref(Lf.level), vid, ctypes.byref(Lc.level), 3, pg, lc.h, mask, pk) != 0
        assert _same_bytes(Lf.read(vid), fine[vid])
    finally:
        D.free(); mem.free()
        lf.destroy(); lc.destroy()
