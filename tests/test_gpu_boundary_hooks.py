"""The boundary-value hooks one by one on the MI355X (include/hpgmg_operators.h hpgmg_boundary_flux / _flux_faces / _restrict / _lift / _interp /
_interp_faces): on every level and adjacent level pair of a 16^3 solver in 2 x 2 x 2 boxes of 8^3 -- box faces that are no domain faces, every
edge and corner, and a chain of levels down to one cell (the n < 2 rule; six Neumann walls stop at 2^3) -- the HIP kernels
(kernels/dense_boundary.hip) leave the bytes of the host defaults (host/hooks_host.inc, in the CPU oracle): the whole 6 n^2 array, every padded box
of the vector.  The whole-solve tests compare them only through a solve.

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

N, BOX = 16, 8
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
        self.phi, self.phi_faces = self.zeros(), self.zeros()

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


def _hooks(lib, faces, arrays):
    """Every hook on every level and level pair: [(what, array after the call)]."""
    mask = mask_of(faces)
    rng = np.random.default_rng(1234 + mask)
    out = []
    with Solver(N, box_dim=BOX, bc=faces, lib=lib) as s:
        hs = lib.hpgmg_user_solver_of(s._ptr)
        levels = [_Level(lib, lib.hpgmg_solver_level(hs, l), arrays, rng) for l in range(lib.hpgmg_solver_num_levels(hs))]
        assert [X.n for X in levels] == [N >> l for l in range(len(levels))] and levels[0].boxes == 8
        assert levels[-1].n == (2 if mask == 63 else 1)
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
    return out


@pytest.mark.parametrize("faces", [("dirichlet",) * 6, ONE, SIDES, CORNERS, ALL], ids=["mask0", "one", "sides", "corners", "all"])
def test_each_hook_equals_the_host_default(libs, faces):
    hip, oracle, K = libs
    ref = _hooks(oracle, faces, HostArrays())
    D = DeviceArrays(K)
    try:
        got = _hooks(hip, faces, D)
    finally:
        D.free()
    assert [what for what, _ in got] == [what for what, _ in ref]
    for (what, a), (_, b) in zip(got, ref):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), what          # the bytes too: the sign of a zero is part of the contract
