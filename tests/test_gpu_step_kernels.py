"""The two passes of the implicit time march (kernels/dense_step.hip; include/hpgmg_operators.h hpgmg_step_rhs / hpgmg_step_rate) at
the edges of their launch shape, three ways: the HIP plugin against the oracle's host default (host/hooks_host.inc) over the WHOLE padded boxes of
EVERY vector of the level -- ghost cells, row padding and vectors that are no operand come back byte for byte as written --, and both against a
NumPy float64 restatement of include/hpgmg_step_math.h.  Every build has -ffp-contract=off and NumPy evaluates one operation per call, so all three
are the same bits: nothing here has a tolerance.

The launch shape, from step_grid() (kStepThreads = 256 cells per workgroup, kStepMaxBlocks = 4096):
    per_box = ceil(side^3 / 256),  gridDim.y = min(boxes, 4096),  cap = 4096 / gridDim.y,  gridDim.x = min(per_box, cap)
    a workgroup makes ceil(per_box / gridDim.x) trips of the x stride (lane q, then q + 256 gridDim.x, ...), a grid row ceil(boxes / gridDim.y)
    boxes; step_rate leaves gridDim.x * gridDim.y partial maxima for final_max_kernel.  step_offset() divides when the side is no power of two.

    (boxes per side, side)  boxes  per_box  gridDim.y   cap  gridDim.x  x trips  boxes per row  partials  side a power of two
    (2, 64)                     8     1024          8   512        512        2              1      4096  yes      (N = 128 in boxes of 64)
    (1, 104)                    1     4394          1  4096       4096        2              1      4096  no: the divide path; 298 workgroups make a second trip
    (3, 12)                    27        7         27   151          7        1              1       189  no; 1728 = 6 * 256 + 192: the last workgroup is partly live
    (1, 6)                      1        1          1  4096          1        1              1         1  no; 216 of 256 lanes live
    (17, 2)                  4913        1       4096     1          1        1              2      4096  yes; 817 grid rows take a second box; 8 of 256 lanes live
    (1, 1)                      1        1          1  4096          1        1              1         1  yes; one cell
The shapes of tests/test_gpu_user_step.py stay at one trip, one box per row and at most 1024 partials.  A cell that only the second x trip visits
has q >= 256 gridDim.x: 131072 at (2, 64), 1048576 at (1, 104); a box that only the second trip over the boxes visits has index >= 4096.

step_rate's maximum is placed by construction (one huge residual), so a lost trip or partial changes the returned value and not only the array.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
from test_gpu_operators import make_pair

pytestmark = pytest.mark.gpu

VARIANT = "7pt-cheby-helm"
VECTORS = 14                              # as a marching solver's finest level: u_old and w are the two vectors past the reserved ones
F_ID, U_ID, R_ID, UOLD_ID, W_ID = H.VECTOR_F, H.VECTOR_U, H.VECTOR_TEMP, 12, 13
A, C = 1.0 / (0.6 * 2e-3), 0.4 / 0.6      # theta = 0.6, dt = 2e-3:  a = 1 / (theta dt),  c = (1 - theta) / theta
HUGE = 1.0e6                              # a residual no other cell comes near: |w| <= 1 + a * 1.5 * 2 + c < 3000 elsewhere
GEOMS = [(2, 64), (1, 104), (3, 12), (1, 6), (17, 2), (1, 1)]
SECOND_X_TRIP = {(2, 64): 256 * 512, (1, 104): 256 * 4096}      # the first cell index q of a box that only the second trip of the x stride visits
# (geometry, where the largest |w| sits): Pair.place() turns the name into (box, cell)
PLACES = [(g, p) for g in GEOMS for p in ("first", "last", "second-x-trip", "box-4500")
          if p in ("first", "last") or (p == "second-x-trip" and g in SECOND_X_TRIP) or (p == "box-4500" and g == (17, 2))]


def _id(v):
    return f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v)


class Pair:
    """The two levels of one geometry, their seeded content and the raw offsets of the interior cells in the kernels' order (k, j, i)."""

    def __init__(self, hip, oracle, geom):
        self.geom = geom
        self.lh, self.lo = make_pair(hip, oracle, VARIANT, *geom, seed=31 + geom[1], vectors=VECTORS)
        lv = self.lh
        assert lv.num_vectors == VECTORS > H.VECTOR_ALPHA and lv.num_boxes == geom[0] ** 3 and lv.box_dim == geom[1]
        self.init = [lv.read_all(v) for v in range(VECTORS)]      # make_pair wrote the same into the oracle's level: check_all compares the two
        d, g = lv.box_dim, lv.ghosts
        k, j, i = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
        self.cells = ((i + g) + (j + g) * lv.jStride + (k + g) * lv.kStride).ravel()      # cells[q]: raw offset of cell q of a box
        self.dirty = set()

    def load(self, changes=None):
        """Both levels back to the seeded content, then `changes`: {vector id: (boxes, volume) array}.  Returns what the levels now hold."""
        now = list(self.init)
        for v, arr in (changes or {}).items():
            now[v] = arr
        for v in sorted(self.dirty | set(changes or {})):
            for lv in (self.lh, self.lo):
                lv.write_all(v, now[v])
        self.dirty = set(changes or {})
        return now

    def place(self, where):
        lv = self.lh
        cells = lv.box_dim ** 3
        if where == "first":
            return 0, 0
        if where == "last":
            return lv.num_boxes - 1, cells - 1
        if where == "second-x-trip":
            q = SECOND_X_TRIP[self.geom] + 77
            assert q < cells
            return lv.num_boxes // 2, q
        assert where == "box-4500" and lv.num_boxes > 4500
        return 4500, 5

    def destroy(self):
        self.lh.destroy(); self.lo.destroy()


_pairs = {}


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom): the levels of one geometry, made once and kept for the module (4913 boxes take seconds to fill box by box)."""
    def get(geom):
        if geom not in _pairs:
            _pairs[geom] = Pair(hip, oracle, geom)
        return _pairs[geom]
    return get


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    while _pairs:
        _pairs.popitem()[1].destroy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def check_all(P, expect):
    """Every vector of both levels over the whole padded boxes, each read once: HIP and oracle hold the same bits (what test_gpu_operators.same
    asks, and stricter: a NaN must be the same NaN), and these are the bits `expect` says."""
    for v in range(VECTORS):
        got_h, got_o = P.lh.read_all(v), P.lo.read_all(v)
        bad = np.argwhere(bits(got_h) != bits(got_o))
        assert bad.size == 0, f"vector {v}: HIP and oracle differ at (box, raw offset) {bad[:5].tolist()} ..."
        bad = np.argwhere(bits(got_h) != bits(expect[v]))
        assert bad.size == 0, f"vector {v} differs from the restatement at (box, raw offset) {bad[:5].tolist()} ..."


def rate_expected(P, now):
    """The restatement of step_rate_cell on the interiors; every other cell and vector as written."""
    q = P.cells
    al, r, u, uold, w = (now[v][:, q] for v in (H.VECTOR_ALPHA, R_ID, U_ID, UOLD_ID, W_ID))
    wn = (r + (A * al) * (u - uold)) - C * w
    expect = list(now)
    expect[W_ID] = now[W_ID].copy()
    expect[W_ID][:, q] = wn
    return expect, wn


def call_rate(lv):
    out = ctypes.c_double(-1.0)
    lv.b.lib.hpgmg_step_rate(lv.ptr, W_ID, R_ID, U_ID, UOLD_ID, A, C, ctypes.byref(out))
    return out.value


@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_step_rhs(pair_of, geom):
    """F = F + ((a alpha) u + c w) and u_old = u on every interior cell of every box, and nothing else: at (2, 64) and (1, 104) half and a
    fifteenth of the cells are written by the second trip of the x stride, at (17, 2) the boxes from 4096 on by the second trip over the boxes."""
    P = pair_of(geom)
    now = P.load()
    P.dirty |= {F_ID, UOLD_ID}
    for lv in (P.lh, P.lo):
        lv.b.lib.hpgmg_step_rhs(lv.ptr, F_ID, U_ID, UOLD_ID, W_ID, A, C)
    q = P.cells
    F, al, u, w = (now[v][:, q] for v in (F_ID, H.VECTOR_ALPHA, U_ID, W_ID))
    expect = list(now)
    expect[F_ID], expect[UOLD_ID] = now[F_ID].copy(), now[UOLD_ID].copy()
    expect[F_ID][:, q] = F + ((A * al) * u + C * w)
    expect[UOLD_ID][:, q] = u
    assert not np.array_equal(expect[F_ID], now[F_ID])
    check_all(P, expect)


@pytest.mark.parametrize("geom,where", PLACES, ids=_id)
def test_step_rate_and_where_its_maximum_sits(pair_of, geom, where):
    """w = (r + (a alpha) (u - u_old)) - c w, and the returned maximum is np.abs(w).max() exactly, wherever the largest |w| sits: in the first
    cell of the first box, the last of the last, a cell of the second x trip, a box of the second trip over the boxes."""
    P = pair_of(geom)
    box, cell = P.place(where)
    r = P.init[R_ID].copy()
    r[box, P.cells[cell]] = -HUGE
    now = P.load({R_ID: r})
    P.dirty.add(W_ID)
    got = [call_rate(lv) for lv in (P.lh, P.lo)]
    expect, wn = rate_expected(P, now)
    want = np.abs(wn).max()
    assert np.unravel_index(np.abs(wn).argmax(), wn.shape) == (box, cell) and want > 0.9 * HUGE
    assert got == [want, want], (got, want)
    check_all(P, expect)


@pytest.mark.parametrize("geom", [(2, 64), (3, 12)], ids=_id)
def test_step_rate_with_a_nan(pair_of, geom):
    """A NaN in r lands in w on both backends alike and never becomes the maximum: that is the largest finite |w|, which sits elsewhere."""
    P = pair_of(geom)
    lv = P.lh
    r = P.init[R_ID].copy()
    r[lv.num_boxes - 1, P.cells[lv.box_dim ** 3 // 3]] = np.nan
    r[0, P.cells[7]] = HUGE
    now = P.load({R_ID: r})
    P.dirty.add(W_ID)
    got = [call_rate(lv) for lv in (P.lh, P.lo)]
    expect, wn = rate_expected(P, now)
    assert np.isnan(wn).sum() == 1 and np.isnan(wn[lv.num_boxes - 1, lv.box_dim ** 3 // 3])
    want = np.nanmax(np.abs(wn))
    assert want > 0.9 * HUGE and got == [want, want], (got, want)
    check_all(P, expect)


def test_refusals():
    """The launchers refuse, before anything is launched, an output that is also an operand, an id outside the level's vectors and a level without
    an alpha vector.  The level is hand-built and holds no box: its device pointers are null and never dereferenced."""
    K = H.load_kernels()
    L = ctypes.POINTER(H.HipLevel)
    K.hpgmg_hip_step_rhs.restype, K.hpgmg_hip_step_rhs.argtypes = ctypes.c_int, [L] + [ctypes.c_int] * 5 + [ctypes.c_double] * 2
    K.hpgmg_hip_step_rate.restype = ctypes.c_int
    K.hpgmg_hip_step_rate.argtypes = [L] + [ctypes.c_int] * 5 + [ctypes.c_double] * 2 + [ctypes.POINTER(ctypes.c_double)]
    lvl = H.HipLevel()
    lvl.dim, lvl.ghosts, lvl.jStride, lvl.kStride, lvl.volume, lvl.num_boxes = 8, 1, 10, 100, 1000, 0
    p = ctypes.byref(lvl)
    out = ctypes.c_double(-1.0)

    def rhs(nv, F, u, uold, w):
        return K.hpgmg_hip_step_rhs(p, nv, F, u, uold, w, A, C)

    def rate(nv, w, r, u, uold):
        out.value = -1.0
        st = K.hpgmg_hip_step_rate(p, nv, w, r, u, uold, A, C, ctypes.byref(out))
        assert out.value == 0.0
        return st

    assert rhs(VECTORS, F_ID, U_ID, UOLD_ID, W_ID) == 0 and rate(VECTORS, W_ID, R_ID, U_ID, UOLD_ID) == 0      # the ids of the tests above pass
    for ids in [(U_ID, U_ID, UOLD_ID, W_ID), (UOLD_ID, U_ID, UOLD_ID, W_ID), (W_ID, U_ID, UOLD_ID, W_ID),      # F is u, u_old, w
                (F_ID, U_ID, U_ID, W_ID), (F_ID, U_ID, W_ID, W_ID)]:                                         # u_old is u, w
        assert rhs(VECTORS, *ids) != 0, ids
    for ids in [(R_ID, R_ID, U_ID, UOLD_ID), (U_ID, R_ID, U_ID, UOLD_ID), (UOLD_ID, R_ID, U_ID, UOLD_ID)]:      # w is r, u, u_old
        assert rate(VECTORS, *ids) != 0, ids
    for slot in range(4):
        for bad in (VECTORS, VECTORS + 50, -1):
            ids = [F_ID, U_ID, UOLD_ID, W_ID]
            ids[slot] = bad
            assert rhs(VECTORS, *ids) != 0, ids
            ids = [W_ID, R_ID, U_ID, UOLD_ID]
            ids[slot] = bad
            assert rate(VECTORS, *ids) != 0, ids
    for nv in (H.VECTOR_ALPHA, 5, 0):                                                                        # no alpha vector
        assert rhs(nv, 2, 1, 3, 4) != 0 and rate(nv, 3, 0, 1, 4) != 0, nv
    assert rhs(H.VECTOR_ALPHA + 1, 2, 1, 3, 4) == 0 and rate(H.VECTOR_ALPHA + 1, 3, 0, 1, 4) == 0
