"""BLAS-1 and every reduction that returns a maximum or an ordered sum, held to the CPU oracle at the edges of their launch shape (kernels/blas1.hip,
kernels/reduce.hip final_max_kernel and the result slot, kernels/pcg.hip pcg_update_kernel, the fused residual + norm of kernels/stencil7_wide.hpp (launched from kernels/stencil.hip), stencil27_tile.hpp and fv4_tile.hpp).  Every
comparison is bitwise: all builds have -ffp-contract=off, a maximum is exact in any order and the sums have one order (misc.c:261-269).  The NumPy
restatements and the launch arithmetic are tests/reduction_lib.py's, pinned on the CPU by tests/test_oracle_reductions.py; every test asserts the path
it claims against those plans.

A MAXIMUM IS PLACED: the data is in [-1, 1] and one cell holds +-HUGE (1e6; a value worked out from the data where the kernel forms a residual), at
each position that only one trip, row in flight, lane, workgroup or partial of the launch reaches -- so a lost one changes the returned value.  On
random data the maximum sits wherever it happens to sit and such a loss passes with probability 1 - (share skipped).

norm -- hpgmg_hip_norm_max: nblk = ceil(boxes side^2 / 4); nblk <= 64: absmax_small_kernel; else per_box = ceil(side^2 / 4), halved while per_box boxes
> 4096; waves = 4 per_box; a wave takes rows w + u waves (u = 0..3, four rows in flight) + 4 waves t (the row0 trips); lanes stride i by 64.

    geom      path            per_box         partials  what it reaches
    (1, 1)    absmax_small    nblk 1                    idle lanes, fewer rows than waves
    (1, 6)    absmax_small    nblk 9
    (1, 16)   absmax_small    nblk 64                   the <= 64 edge
    (2, 8)    absmax_kernel   16              128       one real row of the four in flight
    (3, 12)   absmax_kernel   36              972       the divide path; final_max: lanes 0-203 take the 4-way loop, all lanes the tail (156 partials)
    (1, 104)  absmax_kernel   2704            2704      rows longer than a wave, one row per wave
    (1, 136)  absmax_kernel   4624 -> 2312    2312      halved once, two real rows per wave, three lane trips
    (2, 64)   absmax_kernel   1024 -> 512     4096      halving stops at exactly 4096
    (4, 64)   absmax_kernel   1024 -> 64      4096      all four rows real, four row0 trips
    (17, 2)   absmax_kernel   1               4913      per_box cannot shrink; final_max with n > 4096

dot, mean -- ordered_sum: tiles of side x 8 x 8, ntiles = ceil(side / 8)^2 boxes; <= 64: tile_sum_kernel<true>; else by side: <= 128 wave<2>, <= 256
wave<4>, <= 512 wave<8> (2 x 8 x side x 8 bytes of dynamic LDS), above tile_sum_kernel<false>; then ordered_sum_kernel in waves of 64 partials.

    geom      ntiles  kernel           what it reaches
    (1, 6)    1       tile_sum<true>   a partial tile, lanes past ntiles
    (3, 4)    27      tile_sum<true>
    (1, 64)   64      tile_sum<true>   the <= 64 edge, all lanes live
    (3, 12)   108     wave<2>          tiles with nj = 4 and of 4 planes: 64 / 32 / 32 / 16 rows
    (5, 6)    125     wave<2>          36 rows: five groups, the last of 4 rows
    (1, 104)  169     wave<2>          second chunk with 40 lanes live; ordered_sum_kernel's tail of 41
    (1, 136)  289     wave<4>          third chunk with 8 lanes live
    (1, 264)  1089    wave<8>          fifth chunk with 8 lanes live; the LDS attribute call
    (1, 512)  4096    wave<8>          64 KiB of dynamic LDS exactly; mean only, one vector (1.1 GB)
    (1, 520)  4225    tile_sum<false>  + ordered_sum_kernel; mean only, one vector

Fused residual + norm, 7-point wide kernel (stencil7_wide_kernel, launch_wide_fused): a workgroup owns 128 (i) x 16 (j) cells over a chunk of 16
planes; boxes ceil(side / 16) (side / 16) (side / 128) partials.  Tile forms: the 27-point kernel's tile is 64 (i) x 8 (j) over chunks of 32 planes at
(2, 64) (stencil27_tile.hpp, launch27: 128 partials), the 4th-order kernel's 64 (i) x 8 (j) over chunks of 8 planes (fv4_tile.hpp,
launch_fv4_tile_tj: 512 partials).  norm_copy_restrict_kernel: a wave owns a coarse row, a lane the 2 x 2 x 2 children of a coarse cell, lanes stride
ci by 64.  rebuild7_kernel: a wave per row, ceil(boxes side^2 / 4) partials.  pcg_update_kernel: a workgroup owns 256 columns c = i + side j of a
box over a segment of 16 planes: ceil(side^2 / 256) ceil(side / 16) boxes partials.

A level of one box of side <= 8 sends its BLAS-1 calls and scalars to small_ops_kernel (host/plugin_queue.c); that path is switched off for this
module, so that (1, 1), (1, 3) and (1, 6) reach the kernels named above.
"""
import contextlib
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import reduction_lib as R
from hpgmg_amd.problem import Solver
from hpgmg_testlib import VARIANTS, Level
from reduction_lib import HUGE, bits
from user_problem_lib import random_coefficients

pytestmark = pytest.mark.gpu


def _id(v):
    if isinstance(v, tuple):
        return "x".join(str(x) for x in v)
    return str(v)


@pytest.fixture(scope="module", autouse=True)
def _module(hip, oracle):
    hip.lib.hpgmg_set_small_ops.argtypes = [ctypes.c_int]
    hip.lib.hpgmg_set_ghost_free.argtypes = [ctypes.c_int]
    hip.lib.hpgmg_set_small_ops(0)
    hip.lib.hpgmg_set_ghost_free(1)
    yield
    hip.lib.hpgmg_set_small_ops(1)
    while _kept:
        _kept.popitem()[1].destroy()


def configure(hip, oracle, variant):
    for be in (hip, oracle):
        be.configure(**VARIANTS[variant])


# ---------------------------------------------------------------------------------------------------------------- plain levels of a few vectors
class Pair:
    """The HIP and the oracle level of one geometry with `vectors` vectors and the seeded content of those a test filled."""

    def __init__(self, hip, oracle, geom, vectors):
        configure(hip, oracle, "7pt-cheby-helm")          # one ghost cell; BLAS-1 does not depend on the operator
        self.geom = geom
        self.lh, self.lo = (be.level(*geom, num_vectors=vectors) for be in (hip, oracle))
        lv = self.lh
        assert lv.num_vectors == vectors and lv.num_boxes == geom[0] ** 3 and lv.box_dim == geom[1]
        self.base, self._cells, self.abs0 = {}, None, None

    @property
    def cells(self):
        """(side, side, side) raw offsets of the interior cells (made on first use: the widest boxes never ask)"""
        if self._cells is None:
            self._cells = R.cell_offsets(self.lh)
        return self._cells

    def fill(self, vid, data):
        self.base[vid] = data
        for lv in (self.lh, self.lo):
            lv.write_all(vid, data)

    def plant(self, vid, box, offset, value):
        """One cell of one box changed on both levels (a single-box write; restore() puts the seeded box back)."""
        x = self.base[vid][box].copy()
        x[offset] = value
        for lv in (self.lh, self.lo):
            lv.write_raw(box, vid, x)

    def restore(self, vid, box):
        for lv in (self.lh, self.lo):
            lv.write_raw(box, vid, self.base[vid][box])

    def both(self, name, *args):
        return [getattr(lv.b.lib, name)(lv.ptr, *args) for lv in (self.lh, self.lo)]

    def destroy(self):
        self.lh.destroy(); self.lo.destroy()


_kept = {}


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom, vectors): the levels of one geometry, made once and kept for the module."""
    def get(geom, vectors, key=""):
        k = (geom, vectors, key)
        if k not in _kept:
            _kept[k] = Pair(hip, oracle, geom, vectors)
        return _kept[k]
    return get


def flush(P):
    for lv in (P.lh, P.lo):
        lv.b.lib.hpgmg_operators_flush()


def same_bits(lh, lo, vid, expect=None):
    got_h, got_o = lh.read_all(vid), lo.read_all(vid)
    bad = np.argwhere(bits(got_h) != bits(got_o))
    assert bad.size == 0, f"vector {vid}: HIP and oracle differ at (box, raw offset) {bad[:5].tolist()} ..."
    if expect is not None:
        bad = np.argwhere(bits(got_h) != bits(expect))
        assert bad.size == 0, f"vector {vid} differs from the restatement at (box, raw offset) {bad[:5].tolist()} ..."


# ---------------------------------------------------------------------------------------------------------------- 2. element-wise passes and fill
@pytest.mark.parametrize("geom", [(1, 72), (1, 136), (1, 3), (3, 12)], ids=_id)
def test_elementwise_passes_and_fill_at_rows_longer_than_a_wave(pair_of, geom):
    """add / mul / invert / scale / shift / zero / init / color / random_vector over whole padded boxes of every vector of the level, HIP == oracle ==
    the one-line NumPy expression: (1, 72) two lane trips with 8 lanes live in the second (fill_kernel: padded side 74), (1, 136) three trips,
    (1, 3) a last workgroup with one row of its four, (3, 12) a side that is no power of two."""
    P = pair_of(geom, R.EW_VECTORS)
    assert R.ceil_div(geom[1], 64) == {72: 2, 136: 3, 3: 1, 12: 1}[geom[1]] and R.ceil_div(geom[1] + 2 * P.lh.ghosts, 64) == {72: 2, 136: 3, 3: 1, 12: 1}[geom[1]]
    assert (geom[0] ** 3 * geom[1] ** 2) % R.ROWS_PER_BLOCK == {72: 0, 136: 0, 3: 1, 12: 0}[geom[1]]
    init = R.elementwise_fields(P.lh, 40 + geom[1])
    for v, x in enumerate(init):
        P.fill(v, x)
    for lv in (P.lh, P.lo):
        R.elementwise_calls(lv)
    flush(P)
    expect = R.elementwise_expected(P.lh, init)
    assert not np.array_equal(expect[9], init[9])
    for v in range(R.EW_VECTORS):
        same_bits(P.lh, P.lo, v, expect[v])


# ---------------------------------------------------------------------------------------------------------------- 3. norm
NORM_GEOMS = [(1, 1), (1, 6), (1, 16), (2, 8), (3, 12), (1, 104), (1, 136), (2, 64), (4, 64), (17, 2)]
NORM_PATH = {(1, 1): ("absmax_small", 1), (1, 6): ("absmax_small", 9), (1, 16): ("absmax_small", 64), (2, 8): ("absmax_kernel", 16), (3, 12): ("absmax_kernel", 36),
             (1, 104): ("absmax_kernel", 2704), (1, 136): ("absmax_kernel", 2312), (2, 64): ("absmax_kernel", 512), (4, 64): ("absmax_kernel", 64), (17, 2): ("absmax_kernel", 1)}
NORM_VECTORS = {(2, 64): 3, (1, 104): 3}      # error(1, 2) writes VECTOR_TEMP = 0; elsewhere the level is the one vector


def norm_places(geom):
    """{name: (box, k, j, i)}: where the plan says a cell exists that only one part of the launch reaches."""
    p = R.norm_plan(*geom)
    d, boxes, mid = geom[1], geom[0] ** 3, geom[0] ** 3 // 2
    out = {"first": (0, 0, 0, 0), "last": (boxes - 1, d - 1, d - 1, d - 1)}
    if p.lane_trips > 1:
        out["lane-trip-2"] = (mid, d // 3, d // 2, 64)                      # the first cell of the second trip of `for (i = lane; ...; i += 64)`
        out["lane-trip-last"] = (mid, d // 2, d // 3, 64 * (p.lane_trips - 1) + 1)
    if p.path == "absmax_kernel":
        for u in (1, 2, 3):                                                  # a row only row-in-flight u reaches: waves u <= row < waves (u + 1)
            if p.rows > u * p.waves:
                row = min(u * p.waves + 1, p.rows - 1)
                out[f"row-in-flight-{u}"] = (mid, row // d, row % d, d // 2)
        if p.row0_trips > 1:                                                 # a row only a later trip of the row0 loop reaches
            row = ROWS4 * p.waves + 1
            out["row0-trip-2"] = (mid, row // d, row % d, 1)
            row = ROWS4 * p.waves * (p.row0_trips - 1) + 3 * p.waves + 2
            out["row0-trip-last-u3"] = (mid, row // d, row % d, d - 2)
    if boxes > 2:
        out["middle-box-last-row"] = (mid, d - 1, d - 1, 0)
    if geom == (17, 2):
        out["box-4500"] = (4500, 1, 0, 1)
    return out


ROWS4 = R.ROWS_IN_FLIGHT
NORM_CASES = [(g, name) for g in NORM_GEOMS for name in norm_places(g)]


def norm_pair(pair_of, geom):
    P = pair_of(geom, NORM_VECTORS.get(geom, 1), "norm")
    if not P.base:
        for v in range(P.lh.num_vectors):
            P.fill(v, R.random_field(P.lh, 300 + 7 * geom[1] + v))
    return P


@pytest.mark.parametrize("geom,where", NORM_CASES, ids=_id)
def test_norm_wherever_the_maximum_sits(pair_of, geom, where):
    plan = R.norm_plan(*geom)
    assert (plan.path, plan.per_box if plan.path == "absmax_kernel" else plan.nblk) == NORM_PATH[geom]
    if geom == (1, 16):
        assert plan.nblk == R.SMALL_NORM_BLOCKS
    if geom == (2, 64):
        assert plan.per_box * plan.boxes == R.MAX_NORM_BLOCKS and plan.halvings == 1 and plan.rows_in_flight == 2
    if geom == (4, 64):
        assert plan.rows_in_flight == 4 and plan.row0_trips == 4 and plan.rows == 16 * plan.waves
    if geom == (3, 12):
        assert plan.divide and R.final_max_plan(plan.partials) == (204, 1, 156)
    if geom == (17, 2):
        assert plan.per_box == 1 and plan.partials == 4913 > 4096
    if geom == (1, 136):
        assert plan.halvings == 1 and plan.rows_in_flight == 2 and plan.lane_trips == 3
    if geom == (1, 104):
        assert plan.rows_in_flight == 1 and plan.lane_trips == 2 and plan.halvings == 0
    if geom == (2, 8):
        assert plan.rows_in_flight == 1 and plan.partials == 128
    P = norm_pair(pair_of, geom)
    box, k, j, i = norm_places(geom)[where]
    assert 0 <= box < plan.boxes and max(k, j, i) < geom[1]
    if where.startswith("row-in-flight"):
        u, row = int(where[-1]), k * geom[1] + j
        assert u * plan.waves <= row < (u + 1) * plan.waves
    if where.startswith("row0-trip"):
        assert k * geom[1] + j >= ROWS4 * plan.waves
    if where.startswith("lane-trip"):
        assert i >= 64
    value = HUGE if (NORM_CASES.index((geom, where)) % 2) else -HUGE
    P.plant(0, box, P.cells[k, j, i], value)
    try:
        got = P.both("norm", 0)
        if P.abs0 is None:
            P.abs0 = np.abs(R.interior(P.lh, P.base[0]))
        a, seeded = P.abs0, P.abs0[box, k, j, i]
        a[box, k, j, i] = abs(value)                                         # |what was written|
        try:
            assert np.unravel_index(a.argmax(), a.shape) == (box, k, j, i) and a.max() == HUGE
        finally:
            a[box, k, j, i] = seeded
        assert got == [HUGE, HUGE], (got, where)
    finally:
        P.restore(0, box)
    if where == "first":                                                     # and back on the seeded data: the maximum wherever it happens to sit
        got = P.both("norm", 0)
        assert got[0] == got[1] == R.abs_max(P.lh, P.base[0]) < 1.0


@pytest.mark.parametrize("geom", [(2, 64), (3, 12)], ids=_id)
def test_norm_with_a_nan(pair_of, geom):
    """A NaN never becomes the norm, on both backends alike: that is the largest other magnitude, which sits elsewhere."""
    P = norm_pair(pair_of, geom)
    d, last = geom[1], geom[0] ** 3 - 1
    q = d ** 3 // 3
    x = P.base[0][last].copy()
    x[P.cells.ravel()[q]] = np.nan
    for lv in (P.lh, P.lo):
        lv.write_raw(last, 0, x)
    P.plant(0, 0, P.cells.ravel()[7], HUGE)
    try:
        assert P.both("norm", 0) == [HUGE, HUGE]
    finally:
        P.restore(0, 0); P.restore(0, last)


@pytest.mark.parametrize("geom", [(2, 64), (1, 104)], ids=_id)
def test_error_of_two_vectors(pair_of, geom):
    """error(a, b) = norm(a - b), the difference left in VECTOR_TEMP: HIP == oracle == NumPy, with the largest difference in the last cell."""
    P = norm_pair(pair_of, geom)
    last = geom[0] ** 3 - 1
    P.plant(1, last, P.cells[-1, -1, -1], -HUGE)
    try:
        got = P.both("error", 1, 2)
        flush(P)
        a, b = R.interior(P.lh, P.base[1]), R.interior(P.lh, P.base[2])
        diff = 1.0 * a + (-1.0) * b
        diff[last, -1, -1, -1] = 1.0 * -HUGE + (-1.0) * b[last, -1, -1, -1]
        want = np.abs(diff).max()
        assert np.abs(diff).argmax() == diff.size - 1 and got == [want, want], (got, want)
        expect = P.base[0].copy()
        expect[:, P.cells] = diff
        same_bits(P.lh, P.lo, H.VECTOR_TEMP, expect)
    finally:
        P.restore(1, last)
        P.fill(0, P.base[0])


# ---------------------------------------------------------------------------------------------------------------- 4. dot, mean
SUM_GEOMS = [(1, 6), (3, 4), (1, 64), (3, 12), (5, 6), (1, 104), (1, 136), (1, 264)]
SUM_KERNEL = {(1, 6): (1, "tile_sum<true>"), (3, 4): (27, "tile_sum<true>"), (1, 64): (64, "tile_sum<true>"), (3, 12): (108, "wave<2>"), (5, 6): (125, "wave<2>"),
              (1, 104): (169, "wave<2>"), (1, 136): (289, "wave<4>"), (1, 264): (1089, "wave<8>"), (1, 512): (4096, "wave<8>"), (1, 520): (4225, "tile_sum<false>")}


def sum_plan_checked(geom):
    plan = R.sum_plan(*geom)
    assert (plan.ntiles, plan.kernel) == SUM_KERNEL[geom]
    if geom == (1, 64):
        assert plan.ntiles == R.SMALL_SUM_TILES
    if geom == (3, 12):
        assert plan.tile_rows == [64, 32, 16] and plan.groups == [8, 4, 2]
    if geom == (5, 6):
        assert plan.tile_rows == [36] and plan.groups == [5] and 36 % R.SUM_GROUP == 4
    if geom == (1, 104):
        assert (plan.live_chunks, plan.last_chunk_lanes, plan.tail) == (2, 40, 41)
    if geom == (1, 136):
        assert (plan.chunks, plan.live_chunks, plan.last_chunk_lanes) == (4, 3, 8)
    if geom == (1, 264):
        assert (plan.chunks, plan.live_chunks, plan.last_chunk_lanes) == (8, 5, 8)
    if geom == (1, 512):
        assert plan.lds_bytes == 64 * 1024 and plan.live_chunks == plan.chunks == R.SUM_MAX_CHUNKS and plan.last_chunk_lanes == 64
    if geom == (1, 520):
        assert geom[1] > 64 * R.SUM_MAX_CHUNKS
    return plan


@pytest.mark.parametrize("geom", SUM_GEOMS, ids=_id)
def test_dot_and_mean_in_the_order_of_the_tiles(hip, oracle, geom):
    """dot(a, b), dot(a, a) and mean(a) of random data, whose bits show the order of the additions: HIP == oracle, and up to side 136 == the tile
    chains of reduction_lib (above that the oracle alone is the reference)."""
    sum_plan_checked(geom)
    P = Pair(hip, oracle, geom, 2)
    try:
        a, b = R.random_field(P.lh, 500 + geom[1]), R.random_field(P.lh, 501 + geom[1])
        P.fill(0, a); P.fill(1, b)
        ab, aa, m = P.both("dot", 0, 1), P.both("dot", 0, 0), P.both("mean", 0)
        assert ab[0] == ab[1] and aa[0] == aa[1] and m[0] == m[1], (ab, aa, m)
        assert ab[0] != 0.0 and aa[0] > 0.0 and m[0] != 0.0
        if geom[1] <= 136:
            assert ab[1] == R.tile_sum(P.lh, a, b) and aa[1] == R.tile_sum(P.lh, a, a) and m[1] == R.mean_of(P.lh, R.tile_sum(P.lh, a))
    finally:
        P.destroy()


@pytest.mark.parametrize("geom", [(1, 512), (1, 520)], ids=_id)
def test_mean_of_the_widest_boxes(hip, oracle, geom):
    """The smallest sides that enter their branch: 512 is tile_sum_wave_kernel<8> at exactly 64 KiB of dynamic LDS (the side Solver(box_dim=512)
    allows), 520 tile_sum_kernel<false> + ordered_sum_kernel.  One vector of 1.1 GB, mean only."""
    sum_plan_checked(geom)
    P = Pair(hip, oracle, geom, 1)
    try:
        a = R.random_field(P.lh, 600 + geom[1])
        for lv in (P.lh, P.lo):
            lv.write_raw(0, 0, a[0])
        del a
        m = P.both("mean", 0)
        assert m[0] == m[1] and m[0] != 0.0, m
    finally:
        P.destroy()


# ---------------------------------------------------------------------------------------------------------------- 5. the other maxima
class OperatorPair:
    """A fine level of the reserved vectors on both backends, filled as test_gpu_operators.test_fused_residual_forms fills it, under an MG hierarchy."""

    def __init__(self, hip, oracle, variant, geom):
        self.variant, self.geom, self.hip, self.oracle = variant, geom, hip, oracle
        self.ab = (1.0, 1.0) if "helm" in variant else (0.0, 1.0)
        self.fine, self.mg, self.base = [], [], {}
        for be in (hip, oracle):
            be.configure(**VARIANTS[variant])
            fine = be.level(*geom)
            for vid in range(fine.num_vectors):
                d = R.random_field(fine, 900 + vid)
                if vid >= H.VECTOR_DINV:
                    d = np.abs(d) + 0.5
                if vid in (H.VECTOR_U, H.VECTOR_F):
                    self.base[vid] = d
                fine.write_all(vid, d)
            for vid in range(H.VECTOR_DINV, fine.num_vectors):
                be.lib.exchange_boundary(fine.ptr, vid, H.STENCIL_SHAPE_BOX)
            self.fine.append(fine)
            self.mg.append(be.lib.hpgmg_mg_create(fine.ptr, self.ab[0], self.ab[1], 1))
        self.lh, self.lo = self.fine
        self.ch, self.co = (Level(be, be.lib.hpgmg_mg_level(m, 1)) for be, m in zip((hip, oracle), self.mg))
        self.cells = R.cell_offsets(self.lh)
        L = hip.lib
        c_int, c_dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
        L.hpgmg_residual_norm_fused.restype = c_int
        L.hpgmg_residual_norm_fused.argtypes = [vp, c_int, c_int, c_int, c_dbl, c_dbl, ctypes.POINTER(c_dbl)]
        L.hpgmg_norm_scale_restrict_fused.restype = c_int
        L.hpgmg_norm_scale_restrict_fused.argtypes = [vp, c_int, c_int, vp, ctypes.POINTER(c_dbl)]

    def use(self):
        configure(self.hip, self.oracle, self.variant)

    def plant(self, vid, box, offset, value):
        x = self.base[vid][box].copy()
        x[offset] = value
        for lv in (self.lh, self.lo):
            lv.write_raw(box, vid, x)

    def restore(self, vid, box):
        for lv in (self.lh, self.lo):
            lv.write_raw(box, vid, self.base[vid][box])

    def destroy(self):
        for be, f, m in zip((self.hip, self.oracle), self.fine, self.mg):
            be.lib.hpgmg_mg_destroy(m); f.destroy()


@pytest.fixture
def operator_pair(hip, oracle):
    def get(variant, geom):
        k = (variant, geom)
        if k not in _kept:
            _kept[k] = OperatorPair(hip, oracle, variant, geom)
        _kept[k].use()
        return _kept[k]
    return get


def wide_places(geom):
    """{name: (box, k, j, i)} around every region edge of stencil7_wide_kernel's workgroups: 128 (i) x 16 (j) x 16 planes."""
    d, last = geom[1], geom[0] ** 3 - 1
    out = {"first-box-first": (0, 0, 0, 0), "first-box-last": (0, d - 1, d - 1, d - 1), "last-box-first": (last, 0, 0, 0), "last-box-last": (last, d - 1, d - 1, d - 1),
           "j-15": (last // 2, 40, 15, 9), "j-16": (last // 2, 40, 16, 9), "k-15": (last // 2, 15, 50, 70), "k-16": (last // 2, 16, 50, 70),
           "last-slab": (0, 37, d - 16, 100), "last-plane-chunk": (last, d - 16, 37, 5)}
    if d > 128:
        out.update({"i-127": (0, 100, 100, 127), "i-128": (0, 100, 100, 128)})
    return out


WIDE = [("7pt-cheby-helm", (2, 128)), ("7ptcc-cheby", (1, 256))]
WIDE_CASES = [(v, g, name, stored) for v, g in WIDE for name in wide_places(g) for stored in (True, False)]


@pytest.mark.parametrize("variant,geom,where,stored", WIDE_CASES, ids=_id)
def test_fused_residual_norm_wide_kernel_wherever_the_maximum_sits(operator_pair, variant, geom, where, stored):
    """hpgmg_residual_norm_fused in its stored form (the residual in VECTOR_TEMP) and with res_id = -1 (VECTOR_TEMP untouched): the largest residual
    planted through F on either side of every edge between two workgroups' regions."""
    d, boxes = geom[1], geom[0] ** 3
    assert d % 128 == 0 and boxes * R.ceil_div(d, 16) * (d // 16) * (d // 128) == {128: 512, 256: 512}[d]      # the partials of the launch
    P = operator_pair(variant, geom)
    a, b = P.ab
    box, k, j, i = wide_places(geom)[where]
    h2inv = 1.0 / (P.lh.h * P.lh.h)
    umax = np.abs(P.base[H.VECTOR_U]).max()
    bound = b * h2inv * (6 * 1.5) * 2.0 * umax + a * 1.5 * umax          # |A u| <= b h^-2 (sum of six betas <= 1.5) 2 max|u| + a max(alpha) max|u|
    huge = 2.0 ** 44
    assert huge > 1.0e3 * bound > 0.0
    value = huge if (len(where) % 2) else -huge
    junk = None
    if not stored:
        junk = P.lh.read_raw(box, H.VECTOR_TEMP)
    P.plant(H.VECTOR_F, box, P.cells[k, j, i], value)
    try:
        out = ctypes.c_double(-1.0)
        assert P.hip.lib.hpgmg_residual_norm_fused(P.lh.ptr, H.VECTOR_TEMP if stored else -1, H.VECTOR_U, H.VECTOR_F, a, b, ctypes.byref(out)) == 1
        P.oracle.lib.residual(P.lo.ptr, H.VECTOR_TEMP, H.VECTOR_U, H.VECTOR_F, a, b)
        want = P.oracle.lib.norm(P.lo.ptr, H.VECTOR_TEMP)
        res = P.lo.read_all(H.VECTOR_TEMP)[:, P.cells]
        assert np.unravel_index(np.abs(res).argmax(), res.shape) == (box, k, j, i) and want == np.abs(res).max() > 0.5 * huge
        assert out.value == want, (out.value, want, where)
        got = P.lh.read_raw(box, H.VECTOR_TEMP)
        if stored:
            assert np.array_equal(bits(got[P.cells]), bits(res[box])), "the stored residual of the planted box"
        else:
            assert np.array_equal(bits(got), bits(junk)), "res_id = -1 wrote VECTOR_TEMP"
    finally:
        P.restore(H.VECTOR_F, box)


def tile_places(variant):
    """{name: (box, k, j, i)} at (2, 64): the corners of a box, the first and the last box, either side of a tile edge in i (the box face: a tile
    is as long as the box), j (tiles of 8 rows) and k (chunks of 32 planes, 27-point; of 8 planes, 4th order)."""
    kc = 32 if variant.startswith("27pt") else 8
    out = {f"corner-{c}": (3, 63 * (c >> 2), 63 * ((c >> 1) & 1), 63 * (c & 1)) for c in range(8)}
    out.update({"first-box-first": (0, 0, 0, 0), "last-box-last": (7, 63, 63, 63), "last-box-first": (7, 0, 0, 0),
                "i-hi-of-box-0": (0, 20, 21, 63), "i-lo-of-box-1": (1, 20, 21, 0), "j-7": (5, 30, 7, 11), "j-8": (5, 30, 8, 11),
                "k-below-chunk-edge": (2, kc - 1, 50, 33), "k-above-chunk-edge": (2, kc, 50, 33), "last-chunk": (6, 64 - kc, 62, 62)})
    return out


TILE_CASES = [(v, name) for v in ("27pt-gsrb", "fv4-gsrb") for name in tile_places(v)]


@pytest.mark.parametrize("variant,where", TILE_CASES, ids=_id)
def test_fused_residual_norm_tile_form_wherever_the_maximum_sits(operator_pair, variant, where):
    """The norm-only form of the LDS-tiled 27-point and 4th-order kernels at (2, 64): 64 x 8 tiles over chunks of 32 / 8 planes."""
    geom = (2, 64)
    P = operator_pair(variant, geom)
    a, b = P.ab
    box, k, j, i = tile_places(variant)[where]
    if not hasattr(P, "seeded_norm"):                  # max|F - A u| of the seeded data, from the oracle: what the planted residual must dwarf
        P.oracle.lib.residual(P.lo.ptr, H.VECTOR_TEMP, H.VECTOR_U, H.VECTOR_F, a, b)
        P.seeded_norm = P.oracle.lib.norm(P.lo.ptr, H.VECTOR_TEMP)
    huge = 2.0 ** 44
    assert huge > 1.0e3 * (P.seeded_norm + 1.0) > 1.0e3          # (|A u| <= max|F - A u| + max|F|, and |F| <= 1)
    value = -huge if (len(where) % 2) else huge
    junk = P.lh.read_raw(box, H.VECTOR_TEMP)
    P.plant(H.VECTOR_F, box, P.cells[k, j, i], value)
    try:
        out = ctypes.c_double(-1.0)
        assert P.hip.lib.hpgmg_residual_norm_fused(P.lh.ptr, -1, H.VECTOR_U, H.VECTOR_F, a, b, ctypes.byref(out)) == 1
        P.oracle.lib.residual(P.lo.ptr, H.VECTOR_TEMP, H.VECTOR_U, H.VECTOR_F, a, b)
        want = P.oracle.lib.norm(P.lo.ptr, H.VECTOR_TEMP)
        res = P.lo.read_all(H.VECTOR_TEMP)[:, P.cells]
        assert np.unravel_index(np.abs(res).argmax(), res.shape) == (box, k, j, i) and want == np.abs(res).max() > 0.5 * huge
        assert out.value == want, (out.value, want, where)
        assert np.array_equal(bits(P.lh.read_raw(box, H.VECTOR_TEMP)), bits(junk)), "res_id = -1 wrote VECTOR_TEMP"
    finally:
        P.restore(H.VECTOR_F, box)


def restrict_places(geom):
    """{name: (box, k, j, i)}: each of the eight children of one coarse cell, the first and the last cell, a coarse cell with ci >= 64."""
    d, last = geom[1], geom[0] ** 3 - 1
    ck, cj, ci = 21, 9, 30
    out = {f"child-{c}": (last // 2, 2 * ck + (c >> 2), 2 * cj + ((c >> 1) & 1), 2 * ci + (c & 1)) for c in range(8)}
    out.update({"first": (0, 0, 0, 0), "last": (last, d - 1, d - 1, d - 1)})
    if d // 2 > 64:
        out["ci-100"] = (0, 77, 33, 201)
    return out


RESTRICT_CASES = [(v, g, name) for v, g in WIDE for name in restrict_places(g)]


@pytest.mark.parametrize("variant,geom,where", RESTRICT_CASES, ids=_id)
def test_norm_scale_restrict_wherever_the_maximum_sits(operator_pair, variant, geom, where):
    """hpgmg_norm_scale_restrict_fused (norm_copy_restrict_kernel): a lane takes eight separate maxima, one per child of its coarse cell.  The norm
    is HUGE wherever it sits; R of the planted box and the whole coarse R are the oracle's scale_vector + restriction (the whole fine R once)."""
    P = operator_pair(variant, geom)
    d = geom[1]
    assert R.ceil_div(d // 2, 64) == (2 if d == 256 else 1)
    box, k, j, i = restrict_places(geom)[where]
    if where == "ci-100":
        assert i // 2 >= 64
    value = HUGE if (len(where) + k + j + i) % 2 else -HUGE
    P.plant(H.VECTOR_F, box, P.cells[k, j, i], value)
    try:
        out = ctypes.c_double(-1.0)
        assert P.hip.lib.hpgmg_norm_scale_restrict_fused(P.lh.ptr, H.VECTOR_F, H.VECTOR_R, P.ch.ptr, ctypes.byref(out)) == 1
        L = P.oracle.lib
        want = L.norm(P.lo.ptr, H.VECTOR_F)
        L.scale_vector(P.lo.ptr, H.VECTOR_R, 1.0, H.VECTOR_F)
        L.restriction(P.co.ptr, H.VECTOR_R, P.lo.ptr, H.VECTOR_R, H.RESTRICT_CELL)
        assert out.value == want == HUGE, (out.value, want, where)
        same_bits(P.ch, P.co, H.VECTOR_R)
        boxes = range(P.lh.num_boxes) if where == "first" else [box]
        for q in boxes:
            rh, ro = P.lh.read_raw(q, H.VECTOR_R)[P.cells], P.lo.read_raw(q, H.VECTOR_R)[P.cells]
            assert np.array_equal(bits(rh), bits(ro)), f"R of box {q}"
            if q == box:
                assert rh[k, j, i] == value
    finally:
        P.restore(H.VECTOR_F, box)


@pytest.mark.parametrize("where", ["first", "last"])
def test_deferred_norm_collected_after_other_scalars(operator_pair, where):
    """The deferred record of the result slot (kernels/reduce.hpp): hpgmg_norm_scale_restrict_fused_deferred is issued, then three launches take
    immediate scalars -- a norm with another planted maximum, an ordered sum, and hpgmg_pcg_dot2's two values from one launch -- and only then
    hpgmg_norm_deferred_fetch collects the first.  Every value is the oracle's (whose deferred form answers 0: its value is norm(F)), and the five
    differ pairwise, so a crossed record, ticket or second value cannot pass."""
    variant, geom = WIDE[0]
    assert (variant, geom) == ("7pt-cheby-helm", (2, 128))
    P = operator_pair(variant, geom)
    Lh, Lo = P.hip.lib, P.oracle.lib
    c_int, c_dbl, vp = ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    for L in (Lh, Lo):
        L.hpgmg_norm_scale_restrict_fused_deferred.restype = c_int
        L.hpgmg_norm_scale_restrict_fused_deferred.argtypes = [vp, c_int, c_int, vp]
        L.hpgmg_norm_deferred_fetch.restype = c_dbl
        L.hpgmg_norm_deferred_fetch.argtypes = [vp]
    box, k, j, i = restrict_places(geom)[where]
    other = 0.25 * HUGE                                    # the maximum of U: another value, in another cell of another box
    ubox, uk, uj, ui = (box + 3) % P.lh.num_boxes, 5, 77, 100
    P.plant(H.VECTOR_F, box, P.cells[k, j, i], HUGE if where == "first" else -HUGE)
    P.plant(H.VECTOR_U, ubox, P.cells[uk, uj, ui], -other)
    try:
        assert Lh.hpgmg_norm_scale_restrict_fused_deferred(P.lh.ptr, H.VECTOR_F, H.VECTOR_R, P.ch.ptr) == 1
        ab, cb = c_dbl(-1.0), c_dbl(-1.0)
        got_u = Lh.norm(P.lh.ptr, H.VECTOR_U)
        got_dot = Lh.dot(P.lh.ptr, H.VECTOR_U, H.VECTOR_F)
        assert Lh.hpgmg_pcg_dot2(P.lh.ptr, H.VECTOR_U, H.VECTOR_F, H.VECTOR_DINV, ctypes.byref(ab), ctypes.byref(cb)) == 1      # the kernel took it
        got_f = Lh.hpgmg_norm_deferred_fetch(P.lh.ptr)

        want_f = Lo.norm(P.lo.ptr, H.VECTOR_F)
        if Lo.hpgmg_norm_scale_restrict_fused_deferred(P.lo.ptr, H.VECTOR_F, H.VECTOR_R, P.co.ptr):
            assert Lo.hpgmg_norm_deferred_fetch(P.lo.ptr) == want_f
        else:
            Lo.scale_vector(P.lo.ptr, H.VECTOR_R, 1.0, H.VECTOR_F)
            Lo.restriction(P.co.ptr, H.VECTOR_R, P.lo.ptr, H.VECTOR_R, H.RESTRICT_CELL)
        want_u = Lo.norm(P.lo.ptr, H.VECTOR_U)
        want_dot = Lo.dot(P.lo.ptr, H.VECTOR_U, H.VECTOR_F)
        wab, wcb = c_dbl(-2.0), c_dbl(-2.0)
        assert Lo.hpgmg_pcg_dot2(P.lo.ptr, H.VECTOR_U, H.VECTOR_F, H.VECTOR_DINV, ctypes.byref(wab), ctypes.byref(wcb)) == 0     # the portable form
        got, want = [got_f, got_u, got_dot, ab.value, cb.value], [want_f, want_u, want_dot, wab.value, wcb.value]
        assert want_f == HUGE and want_u == other
        assert len(set(bits(np.array(want)).tolist())) == 5, want
        assert bits(np.array(got)).tolist() == bits(np.array(want)).tolist(), (got, want, where)
        same_bits(P.ch, P.co, H.VECTOR_R)
        for q in (range(P.lh.num_boxes) if where == "first" else [box]):
            rh, ro = P.lh.read_raw(q, H.VECTOR_R)[P.cells], P.lo.read_raw(q, H.VECTOR_R)[P.cells]
            assert np.array_equal(bits(rh), bits(ro)), f"R of box {q}"
    finally:
        P.restore(H.VECTOR_F, box)
        P.restore(H.VECTOR_U, ubox)


def rebuild_restated(lv, a, b):
    """rebuild7_kernel (operators.7pt.c:158-227, variable coefficients with alpha) line by line on what the level holds after the call: one
    operation per statement, the same order, the wall flags from the global index.  Returns (Dinv, Di) on the interiors, (boxes, k, j, i)."""
    d, n, jS, kS = lv.box_dim, lv.dim, lv.jStride, lv.kStride
    q = R.cell_offsets(lv)
    bi, bj, bk, al = (lv.read_all(v) for v in (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K, H.VECTOR_ALPHA))
    h2inv = 1.0 / (lv.h * lv.h)
    k, j, i = np.meshgrid(np.arange(d), np.arange(d), np.arange(d), indexing="ij")
    shape = (lv.num_boxes, d, d, d)
    ilo, ihi, jlo, jhi, klo, khi = (np.ones(shape) for _ in range(6))
    for box in range(lv.num_boxes):
        li, lj, lk = lv.box_low(box)
        ilo[box][li + i - 1 < 0] = 0.0; ihi[box][li + i + 1 >= n] = 0.0
        jlo[box][lj + j - 1 < 0] = 0.0; jhi[box][lj + j + 1 >= n] = 0.0
        klo[box][lk + k - 1 < 0] = 0.0; khi[box][lk + k + 1 >= n] = 0.0
    s = np.abs(bi[:, q] * ilo)
    s = s + np.abs(bj[:, q] * jlo)
    s = s + np.abs(bk[:, q] * klo)
    s = s + np.abs(bi[:, q + 1] * ihi)
    s = s + np.abs(bj[:, q + jS] * jhi)
    s = s + np.abs(bk[:, q + kS] * khi)
    sum_abs = abs(b * h2inv) * s
    t = bi[:, q] * (ilo - 2.0)
    t = t + bj[:, q] * (jlo - 2.0)
    t = t + bk[:, q] * (klo - 2.0)
    t = t + bi[:, q + 1] * (ihi - 2.0)
    t = t + bj[:, q + jS] * (jhi - 2.0)
    t = t + bk[:, q + kS] * (khi - 2.0)
    aii = ((-b) * h2inv) * t
    aii = aii + a * al[:, q]
    return 1.0 / aii, (aii + sum_abs) / aii


REBUILD_CASES = [((2, 64), "first"), ((2, 64), "last"), ((1, 104), "i-64"), ((1, 3), "last-workgroup"), ((1, 1), "the-cell")]


@pytest.mark.parametrize("geom,where", REBUILD_CASES, ids=_id)
def test_rebuild_operator_eigenvalue_bound_wherever_it_sits(hip, oracle, geom, where):
    """rebuild_operator of the 7-point Helmholtz operator (a = b = 1): alpha = 1e3 h^-2 everywhere (Di <= 1 + 9 / 1e3) but 0.0 in one cell, whose
    Di = 1 + sum|Aij| / Aii is then the largest by far -- unless every face of the cell is a wall, (1, 1), where Di = 1 exactly and alone.
    (2, 64) leaves 8192 partials: final_max_kernel's 4-way loop, eight trips and no tail."""
    d, boxes = geom[1], geom[0] ** 3
    nblk = R.ceil_div(boxes * d * d, R.ROWS_PER_BLOCK)
    assert nblk == {(2, 64): 8192, (1, 104): 2704, (1, 3): 3, (1, 1): 1}[geom]
    if geom == (2, 64):
        assert R.final_max_plan(nblk) == (256, 8, 0)
    box, k, j, i = {"first": (0, 0, 0, 0), "last": (boxes - 1, d - 1, d - 1, d - 1), "i-64": (0, 50, 51, 64 + 13), "last-workgroup": (0, 2, 2, 1), "the-cell": (0, 0, 0, 0)}[where]
    if where == "last-workgroup":
        assert (k * d + j) // R.ROWS_PER_BLOCK == nblk - 1 and (boxes * d * d) % R.ROWS_PER_BLOCK == 1
    configure(hip, oracle, "7pt-cheby-helm")
    levels = [be.level(*geom) for be in (hip, oracle)]
    lh, lo = levels
    try:
        q = R.cell_offsets(lh)
        h2inv = 1.0 / (lh.h * lh.h)
        alpha = np.full((boxes, lh.volume), 1.0e3 * h2inv)
        alpha[box, q[k, j, i]] = 0.0
        for lv in levels:
            for n, vid in enumerate((H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)):
                lv.write_all(vid, R.random_field(lv, 700 + n + d) * 0.5 + 1.0)          # in [0.5, 1.5)
            lv.write_all(H.VECTOR_ALPHA, alpha)
            lv.write_all(H.VECTOR_DINV, R.random_field(lv, 710 + d))
            lv.b.lib.rebuild_operator(lv.ptr, None, 1.0, 1.0)
            lv.b.lib.hpgmg_operators_flush()
        dinv, Di = rebuild_restated(lo, 1.0, 1.0)
        assert np.unravel_index(Di.argmax(), Di.shape) == (box, k, j, i)
        if geom != (1, 1):
            assert Di.max() > 1.1 and np.sort(Di.ravel())[-2] < 1.01
        assert lh.eigenvalue == lo.eigenvalue == Di.max(), (lh.eigenvalue, lo.eigenvalue, Di.max())
        same_bits(lh, lo, H.VECTOR_DINV)
        same_bits(lh, lo, H.VECTOR_L1INV)
        assert np.array_equal(bits(lo.read_all(H.VECTOR_DINV)[:, q]), bits(dinv))
    finally:
        lh.destroy(); lo.destroy()


class PcgPair:
    """The finest levels of a HIP and an oracle Solver that method="pcg" has grown by its three vectors (as tests/test_gpu_user_pcg.py _hooks)."""

    def __init__(self, hip, oracle, n, box_dim):
        self.n, self.stack, self.levels, self.libs = n, contextlib.ExitStack(), [], (hip.lib, oracle.lib)
        coef = random_coefficients(n, "dirichlet", False, seed=900 + n)
        for lib in self.libs:
            s = self.stack.enter_context(Solver(n, box_dim=box_dim, bc="dirichlet", a=0.0, b=0.9, lib=lib))
            s.set_coefficients(*coef)
            s.solve(np.ones((n, n, n)), method="pcg", max_iter=1)
            self.levels.append(lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(s._ptr), 0))
        self.p_id = hip.lib.hpgmg_vectors_reserved()
        rng = np.random.default_rng(n)
        self.vectors = {name: rng.random((n, n, n)) * 2.0 - 1.0 for name in ("x", "r", "p", "Ap")}
        self.ids = {"x": H.VECTOR_U, "r": H.VECTOR_R, "p": self.p_id, "Ap": self.p_id + 1}
        for name in ("p", "Ap"):
            self.put(name, self.vectors[name])

    def put(self, name, array):
        for lib, L in zip(self.libs, self.levels):
            assert lib.hpgmg_dense_pack(L, self.ids[name], array.ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0

    def get(self, lib, L, name):
        v = np.empty((self.n,) * 3)
        assert lib.hpgmg_dense_unpack(L, self.ids[name], v.ctypes.data, H.WHERE_HOST) == 0
        return v

    def destroy(self):
        self.stack.close()


PCG_PLACES = {(128, 128): {"first": (0, 0, 0), "last": (127, 127, 127), "last-column-block": (5, 126, 3), "last-segment": (113, 40, 77)},
              (88, 8): {"first": (0, 0, 0), "last": (87, 87, 87), "last-box": (81, 82, 83), "middle-box": (41, 44, 47)}}
PCG_CASES = [(g, name) for g in PCG_PLACES for name in PCG_PLACES[g]]


@pytest.mark.parametrize("size,where", PCG_CASES, ids=_id)
def test_pcg_update_rmax_wherever_it_sits(hip, oracle, size, where):
    """hpgmg_pcg_update: x = x + alpha p, r = r - alpha Ap and max|r|.  (128, 128) leaves 512 workgroup values (64 column blocks x 8 segments:
    final_max_kernel's tail loop alone), (88, 8) 1331 (one per box: its 4-way loop and a tail of 307)."""
    n, box_dim = size
    boxes, ncb, nseg = (n // box_dim) ** 3, R.ceil_div(box_dim ** 2, 256), R.ceil_div(box_dim, 16)
    items = boxes * ncb * nseg
    assert items == {(128, 128): 512, (88, 8): 1331}[size] and R.final_max_plan(items) == {512: (0, 0, 512), 1331: (256, 1, 307)}[items]
    k, j, i = PCG_PLACES[size][where]
    if where == "last-column-block":
        assert (i + box_dim * j) // 256 == ncb - 1 > 0
    if where == "last-segment":
        assert k // 16 == nseg - 1 > 0
    if ("pcg", size) not in _kept:
        _kept["pcg", size] = PcgPair(hip, oracle, n, box_dim)
    P = _kept["pcg", size]
    configure(hip, oracle, "7pt-cheby")                # a = 0: the variant the two solvers were made with
    r = P.vectors["r"].copy()
    r[k, j, i] = HUGE if (k + len(where)) % 2 else -HUGE
    P.put("x", P.vectors["x"]); P.put("r", r)
    alpha_cg, out = 1.0e-3, []
    for lib, L in zip(P.libs, P.levels):
        value = ctypes.c_double(-1.0)
        took = lib.hpgmg_pcg_update(L, H.VECTOR_U, H.VECTOR_R, P.ids["p"], P.ids["Ap"], alpha_cg, ctypes.byref(value))
        out.append((took, value.value, P.get(lib, L, "x"), P.get(lib, L, "r")))
    (took_h, rmax_h, x_h, r_h), (took_o, rmax_o, x_o, r_o) = out
    assert (took_h, took_o) == (1, 0)
    assert np.unravel_index(np.abs(r_o).argmax(), r_o.shape) == (k, j, i) and np.abs(r_o).max() > 0.9 * HUGE
    assert rmax_h == rmax_o == np.abs(r_o).max(), (rmax_h, rmax_o, np.abs(r_o).max())
    assert np.array_equal(bits(r_h), bits(r_o)) and np.array_equal(bits(x_h), bits(x_o))
    assert np.array_equal(bits(r_o), bits(r - alpha_cg * P.vectors["Ap"])) and np.array_equal(bits(x_o), bits(P.vectors["x"] + alpha_cg * P.vectors["p"]))
