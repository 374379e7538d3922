"""The single-level dense-array and boundary hooks on the MI355X, each alone, at the edges of their launch shape (kernels/dense_io.hip: pack,
pack_walls, unpack; kernels/dense_boundary.hip: the lifted packs, boundary_flux and its _faces / _robin forms, store_walls, check_kappa, restrict;
kernels/dense_flux.hip: unpack_flux).  Every output is pre-filled with NaN (the wall array: a sentinel), then

    HIP from host arrays  ==  HIP from device arrays (where the hook has a `where`)  ==  the CPU oracle  ==  the NumPy restatement

as 64-bit patterns over whole padded boxes and whole arrays, so the sign of a zero and one cell too many both count.  The restatements
(tests/dense_hooks_lib.py) are pinned on the oracle by tests/test_oracle_dense_hooks.py; the hooks that do arithmetic (lifted pack, boundary_flux,
unpack_flux) share it with the oracle through include/hpgmg_boundary_math.h, so for them HIP == oracle checks what each side keeps of its own --
indexing, ownership of a cell by one lane, the launch mapping, staging from host arrays, the status word -- and unpack_flux is also held to
user_flux_lib.reference within the bound tests/test_oracle_user_flux.py holds the oracle to.

The launch shapes (256 lanes per workgroup; x capped at 16384 workgroups = 4,194,304 lanes, the rest by grid stride; grid row y = box):

    (boxes per side, side)  padded volume  cells      6 side^2  what it reaches
    (1, 162)                4,410,944      4,251,528   157,464  a second, short trip of the x stride in pack, pack_walls, pack_lifted (over the
                                                                padded volume), unpack and unpack_flux (over the cells); 161^3 is below one trip
    (3, 12)                     3,136          1,728       864  27 boxes on zero (the middle one) to three walls; the last of 4 face workgroups partly live
    (17, 2)                        64              8        24  4913 boxes, most on no wall
    (1, 6)                        512            216       216  one partly live workgroup, a side that is no power of two
    (1, 1)                         36              1         6  one cell on all six walls
and a periodic (3, 12) for pack, unpack and unpack_flux.  The status word is probed with one bad value at each position only one lane or one trip
reaches.  Not reached by any test: the grid-row stride (more than 65535 boxes) and the x cap of the face kernels (a side above 836); DESIGN.md §11.
"""
import ctypes

import numpy as np
import pytest

import dense_hooks_lib as DH
import hpgmg_amd as H
from hpgmg_testlib import VARIANTS, Backend
from test_gpu_boundary_hooks import HostArrays
from test_gpu_operators import make_pair
from test_gpu_user_problem import DeviceArrays
from test_gpu_user_sensitivity import _Plugin
from user_flux_lib import reference
from user_robin_lib import D, N, R

pytestmark = pytest.mark.gpu

VARIANT = "7pt-cheby-helm"
B_COEF = 1.5
OUT, U_ID = H.VECTOR_TEMP, H.VECTOR_U                 # the vector the packs write; the seeded vector unpack and unpack_flux read
BETAS = (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
SENTINEL = -7.0
PERIODIC = (3, 12, "periodic")
NOT_FINITE, OUT_OF_RANGE = H.DENSE_NOT_FINITE, H.DENSE_OUT_OF_RANGE


def _id(g):
    return DH.geom_id(g[:2]) + ("-periodic" if len(g) > 2 else "") if isinstance(g[0], int) else g[0]


@pytest.fixture(scope="module")
def libs():
    hip = Backend.hip().lib
    K = H.load_kernels()
    assert K.hpgmg_hip_set_device(0) == 0
    for lib in (hip, Backend.oracle().lib):
        lib.hpgmg_set_verbose(0)
    return hip, Backend.oracle().lib, K


class _Mem(_Plugin):
    """_Plugin that also reads an array back."""

    def get(self, p, shape):
        out = np.empty(shape)
        self.lib.hpgmg_vector_download(out.ctypes.data, p, out.size)
        return out


class Pair:
    """The two levels of one geometry with the same seeded content, u's box-to-box ghost zones filled (unpack_flux's contract), and what the oracle's
    level holds of the vectors the tests read."""

    def __init__(self, hip, oracle, geom):
        periodic = len(geom) > 2
        self.lh, self.lo = make_pair(hip, oracle, VARIANT, *geom[:2], seed=53 + geom[1], vectors=DH.VECTORS,
                                     bc=H.BC_PERIODIC if periodic else H.BC_DIRICHLET)
        for lv in (self.lh, self.lo):
            lv.b.lib.exchange_boundary(lv.ptr, U_ID, lv.b.lib.stencil_get_shape())
        lv = self.lo
        assert lv.num_vectors == DH.VECTORS and lv.num_boxes == geom[0] ** 3 and lv.box_dim == geom[1] and lv.ghosts == 1
        self.geo = DH.Geo(lv, periodic)
        self.n, self.h, self.periodic = lv.dim, lv.h, periodic
        self.u_boxes, self.betas = lv.read_all(U_ID), [lv.read_all(v) for v in BETAS]
        assert DH.same_bits(self.lh.read_all(U_ID), self.u_boxes)
        self.u = DH.unpack(self.geo, self.u_boxes)
        self.nan = np.full((lv.num_boxes, lv.volume), np.nan)

    def sides(self, K):
        """(name, level, where, holder of dense arrays) of the three ways a hook with a `where` runs."""
        return [("hip-host", self.lh, H.WHERE_HOST, HostArrays()), ("hip-device", self.lh, H.WHERE_PLUGIN, DeviceArrays(K)),
                ("oracle", self.lo, H.WHERE_HOST, HostArrays())]

    def destroy(self):
        self.lh.destroy(); self.lo.destroy()


_pairs = {}


@pytest.fixture
def pair_of(hip, oracle):
    """pair_of(geom): made once and kept for the module (4913 boxes take seconds to fill box by box)."""
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


def _agree(seen, want=None, computed_nan=False):
    """Every side's arrays have the oracle's bits, and those the restatement's.  computed_nan: the run planted a value that is not finite in the
    input of a hook that does arithmetic; where that leaves a NaN, any NaN agrees (dense_hooks_lib.same_bits), every other entry still bit for bit."""
    ref = seen["oracle"]
    for key, arrays in seen.items():
        assert len(arrays) == len(ref)
        for slot, (a, b) in enumerate(zip(arrays, ref)):
            assert DH.same_bits(a, b, computed_nan), f"{key} array {slot} against the oracle: {DH.first_differences(a, b, computed_nan=computed_nan)}"
    for slot, b in enumerate(want or []):
        assert DH.same_bits(ref[slot], b), f"the oracle's array {slot} against the restatement: {DH.first_differences(ref[slot], b)}"


def _source(shape, seed, check=H.DENSE_CHECK_FINITE):
    """Random values that pass `check`; FINITE: both signs with some 0.0 and -0.0, NONNEGATIVE: with some 0.0 and -0.0 (-0.0 >= 0.0 holds)."""
    rng = np.random.default_rng(seed)
    src = rng.random(shape)
    if check == H.DENSE_CHECK_POSITIVE:
        return src + 0.5
    if check == H.DENSE_CHECK_FINITE:
        src = src * 2.0 - 1.0
    flat = src.reshape(-1)
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 50))] = -0.0
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 50))] = 0.0
    return src


def _boundary(n, mask, with_kappa, seed):
    """g, wall, kappa (None without) and the wall kinds per face."""
    rng = np.random.default_rng(seed)
    g = rng.random((6, n, n)) * 4.0 - 2.0
    wall = rng.random((6, n, n)) + 0.5 if mask else None
    kappa = rng.random((6, n, n)) * 3.0 if with_kappa else None
    if kappa is not None:
        kappa.reshape(-1)[::3] = 0.0
    faces = tuple((R if with_kappa else N) if (mask >> f) & 1 else D for f in range(6))
    return g, wall, kappa, faces


def _cells(geom, n):
    """(name, (k, j, i)) of the cells a status probe plants a bad value in."""
    out = [("first", (0, 0, 0)), ("last", (n - 1, n - 1, n - 1))]
    if geom[:2] == (1, 162):
        out.append(("second-trip", (157, 3, 5)))          # padded offset >= 4,194,304 (interior k >= 156); cell index 157 * 162^2 >= 4,194,304 too
    if geom[:2] == (3, 12):
        out.append(("middle-box", (17, 12, 23)))
    return out


def _face_entries(n):
    """One entry on each of the six faces in turn: a corner, the last entry, and one off the corners where the face has one."""
    spots = [(0, 0), (n - 1, n - 1), (n // 2, 0), (0, n - 1), (n - 1, n // 3), (n // 2, n // 2)]
    return [(face,) + spots[face] for face in range(6)]


# ---------------------------------------------------------------- pack
@pytest.mark.parametrize("layout", DH.LAYOUTS)
@pytest.mark.parametrize("geom", DH.GEOMS + [PERIODIC], ids=_id)
def test_pack(libs, pair_of, geom, layout):
    _, _, K = libs
    P = pair_of(geom)
    shape = DH.dense_shape(P.geo, layout)
    assert shape == tuple(P.n + (not P.periodic and layout == H.DENSE_FACE_I + a) for a in (2, 1, 0))
    for check in (H.DENSE_CHECK_FINITE, H.DENSE_CHECK_POSITIVE, H.DENSE_CHECK_NONNEGATIVE):
        src = _source(shape, 1000 + geom[1] + 10 * layout + check, check)
        seen = {}
        for key, lv, where, mem in P.sides(K):
            try:
                lv.write_all(OUT, P.nan)
                assert lv.b.lib.hpgmg_dense_pack(lv.ptr, OUT, mem.put(src), where, layout, check) == 0, (key, check)
                seen[key] = [lv.read_all(OUT)]
            finally:
                mem.free()
        _agree(seen, [DH.pack(P.geo, src, layout)])


def _pack_status(P, K, layout, check, plants, expect, compare_vector=False):
    """One pack of an all-ones array with `plants` ([(index, value)]) on the three sides: every status is `expect`."""
    src = np.ones(DH.dense_shape(P.geo, layout))
    for at, value in plants:
        src[at] = value
    assert DH.check_bits(src, check) == expect
    seen = {}
    for key, lv, where, mem in P.sides(K):
        try:
            if compare_vector:
                lv.write_all(OUT, P.nan)
            assert lv.b.lib.hpgmg_dense_pack(lv.ptr, OUT, mem.put(src), where, layout, check) == expect, (key, layout, check, plants)
            if compare_vector:
                seen[key] = [lv.read_all(OUT)]
        finally:
            mem.free()
    if compare_vector:
        _agree(seen, [DH.pack(P.geo, src, layout)])         # a bad status still leaves the vector as the oracle leaves it


VALUES = [(np.nan, H.DENSE_CHECK_FINITE, NOT_FINITE), (np.inf, H.DENSE_CHECK_FINITE, NOT_FINITE), (-1.0, H.DENSE_CHECK_POSITIVE, OUT_OF_RANGE),
          (0.0, H.DENSE_CHECK_POSITIVE, OUT_OF_RANGE), (-1.0, H.DENSE_CHECK_NONNEGATIVE, OUT_OF_RANGE), (-0.0, H.DENSE_CHECK_NONNEGATIVE, 0),
          (np.nan, H.DENSE_CHECK_POSITIVE, NOT_FINITE), (-np.inf, H.DENSE_CHECK_NONNEGATIVE, NOT_FINITE)]


@pytest.mark.parametrize("geom", DH.GEOMS + [PERIODIC], ids=_id)
def test_pack_status_word(libs, pair_of, geom):
    """One bad value per call, at each position only one lane or one trip reaches; then NaN in one place and -1.0 in another: both bits."""
    _, _, K = libs
    P = pair_of(geom)
    n = P.n
    cells = _cells(geom, n)
    big = geom[:2] == (1, 162)
    for name, at in cells:
        for value, check, expect in (VALUES[:1] if big and name != "second-trip" else VALUES):
            _pack_status(P, K, H.DENSE_CELL, check, [(at, value)], expect)
    if n > 1:
        _pack_status(P, K, H.DENSE_CELL, H.DENSE_CHECK_POSITIVE, [(cells[0][1], np.nan), (cells[-1][1], -1.0)], NOT_FINITE | OUT_OF_RANGE, compare_vector=True)
    if P.periodic:
        return
    for axis in range(3):                                   # entry N of a face array: the high ghost layer of the boxes on the high face
        layout = H.DENSE_FACE_I + axis
        for q, p in ((n - 1, n - 1), (n // 2, 0))[:1 if big else 2]:
            at = [q, p]
            at.insert(2 - axis, n)
            for value, check, expect in (VALUES[2:3] if big else VALUES):
                _pack_status(P, K, layout, check, [(tuple(at), value)], expect)
        first = (0, 0, 0)
        _pack_status(P, K, layout, H.DENSE_CHECK_NONNEGATIVE, [(first, -1.0), (tuple(at), np.inf)], NOT_FINITE | OUT_OF_RANGE, compare_vector=True)


# ---------------------------------------------------------------- pack_walls
@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("geom", DH.GEOMS, ids=_id)
def test_pack_walls(libs, pair_of, geom, axis):
    _, _, K = libs
    P = pair_of(geom)
    n, layout = P.n, H.DENSE_FACE_I + axis
    src = _source(DH.dense_shape(P.geo, layout), 2000 + geom[1] + axis)
    before = np.full((6, n, n), SENTINEL)

    def run(src, mask, check, expect):
        seen = {}
        for key, lv, where, mem in P.sides(K):
            walls = _Mem(lv.b.lib)
            try:
                lv.write_all(OUT, P.nan)
                pw = walls.put(before)
                assert lv.b.lib.hpgmg_dense_pack_walls(lv.ptr, OUT, mem.put(src), where, layout, check, mask, pw) == expect, (key, mask)
                seen[key] = [lv.read_all(OUT), walls.get(pw, before.shape)]
            finally:
                mem.free(); walls.free()
        _agree(seen, DH.pack_walls(P.geo, src, layout, mask, before))
        owned = [2 * axis + side for side in (0, 1) if (mask >> (2 * axis + side)) & 1]
        assert (np.delete(seen["hip-device"][1], owned, axis=0) == SENTINEL).all()          # what the array does not own keeps its pre-fill

    for mask in DH.wall_masks(axis):
        run(src, mask, H.DENSE_CHECK_FINITE, 0)
    bad = np.ones_like(src)                                 # a value on a masked wall is still checked: the last entry of the high wall, the first of the low
    at = [n - 1, n - 1]
    at.insert(2 - axis, n)
    bad[tuple(at)] = -1.0
    run(bad, 63, H.DENSE_CHECK_POSITIVE, OUT_OF_RANGE)
    bad[0, 0, 0] = np.nan
    run(bad, 63, H.DENSE_CHECK_POSITIVE, NOT_FINITE | OUT_OF_RANGE)


# ---------------------------------------------------------------- unpack
@pytest.mark.parametrize("geom", DH.GEOMS + [PERIODIC], ids=_id)
def test_unpack(libs, pair_of, geom):
    """No round trip: the expected array is the oracle level's interior(); the vector's ghost zones and padding hold other seeded data."""
    _, _, K = libs
    P = pair_of(geom)
    shape = (P.n,) * 3
    seen = {}
    for key, lv, where, mem in P.sides(K):
        try:
            p = mem.put(np.full(shape, np.nan))
            assert lv.b.lib.hpgmg_dense_unpack(lv.ptr, U_ID, p, where) == 0, key
            seen[key] = [mem.get(p, shape)]
        finally:
            mem.free()
    _agree(seen, [DH.unpack(P.geo, P.u_boxes)])
    assert DH.same_bits(seen["hip-host"][0], P.lo.interior(U_ID))


# ---------------------------------------------------------------- the lifted packs
def _lifted(lv, where, pf, mask, with_kappa, pg, pwall, pkappa):
    lib = lv.b.lib
    if with_kappa:
        return lib.hpgmg_dense_pack_lifted_robin(lv.ptr, OUT, pf, where, pg, B_COEF, mask, pwall, pkappa)
    if mask:
        return lib.hpgmg_dense_pack_lifted_faces(lv.ptr, OUT, pf, where, pg, B_COEF, mask, pwall)
    return lib.hpgmg_dense_pack_lifted(lv.ptr, OUT, pf, where, pg, B_COEF)


def _run_lifted(P, K, f, g, wall, kappa, mask, with_kappa, expect):
    seen = {}
    for key, lv, where, mem in P.sides(K):
        bnd = _Mem(lv.b.lib)
        try:
            lv.write_all(OUT, P.nan)
            st = _lifted(lv, where, mem.put(f), mask, with_kappa, bnd.put(g), bnd.put(wall), bnd.put(kappa))
            assert st == expect, (key, st)
            seen[key] = [lv.read_all(OUT)]
        finally:
            mem.free(); bnd.free()
    _agree(seen, computed_nan=expect != 0)
    return seen["oracle"][0]


@pytest.mark.parametrize("walls", DH.WALLS, ids=_id)
@pytest.mark.parametrize("geom", DH.GEOMS, ids=_id)
def test_pack_lifted(libs, pair_of, geom, walls):
    """pack_lifted (mask 0), _faces (six Neumann walls) and _robin (a mixed mask with kappa): whole padded boxes and the status; f and each of the
    six faces of g are probed with one value that is not finite."""
    _, mask, with_kappa = walls
    _, _, K = libs
    P = pair_of(geom)
    n = P.n
    f = _source((n,) * 3, 3000 + n + mask)
    g, wall, kappa, _ = _boundary(n, mask, with_kappa, 3100 + n + mask)
    got = _run_lifted(P, K, f, g, wall, kappa, mask, with_kappa, 0)
    zero = DH.pack(P.geo, f, H.DENSE_CELL)
    assert not np.isnan(got).any()
    inner = np.zeros((n,) * 3, dtype=bool)
    inner[1:-1, 1:-1, 1:-1] = True                          # off the walls the lifted pack is the plain pack, ghosts and padding included
    changed = DH.unpack(P.geo, (got.view(np.uint64) != zero.view(np.uint64)).astype(np.float64)) != 0.0
    assert not (changed & inner).any() and (n < 3 or changed.any())
    outside = got.copy()
    outside[:, P.geo.offsets(P.geo.dim, P.geo.dim, P.geo.dim).ravel()] = 0.0
    assert not outside.view(np.uint64).any()                # ghost zones and padding: +0.0
    big = geom == (1, 162)
    for name, at in _cells(geom, n):
        if big and name == "first":
            continue
        bad = f.copy()
        bad[at] = np.inf if name == "last" else np.nan
        _run_lifted(P, K, bad, g, wall, kappa, mask, with_kappa, NOT_FINITE)
    for face, q, p in _face_entries(n)[::3 if big else 1]:
        bad = g.copy()
        bad[face, q, p] = np.nan if face & 1 else -np.inf
        _run_lifted(P, K, f, bad, wall, kappa, mask, with_kappa, NOT_FINITE)


# ---------------------------------------------------------------- boundary_flux
def _flux(lv, pphi, mask, with_kappa, pg, pwall, pkappa):
    lib = lv.b.lib
    if with_kappa:
        return lib.hpgmg_boundary_flux_robin(lv.ptr, pphi, pg, B_COEF, mask, pwall, pkappa)
    if mask:
        return lib.hpgmg_boundary_flux_faces(lv.ptr, pphi, pg, B_COEF, mask, pwall)
    return lib.hpgmg_boundary_flux(lv.ptr, pphi, pg, B_COEF)


@pytest.mark.parametrize("walls", DH.WALLS, ids=_id)
@pytest.mark.parametrize("geom", DH.GEOMS, ids=_id)
def test_boundary_flux(libs, pair_of, geom, walls):
    """flux, flux_faces, flux_robin: every one of the 6 n^2 entries written, with the oracle's bits; each face of g probed with a bad value."""
    _, mask, with_kappa = walls
    P = pair_of(geom)
    n = P.n
    g, wall, kappa, _ = _boundary(n, mask, with_kappa, 4000 + n + mask)

    def run(g, expect):
        seen = {}
        for key, lv in (("hip", P.lh), ("oracle", P.lo)):
            bnd = _Mem(lv.b.lib)
            try:
                pphi = bnd.put(np.full((6, n, n), np.nan))
                assert _flux(lv, pphi, mask, with_kappa, bnd.put(g), bnd.put(wall), bnd.put(kappa)) == expect, key
                seen[key] = [bnd.get(pphi, (6, n, n))]
            finally:
                bnd.free()
        _agree(seen, computed_nan=expect != 0)
        return seen["hip"][0]

    phi = run(g, 0)
    assert np.isfinite(phi).all()                           # no NaN left: every entry has a box face that owns it
    for face, q, p in _face_entries(n):
        bad = g.copy()
        bad[face, q, p] = np.inf if face & 1 else np.nan
        run(bad, NOT_FINITE)


# ---------------------------------------------------------------- store_walls
@pytest.mark.parametrize("walls", DH.WALLS, ids=_id)
@pytest.mark.parametrize("geom", DH.GEOMS, ids=_id)
def test_store_walls(libs, pair_of, geom, walls):
    """The three beta vectors over whole padded boxes: the entries on a masked wall become wall * (t / (2.0 + t)), every other one is unchanged."""
    _, mask, with_kappa = walls
    P = pair_of(geom)
    n = P.n
    _, wall, kappa, _ = _boundary(n, mask, with_kappa, 5000 + n + mask)
    if wall is None:
        wall = np.ones((6, n, n))                           # mask 0 with a wall array: nothing may change
    seen = {}
    try:
        for key, lv in (("hip", P.lh), ("oracle", P.lo)):
            bnd = _Mem(lv.b.lib)
            try:
                lv.b.lib.hpgmg_boundary_store_walls(lv.ptr, bnd.put(wall), bnd.put(kappa), mask)
                seen[key] = [lv.read_all(v) for v in BETAS]
            finally:
                bnd.free()
    finally:
        for lv in (P.lh, P.lo):
            for v, b in zip(BETAS, P.betas):
                lv.write_all(v, b)
    want = DH.store_walls(P.geo, P.betas, wall, kappa, P.h, mask)
    _agree(seen, want)
    changed = sum(int((a != b).sum()) for a, b in zip(seen["hip"], P.betas))
    assert changed == bin(mask).count("1") * n * n


# ---------------------------------------------------------------- check_kappa
@pytest.mark.parametrize("geom", DH.GEOMS, ids=_id)
def test_check_kappa(libs, pair_of, geom):
    _, _, K = libs
    P = pair_of(geom)
    for name, plants, robin_mask, status, positive in DH.KAPPA_CASES:
        kappa = DH.kappa_case(P.n, plants)
        assert DH.check_kappa(kappa, robin_mask) == (status, positive)
        for key, lv, where, mem in P.sides(K):
            bnd = _Mem(lv.b.lib)
            try:
                any_positive = ctypes.c_int(-1)
                p = bnd.put(kappa) if where == H.WHERE_PLUGIN else mem.put(kappa)
                assert lv.b.lib.hpgmg_boundary_check_kappa(lv.ptr, p, where, robin_mask, ctypes.byref(any_positive)) == status, (key, name)
                assert any_positive.value == positive, (key, name)
            finally:
                mem.free(); bnd.free()


# ---------------------------------------------------------------- restrict
@pytest.mark.parametrize("n_c", [81, 18, 17, 3, 1])
def test_restrict(libs, pair_of, n_c):
    P = pair_of((1, 1))                                     # the hook takes the sizes from the levels: the oracle's from both, the plugin's from the coarse
    g_f = np.random.default_rng(6000 + n_c).random((6, 2 * n_c, 2 * n_c)) * 4.0 - 2.0
    seen = {}
    for key, be in (("hip", P.lh.b), ("oracle", P.lo.b)):
        be.configure(**VARIANTS[VARIANT])
        lf, lc = be.level(1, 2 * n_c, num_vectors=1), be.level(1, n_c, num_vectors=1)
        bnd = _Mem(be.lib)
        try:
            pc = bnd.put(np.full((6, n_c, n_c), np.nan))
            be.lib.hpgmg_boundary_restrict(lc.ptr, pc, lf.ptr, bnd.put(g_f))
            seen[key] = [bnd.get(pc, (6, n_c, n_c))]
        finally:
            bnd.free()
            lf.destroy(); lc.destroy()
    _agree(seen, [DH.restrict(g_f)])


# ---------------------------------------------------------------- unpack_flux
def _run_flux(P, K, g, wall, kappa, mask, expect):
    shapes = [DH.dense_shape(P.geo, H.DENSE_FACE_I + a) for a in range(3)]
    seen = {}
    for key, lv, where, mem in P.sides(K):
        bnd = _Mem(lv.b.lib)
        try:
            ptr = [mem.put(np.full(s, np.nan)) for s in shapes]
            st = lv.b.lib.hpgmg_dense_unpack_flux(lv.ptr, U_ID, bnd.put(g), B_COEF, mask, bnd.put(wall), bnd.put(kappa), *ptr, where)
            assert st == expect, (key, st)
            seen[key] = [mem.get(p, s) for p, s in zip(ptr, shapes)]
        finally:
            mem.free(); bnd.free()
    _agree(seen, computed_nan=expect != 0)
    return seen["hip-device"]


@pytest.mark.parametrize("geom,walls", [(g, w) for g in DH.GEOMS for w in DH.WALLS] + [(PERIODIC, DH.WALLS[0])], ids=_id)
def test_unpack_flux(libs, pair_of, geom, walls):
    """Three ways with the same bits in every entry and none left NaN; and within user_flux_lib.reference's own bound of that NumPy evaluation
    (16 eps of the face's terms: the closeness tests/test_oracle_user_flux.py holds the oracle to).  The reference's betas are the level's, as
    dense_hooks_lib.unpack gathers a face array, with the wall array's values on the masked walls."""
    _, mask, with_kappa = walls
    _, _, K = libs
    P = pair_of(geom)
    n = P.n
    g, wall, kappa, faces = _boundary(n, mask, with_kappa, 7000 + n + mask)
    if P.periodic:
        g = None
    q = _run_flux(P, K, g, wall, kappa, mask, 0)
    assert all(np.isfinite(x).all() for x in q)
    betas = [DH.unpack(P.geo, b, H.DENSE_FACE_I + a) for a, b in enumerate(P.betas)]
    for face in range(6):
        if (mask >> face) & 1:
            np.moveaxis(betas[face >> 1], 2 - (face >> 1), 0)[n if face & 1 else 0] = wall[face]
    ref = reference(n, "periodic" if P.periodic else "dirichlet", None if P.periodic else faces, B_COEF, P.h, betas, P.u, g, kappa)
    for axis, (got, (q_ref, bound)) in enumerate(zip(q, ref)):
        excess = np.abs(got - q_ref) - bound
        assert (excess <= 0.0).all(), (axis, np.unravel_index(excess.argmax(), excess.shape), excess.max())
    if g is not None:
        for face, fq, fp in _face_entries(n)[::3 if geom == (1, 162) else 1]:
            bad = g.copy()
            bad[face, fq, fp] = np.nan if face & 1 else np.inf
            _run_flux(P, K, bad, wall, kappa, mask, NOT_FINITE)


# ---------------------------------------------------------------- refusals
def _refusals(P, lv, where, mem, bnd):
    """[(what, code)] of every refused call, in one order on either side; the outputs are pre-filled with NaN by the caller."""
    lib, L, n = lv.b.lib, lv.ptr, P.n
    cell, face_i = mem.put(np.ones((n,) * 3)), mem.put(np.ones(DH.dense_shape(P.geo, H.DENSE_FACE_I)))
    g, wall = bnd.put(np.ones((6, n, n))), bnd.put(np.ones((6, n, n)))
    phi = bnd.put(np.full((6, n, n), np.nan))
    out = [mem.put(np.full(DH.dense_shape(P.geo, H.DENSE_FACE_I + a), np.nan)) for a in range(3)]
    dst = mem.put(np.full((n,) * 3, np.nan))
    F, POS = H.DENSE_CHECK_FINITE, H.DENSE_CHECK_POSITIVE
    any_positive = ctypes.c_int(-1)
    calls = [
        ("pack: layout 4", lambda: lib.hpgmg_dense_pack(L, OUT, cell, where, 4, F)),
        ("pack: layout -1", lambda: lib.hpgmg_dense_pack(L, OUT, cell, where, -1, F)),
        ("pack: null array", lambda: lib.hpgmg_dense_pack(L, OUT, None, where, H.DENSE_CELL, F)),
        ("pack: id -1", lambda: lib.hpgmg_dense_pack(L, -1, cell, where, H.DENSE_CELL, F)),
        ("pack: id past the last", lambda: lib.hpgmg_dense_pack(L, lv.num_vectors, cell, where, H.DENSE_CELL, F)),
        ("pack: where 2", lambda: lib.hpgmg_dense_pack(L, OUT, cell, 2, H.DENSE_CELL, F)),
        ("pack_walls: a cell layout", lambda: lib.hpgmg_dense_pack_walls(L, OUT, cell, where, H.DENSE_CELL, POS, 3, wall)),
        ("pack_walls: layout 4", lambda: lib.hpgmg_dense_pack_walls(L, OUT, face_i, where, 4, POS, 3, wall)),
        ("pack_walls: mask 64", lambda: lib.hpgmg_dense_pack_walls(L, OUT, face_i, where, H.DENSE_FACE_I, POS, 64, wall)),
        ("pack_walls: mask without wall", lambda: lib.hpgmg_dense_pack_walls(L, OUT, face_i, where, H.DENSE_FACE_I, POS, 3, None)),
        ("pack_walls: null array", lambda: lib.hpgmg_dense_pack_walls(L, OUT, None, where, H.DENSE_FACE_I, POS, 3, wall)),
        ("pack_walls: id past the last", lambda: lib.hpgmg_dense_pack_walls(L, lv.num_vectors, face_i, where, H.DENSE_FACE_I, POS, 3, wall)),
        ("unpack: null array", lambda: lib.hpgmg_dense_unpack(L, U_ID, None, where)),
        ("unpack: id -1", lambda: lib.hpgmg_dense_unpack(L, -1, dst, where)),
        ("unpack: id past the last", lambda: lib.hpgmg_dense_unpack(L, lv.num_vectors, dst, where)),
        ("unpack: where 2", lambda: lib.hpgmg_dense_unpack(L, U_ID, dst, 2)),
        ("pack_lifted: null g", lambda: lib.hpgmg_dense_pack_lifted(L, OUT, cell, where, None, B_COEF)),
        ("pack_lifted: null f", lambda: lib.hpgmg_dense_pack_lifted(L, OUT, None, where, g, B_COEF)),
        ("pack_lifted: id past the last", lambda: lib.hpgmg_dense_pack_lifted(L, lv.num_vectors, cell, where, g, B_COEF)),
        ("pack_lifted_faces: mask 64", lambda: lib.hpgmg_dense_pack_lifted_faces(L, OUT, cell, where, g, B_COEF, 64, wall)),
        ("pack_lifted_faces: mask without wall", lambda: lib.hpgmg_dense_pack_lifted_faces(L, OUT, cell, where, g, B_COEF, 5, None)),
        ("pack_lifted_robin: mask -1", lambda: lib.hpgmg_dense_pack_lifted_robin(L, OUT, cell, where, g, B_COEF, -1, wall, wall)),
        ("pack_lifted_robin: mask without wall", lambda: lib.hpgmg_dense_pack_lifted_robin(L, OUT, cell, where, g, B_COEF, 5, None, wall)),
        ("flux_faces: mask 64", lambda: lib.hpgmg_boundary_flux_faces(L, phi, g, B_COEF, 64, wall)),
        ("flux_faces: mask without wall", lambda: lib.hpgmg_boundary_flux_faces(L, phi, g, B_COEF, 5, None)),
        ("flux_robin: mask 64", lambda: lib.hpgmg_boundary_flux_robin(L, phi, g, B_COEF, 64, wall, wall)),
        ("flux_robin: mask without wall", lambda: lib.hpgmg_boundary_flux_robin(L, phi, g, B_COEF, 5, None, wall)),
        ("unpack_flux: mask 64", lambda: lib.hpgmg_dense_unpack_flux(L, U_ID, g, B_COEF, 64, wall, None, *out, where)),
        ("unpack_flux: mask without wall", lambda: lib.hpgmg_dense_unpack_flux(L, U_ID, g, B_COEF, 5, None, None, *out, where)),
        ("unpack_flux: null array", lambda: lib.hpgmg_dense_unpack_flux(L, U_ID, g, B_COEF, 0, None, None, out[0], None, out[2], where)),
        ("unpack_flux: id -1", lambda: lib.hpgmg_dense_unpack_flux(L, -1, g, B_COEF, 0, None, None, *out, where)),
        ("unpack_flux: id past the last", lambda: lib.hpgmg_dense_unpack_flux(L, lv.num_vectors, g, B_COEF, 0, None, None, *out, where)),
        ("unpack_flux: where 2", lambda: lib.hpgmg_dense_unpack_flux(L, U_ID, g, B_COEF, 0, None, None, *out, 2)),
        ("check_kappa: null array", lambda: lib.hpgmg_boundary_check_kappa(L, None, where, 63, ctypes.byref(any_positive))),
        ("check_kappa: mask 64", lambda: lib.hpgmg_boundary_check_kappa(L, g if where == H.WHERE_PLUGIN else cell, where, 64, ctypes.byref(any_positive))),
        ("check_kappa: where 2", lambda: lib.hpgmg_boundary_check_kappa(L, g, 2, 63, ctypes.byref(any_positive))),
    ]
    codes = [(what, call()) for what, call in calls]
    outputs = [mem.get(dst, (n,) * 3), bnd.get(phi, (6, n, n))] + [mem.get(p, DH.dense_shape(P.geo, H.DENSE_FACE_I + a)) for a, p in enumerate(out)]
    return codes, outputs, any_positive.value


def test_refusals(libs, pair_of):
    """A bad layout, a mask of 64, a mask without `wall`, a null array, a vector id out of range, a `where` that is none: -1 from both sides, and
    the NaN pre-fill of the vector and of every output array untouched."""
    _, _, K = libs
    P = pair_of((3, 12))
    seen = {}
    for key, lv, where, mem in P.sides(K):
        bnd = _Mem(lv.b.lib)
        try:
            lv.write_all(OUT, P.nan)
            codes, outputs, positive = _refusals(P, lv, where, mem, bnd)
            assert all(np.isnan(x).all() for x in outputs), key
            assert np.isnan(lv.read_all(OUT)).all(), key
            assert positive == 0, key                       # a refused check_kappa still clears any_positive
            seen[key] = codes
        finally:
            mem.free(); bnd.free()
    assert seen["hip-host"] == seen["hip-device"] == seen["oracle"]
    assert [code for _, code in seen["oracle"]] == [-1] * len(seen["oracle"]), seen["oracle"]


def test_a_periodic_level_refuses_boundary_data(libs, pair_of):
    """g or a mask on a periodic level: refused on both sides alike, as are pack_walls and the lifted pack; the face arrays there are (N, N, N)."""
    _, _, K = libs
    P = pair_of(PERIODIC)
    n = P.n
    assert all(DH.dense_shape(P.geo, layout) == (n, n, n) for layout in DH.LAYOUTS)
    seen = {}
    for key, lv, where, mem in P.sides(K):
        bnd = _Mem(lv.b.lib)
        lib, L = lv.b.lib, lv.ptr
        try:
            lv.write_all(OUT, P.nan)
            g, wall = bnd.put(np.ones((6, n, n))), bnd.put(np.ones((6, n, n)))
            cell = mem.put(np.ones((n, n, n)))
            out = [mem.put(np.full((n, n, n), np.nan)) for _ in range(3)]
            seen[key] = [lib.hpgmg_dense_unpack_flux(L, U_ID, g, B_COEF, 0, None, None, *out, where),
                         lib.hpgmg_dense_unpack_flux(L, U_ID, None, B_COEF, 3, wall, None, *out, where),
                         lib.hpgmg_dense_pack_walls(L, OUT, cell, where, H.DENSE_FACE_I, H.DENSE_CHECK_FINITE, 3, wall),
                         lib.hpgmg_dense_pack_lifted(L, OUT, cell, where, g, B_COEF)]
            assert all(np.isnan(mem.get(p, (n, n, n))).all() for p in out), key
            assert np.isnan(lv.read_all(OUT)).all(), key
        finally:
            mem.free(); bnd.free()
    assert seen["hip-host"] == seen["hip-device"] == seen["oracle"] == [-1] * 4
