"""The NumPy restatements of tests/dense_hooks_lib.py pinned on the CPU oracle (the host defaults of host/hooks_host.inc), before
tests/test_gpu_dense_hooks.py trusts them: pack (four layouts, Dirichlet and periodic), pack_walls, unpack, boundary_restrict, store_walls and
check_kappa, bit for bit over whole padded boxes and whole arrays, every output pre-filled with NaN (the wall array: a sentinel), at the geometries
of the GPU test -- (1, 162), (3, 12), (17, 2), (1, 6), (1, 1) and a periodic (3, 12).  Every build has -ffp-contract=off: nothing has a tolerance.

That the pin has teeth is shown once, in test_a_restatement_with_j_and_k_swapped_fails_the_pin: the pack and the unpack restatements fed (pack) or
read (unpack) with j and k exchanged do not give the oracle's bits.
"""
import ctypes

import numpy as np
import pytest

import dense_hooks_lib as DH
import hpgmg_amd as H
from hpgmg_testlib import VARIANTS, seeded_field

ID = H.VECTOR_U
BETAS = (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
SENTINEL = -7.0
_levels = {}


@pytest.fixture
def level_of(oracle):
    """level_of(geom, periodic=False): an oracle level with the ten vectors the hooks name, and its Geo; kept for the module."""
    def get(geom, periodic=False):
        key = geom + (periodic,)
        if key not in _levels:
            oracle.configure(**VARIANTS["7pt-cheby-helm"])
            lv = oracle.level(*geom, num_vectors=DH.VECTORS, bc=H.BC_PERIODIC if periodic else H.BC_DIRICHLET)
            assert lv.num_boxes == geom[0] ** 3 and lv.box_dim == geom[1] and lv.ghosts == 1
            _levels[key] = (lv, DH.Geo(lv, periodic))
        return _levels[key]
    return get


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    while _levels:
        _levels.popitem()[1][0].destroy()


def _nan_fill(lv, vid):
    lv.write_all(vid, np.full((lv.num_boxes, lv.volume), np.nan))


def _source(geo, layout, seed):
    """Random values, some of them exactly 0.0 and -0.0 (a pack copies the sign of a zero)."""
    rng = np.random.default_rng(seed)
    src = rng.random(DH.dense_shape(geo, layout)) * 2.0 - 1.0
    flat = src.reshape(-1)
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 50))] = -0.0
    flat[rng.integers(0, flat.size, size=max(1, flat.size // 50))] = 0.0
    return src


class _Mem:
    """Boundary arrays in the oracle's plugin memory (hpgmg_vector_alloc)."""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, a):
        if a is None:
            return None
        p = self.lib.hpgmg_vector_alloc(a.size)
        self.lib.hpgmg_vector_upload(p, np.ascontiguousarray(a).ctypes.data, a.size)
        self.ptrs.append(p)
        return p

    def get(self, p, shape):
        out = np.empty(shape)
        self.lib.hpgmg_vector_download(out.ctypes.data, p, out.size)
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.hpgmg_vector_free(p)
        self.ptrs = []


def test_the_162_box_is_above_one_trip_and_161_is_not(level_of):
    lv, geo = level_of((1, 162))
    assert (geo.jS, geo.kS, geo.vol) == (164, 26896, 4410944)
    assert geo.vol > DH.TRIP and 162 ** 3 > DH.TRIP > 161 ** 3
    first_of_plane = geo.offsets(1, 1, 162)[:, 0, 0] - geo.g * (1 + geo.jS)                # of the padded plane of interior plane k
    assert first_of_plane[156] >= DH.TRIP > first_of_plane[0]                               # interior k >= 156: reached by the second trip only


@pytest.mark.parametrize("layout", DH.LAYOUTS)
@pytest.mark.parametrize("geom", DH.GEOMS + [(3, 12, "periodic")], ids=lambda g: DH.geom_id(g[:2]) + ("-periodic" if len(g) > 2 else ""))
def test_pack(oracle, level_of, geom, layout):
    lv, geo = level_of(geom[:2], len(geom) > 2)
    src = _source(geo, layout, 100 + geom[1] + layout)
    _nan_fill(lv, ID)
    assert oracle.lib.hpgmg_dense_pack(lv.ptr, ID, src.ctypes.data, H.WHERE_HOST, layout, H.DENSE_CHECK_FINITE) == 0
    got, want = lv.read_all(ID), DH.pack(geo, src, layout)
    assert DH.same_bits(got, want), DH.first_differences(got, want)
    back = DH.unpack(geo, want, layout)                     # the gather undoes the pack: every entry of the array is determined by one box
    assert DH.same_bits(back, src)


@pytest.mark.parametrize("geom", DH.GEOMS + [(3, 12, "periodic")], ids=lambda g: DH.geom_id(g[:2]) + ("-periodic" if len(g) > 2 else ""))
def test_unpack(oracle, level_of, geom):
    lv, geo = level_of(geom[:2], len(geom) > 2)
    boxes = seeded_field(lv, 300 + geom[1])                 # ghost zones and padding differ from the interior
    lv.write_all(ID, boxes)
    dst = np.full((geo.n,) * 3, np.nan)
    assert oracle.lib.hpgmg_dense_unpack(lv.ptr, ID, dst.ctypes.data, H.WHERE_HOST) == 0
    want = DH.unpack(geo, boxes)
    assert DH.same_bits(dst, want), DH.first_differences(dst, want)
    assert DH.same_bits(dst, lv.interior(ID))


def test_a_restatement_with_j_and_k_swapped_fails_the_pin(oracle, level_of):
    lv, geo = level_of((3, 12))
    src = _source(geo, H.DENSE_CELL, 77)
    _nan_fill(lv, ID)
    assert oracle.lib.hpgmg_dense_pack(lv.ptr, ID, src.ctypes.data, H.WHERE_HOST, H.DENSE_CELL, H.DENSE_CHECK_FINITE) == 0
    got = lv.read_all(ID)
    assert DH.same_bits(got, DH.pack(geo, src, H.DENSE_CELL))
    assert not DH.same_bits(got, DH.pack(geo, np.ascontiguousarray(src.transpose(1, 0, 2)), H.DENSE_CELL))      # src[gj][gk][gi]
    dst = np.full((geo.n,) * 3, np.nan)
    assert oracle.lib.hpgmg_dense_unpack(lv.ptr, ID, dst.ctypes.data, H.WHERE_HOST) == 0
    assert DH.same_bits(dst, DH.unpack(geo, got))
    assert not DH.same_bits(dst, np.ascontiguousarray(DH.unpack(geo, got).transpose(1, 0, 2)))                  # dst[gj][gk][gi]


@pytest.mark.parametrize("axis", range(3))
@pytest.mark.parametrize("geom", DH.GEOMS, ids=DH.geom_id)
def test_pack_walls(oracle, level_of, geom, axis):
    lv, geo = level_of(geom)
    layout = H.DENSE_FACE_I + axis
    src = _source(geo, layout, 500 + geom[1] + axis)
    mem = _Mem(oracle.lib)
    try:
        for mask in DH.wall_masks(axis):
            before = np.full((6, geo.n, geo.n), SENTINEL)
            pw = mem.put(before)
            _nan_fill(lv, BETAS[axis])
            assert oracle.lib.hpgmg_dense_pack_walls(lv.ptr, BETAS[axis], src.ctypes.data, H.WHERE_HOST, layout, H.DENSE_CHECK_FINITE, mask, pw) == 0
            want, want_wall = DH.pack_walls(geo, src, layout, mask, before)
            got, got_wall = lv.read_all(BETAS[axis]), mem.get(pw, before.shape)
            assert DH.same_bits(got, want), (mask, DH.first_differences(got, want))
            assert DH.same_bits(got_wall, want_wall), (mask, DH.first_differences(got_wall, want_wall))
            owned = [2 * axis + side for side in (0, 1) if (mask >> (2 * axis + side)) & 1]
            assert (np.delete(got_wall, owned, axis=0) == SENTINEL).all()          # what the array does not own keeps its pre-fill
            mem.free()
    finally:
        mem.free()


@pytest.mark.parametrize("fine,coarse", [((1, 162), (1, 81)), ((3, 12), (3, 6)), ((17, 2), (17, 1)), ((1, 6), (1, 3)), ((1, 2), (1, 1))],
                         ids=lambda g: DH.geom_id(g))
def test_restrict(oracle, fine, coarse):
    oracle.configure(**VARIANTS["7pt-cheby-helm"])
    lf, lc = oracle.level(*fine, num_vectors=1), oracle.level(*coarse, num_vectors=1)
    mem = _Mem(oracle.lib)
    try:
        nf, nc = lf.dim, lc.dim
        assert nf == 2 * nc
        g_f = np.random.default_rng(600 + nf).random((6, nf, nf)) * 4.0 - 2.0
        pc = mem.put(np.full((6, nc, nc), np.nan))
        oracle.lib.hpgmg_boundary_restrict(lc.ptr, pc, lf.ptr, mem.put(g_f))
        got, want = mem.get(pc, (6, nc, nc)), DH.restrict(g_f)
        assert DH.same_bits(got, want), DH.first_differences(got, want)
    finally:
        mem.free()
        lf.destroy(); lc.destroy()


@pytest.mark.parametrize("walls", DH.WALLS, ids=DH.geom_id)
@pytest.mark.parametrize("geom", DH.GEOMS, ids=DH.geom_id)
def test_store_walls(oracle, level_of, geom, walls):
    _, mask, with_kappa = walls
    lv, geo = level_of(geom)
    rng = np.random.default_rng(700 + geom[1] + mask)
    betas = [np.abs(seeded_field(lv, 710 + geom[1] + a)) + 0.5 for a in range(3)]
    wall = rng.random((6, geo.n, geo.n)) + 0.5
    kappa = rng.random((6, geo.n, geo.n)) * 3.0 if with_kappa else None
    if kappa is not None:
        kappa.reshape(-1)[::3] = 0.0                        # a Robin wall with kappa = 0.0 is a Neumann wall: beta 0.0
    for vid, b in zip(BETAS, betas):
        lv.write_all(vid, b)
    mem = _Mem(oracle.lib)
    try:
        oracle.lib.hpgmg_boundary_store_walls(lv.ptr, mem.put(wall), mem.put(kappa), mask)
    finally:
        mem.free()
    want = DH.store_walls(geo, betas, wall, kappa, lv.h, mask)
    changed = 0
    for vid, w, b in zip(BETAS, want, betas):
        got = lv.read_all(vid)
        assert DH.same_bits(got, w), (vid, DH.first_differences(got, w))
        changed += int((w != b).sum())
    assert changed == bin(mask).count("1") * geo.n * geo.n          # every entry of a masked wall, and nothing else (no beta equals its wall value)


@pytest.mark.parametrize("case", DH.KAPPA_CASES, ids=lambda c: c[0])
@pytest.mark.parametrize("geom", [(3, 12), (1, 6), (1, 1)], ids=DH.geom_id)
def test_check_kappa(oracle, level_of, geom, case):
    _, plants, robin_mask, status, positive = case
    lv, geo = level_of(geom)
    kappa = DH.kappa_case(geo.n, plants)
    assert DH.check_kappa(kappa, robin_mask) == (status, positive)
    mem = _Mem(oracle.lib)
    try:
        for where, p in ((H.WHERE_HOST, kappa.ctypes.data), (H.WHERE_PLUGIN, mem.put(kappa))):
            any_positive = ctypes.c_int(-1)
            assert oracle.lib.hpgmg_boundary_check_kappa(lv.ptr, p, where, robin_mask, ctypes.byref(any_positive)) == status
            assert any_positive.value == positive
    finally:
        mem.free()
